"""Host-side mirror of the `lynse._core` surface for the FLAT / IVF-Flat hot path.

Same class / function names, argument meaning and error behaviour as the reference's PyO3 module
(src/python/mod.rs) for the entry points on this path, so the reference's own benchmarks and tests
(`benchmarks/flat_search_bench.py`, `tests/standard_tests/test_backend.py`) read unchanged against it:

    FlatIndex            src/python/mod.rs:1942-2047   (FlatMmap)
    IvfFlatIndex         src/python/mod.rs:2056-2156   (IvfFlatMmap)
    py_compute_distance  src/python/mod.rs:2161-2185
    py_top_k_search      src/python/mod.rs:2189-2223
    DatabaseManager / Collection / SearchResult  (the subset `flat_search_bench.py:43-96` drives,
                         src/python/mod.rs:984-1005, :1135-1150, :1171-1193, :1343, :1383-1408,
                         :1876-1921, :2235-2418)

All arithmetic happens in liblynse_hip.so on the GPU; nothing here computes distances on the host.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, lib
from .fields import FieldFilter, FieldTable, parse_where
from .vector_fields import (DEFAULT_VECTOR_FIELD_NAME, KNOWN_INDEX_MODES, ROWMAP_NONE, NamedVectorField, RowMap, field_mode_kind,
                            normalize_field_index_mode, resolve_named_vector_metric, validate_vector_field_name, vector_dtype_name,
                            words_of_rows)

_METRIC_IS_BINARY = {_lib.METRIC_HAMMING, _lib.METRIC_JACCARD, _lib.METRIC_DICE, _lib.METRIC_TANIMOTO}


def visible_devices() -> list:
    """`LYNSE_HIP_DEVICES` (the build's one addition to the reference's env-only configuration, next to `RAYON_NUM_THREADS` /
    `LYNSE_SEGMENT_TARGET_BYTES`): a comma-separated list of HIP device ordinals this process may use, e.g. "2,3" — rank r of a node-local
    job takes entry r % len.  Unset: every device the runtime shows."""
    v = os.environ.get("LYNSE_HIP_DEVICES", "").strip()
    if v:
        try:
            devs = [int(x) for x in v.split(",") if x.strip() != ""]
        except ValueError:
            raise ValueError(f"LYNSE_HIP_DEVICES must be a comma-separated list of device ordinals, got {v!r}") from None
        if not devs or min(devs) < 0:
            raise ValueError(f"LYNSE_HIP_DEVICES must name at least one non-negative device ordinal, got {v!r}")
        return devs
    return list(range(max(_lib.device_count(), 1)))


def default_device() -> int:
    """Device ordinal: LYNSE_HIP_DEVICE, else entry LOCAL_RANK % len of LYNSE_HIP_DEVICES, else LOCAL_RANK (one process per GPU), else the
    first entry of LYNSE_HIP_DEVICES, else 0."""
    v = os.environ.get("LYNSE_HIP_DEVICE")
    if v is not None and v != "":
        return int(v)
    rank = os.environ.get("LOCAL_RANK")
    if os.environ.get("LYNSE_HIP_DEVICES", "").strip():
        devs = visible_devices()
        return devs[int(rank) % len(devs)] if rank not in (None, "") else devs[0]
    if rank not in (None, ""):
        return int(rank)
    return 0


def metric_from_str(metric: str) -> int:
    """DistanceMetric::from_str (src/distance/mod.rs:39-63); unknown -> ValueError("Unknown metric: ...")."""
    out = C.c_int(-1)
    check(lib.lynse_hip_metric_from_str(str(metric).encode(), C.byref(out)))
    return out.value


def metric_from_index_mode(mode: str) -> int:
    out = C.c_int(-1)
    check(lib.lynse_hip_metric_from_index_mode(str(mode).encode(), C.byref(out)))
    return out.value


def ivf_quantizer_of(mode: str) -> Optional[str]:
    """The quantizer an `IVF-*` index mode names (src/index/mod.rs:361-385): None for IVF-Flat and the binary modes (their
    quantizer follows from the metric), "sq8" for IVF-{IP,L2,COS,COSINE}-SQ8 (ip / l2 / cosine only); PQ is not built."""
    parts = str(mode).upper().split("-")
    if any(t == "PQ" or (t.startswith("PQ") and t[2:].isdigit()) for t in parts):   # IVF-*-PQ and IVF-*-PQ<n>
        raise NotImplementedError("quantized IVF variants other than SQ8 (PQ) are outside this path")
    if "SQ8" in parts:
        if metric_from_index_mode(mode) not in (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE):
            raise NotImplementedError(f"{mode}: IVF-*-SQ8 is defined for ip / l2 / cosine")
        return "sq8"
    return None


PQ_OVERSAMPLE = 32   # engine.rs PQ_OVERSAMPLE / pq_mmap.rs DEFAULT_OVERSAMPLE


def parse_n_subspaces(index_type: str, dim: int) -> int:
    """parse_n_subspaces (src/storage/pq_mmap.rs:1107-1128): the digits after "PQ" when they are > 0 and divide `dim`, else the first
    divisor of `dim` in [16, 8, 32, 4, 12, 24, 6, 2, 1]."""
    s = str(index_type).upper()
    pos = s.find("PQ")
    if pos >= 0:
        digits = ""
        for ch in s[pos + 2:]:
            if not ch.isdigit():
                break
            digits += ch
        if digits:
            n = int(digits)
            if n > 0 and dim % n == 0:
                return n
    for c in (16, 8, 32, 4, 12, 24, 6, 2, 1):
        if dim % c == 0:
            return c
    return 1


def flat_pq_mode(mode: str) -> bool:
    """True for FLAT-{IP,L2,COS,COSINE}-PQ[<n>]; binary metrics are refused (the other FLAT quantisers: flat_rabitq_mode)."""
    parts = str(mode).upper().split("-")
    if not parts or parts[0] != "FLAT":
        return False
    if not any(p.startswith("PQ") and p[2:].isdigit() or p == "PQ" for p in parts[1:]):
        return False
    if metric_from_index_mode(mode) not in (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE):
        raise NotImplementedError(f"{mode}: FLAT-*-PQ is defined for ip / l2 / cosine")
    return True


RABITQ_OVERSAMPLE = 200   # rabitq_mmap.rs DEFAULT_OVERSAMPLE
RABITQ_INDEX_FILE = "rabitq_index.bin"


def flat_rabitq_mode(mode: str) -> bool:
    """True for FLAT-{IP,L2,COS,COSINE}-RABITQ; binary metrics are refused, and so is the remaining FLAT quantiser (PolarVec)."""
    parts = str(mode).upper().split("-")
    if not parts or parts[0] != "FLAT":
        return False
    if "POLARVEC" in parts[1:]:
        raise NotImplementedError("PolarVec flat modes are outside this path (SURVEY.md §2)")
    if "RABITQ" not in parts[1:]:
        return False
    if metric_from_index_mode(mode) not in (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE):
        raise NotImplementedError(f"{mode}: FLAT-*-RABITQ is defined for ip / l2 / cosine")
    return True


POLARVEC_OVERSAMPLE = 20   # polarvec_mmap.rs DEFAULT_OVERSAMPLE
POLARVEC_DEFAULT_BITS = 4
POLARVEC_INDEX_FILE = "polarvec_index.bin"


def flat_polarvec_mode(mode: str) -> Optional[int]:
    """The bit count of FLAT-{IP,L2,COS,COSINE}-POLARVEC<digits> (any letter case), None for a mode without such a token.  Digits
    outside 1..8 mean 4 (parse_bits, polarvec_mmap.rs:1269-1282); binary and additive metrics are refused.  The reference reads the
    bare token POLARVEC as 4 bits too; this build refuses it, as flat_rabitq_mode always has: ask for POLARVEC4."""
    parts = str(mode).upper().split("-")
    if not parts or parts[0] != "FLAT":
        return None
    if "POLARVEC" in parts[1:]:
        raise NotImplementedError(f"{mode}: name the bit count (FLAT-*-POLARVEC4); the bare token is refused (DESIGN.md §23)")
    tok = next((p for p in parts[1:] if p.startswith("POLARVEC") and p[8:].isdigit()), None)
    if tok is None:
        return None
    if metric_from_index_mode(mode) not in (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE):
        raise NotImplementedError(f"{mode}: FLAT-*-POLARVEC is defined for ip / l2 / cosine")
    bits = int(tok[8:])
    return bits if 1 <= bits <= 8 else POLARVEC_DEFAULT_BITS


SPANN_MODES = {"SPANN-IP": (_lib.METRIC_IP, False), "SPANN-L2": (_lib.METRIC_L2, False), "SPANN-COS": (_lib.METRIC_COSINE, False),
               "SPANN-COSINE": (_lib.METRIC_COSINE, False), "SPANN-IP-SQ8": (_lib.METRIC_IP, True), "SPANN-L2-SQ8": (_lib.METRIC_L2, True),
               "SPANN-COS-SQ8": (_lib.METRIC_COSINE, True), "SPANN-COSINE-SQ8": (_lib.METRIC_COSINE, True)}
SPANN_DEFAULT_REPLICAS = 1   # spann::DEFAULT_REPLICA_COUNT


def spann_mode_of(mode: str) -> Optional[tuple]:
    """The SPANN index modes (src/index/mod.rs:387-419): (metric id, sq8) for SPANN-{IP,L2,COS,COSINE}[-SQ8], None for a mode that is
    not SPANN-*; any other SPANN-* name is refused as the reference refuses an unknown index type (ValueError, InvalidArgument)."""
    u = str(mode).upper()
    if not u.startswith("SPANN"):
        return None
    if u not in SPANN_MODES:
        raise ValueError(f"Invalid argument: Unknown index type: {mode}")
    return SPANN_MODES[u]


ADDITIVE_METRICS = (_lib.METRIC_L1, _lib.METRIC_CHEBYSHEV, _lib.METRIC_CANBERRA, _lib.METRIC_BRAY_CURTIS)
# resolve_domain_index_type's flat names of the additive metrics (src/index/mod.rs:426-495)
ADDITIVE_FLAT_MODES = {"FLAT-L1": _lib.METRIC_L1, "FLAT-MANHATTAN": _lib.METRIC_L1, "FLAT-CITYBLOCK": _lib.METRIC_L1,
                       "FLAT-CHEBYSHEV": _lib.METRIC_CHEBYSHEV, "FLAT-CHEBYCHEV": _lib.METRIC_CHEBYSHEV, "FLAT-LINF": _lib.METRIC_CHEBYSHEV,
                       "FLAT-CANBERRA": _lib.METRIC_CANBERRA, "FLAT-BRAY-CURTIS": _lib.METRIC_BRAY_CURTIS,
                       "FLAT-BRAYCURTIS": _lib.METRIC_BRAY_CURTIS}
# supports_flat_approx (src/distance/mod.rs:177-188): the metrics `search(approx=True)` takes the approximate flat search under
APPROX_FLAT_METRICS = (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE) + ADDITIVE_METRICS


def normalize_eps(eps: Optional[float]) -> float:
    """normalize_eps (approx_search.rs:113-119): None, non-finite or <= 0 -> 1e-4, else max(eps, 1e-8), as f32."""
    return float(lib.lynse_hip_normalize_eps(np.float32(np.nan if eps is None else eps)))


def round_distances_to_eps(dists, eps: float) -> np.ndarray:
    """round_distances_to_eps (approx_search.rs:123-143) -> a new f32 array: (v / eps).round() * eps in f32, half away from zero (not
    numpy's half-to-even); a non-finite value, quotient or product passes through."""
    out = np.array(dists, dtype=np.float32).reshape(-1)
    if out.size:
        lib.lynse_hip_round_distances_to_eps(_ptr(out), out.size, np.float32(eps))
    return out


def additive_mode_of(mode: str) -> Optional[int]:
    """The metric id of a FLAT-{L1,MANHATTAN,CITYBLOCK,CHEBYSHEV,CHEBYCHEV,LINF,CANBERRA,BRAY-CURTIS,BRAYCURTIS} index mode (any letter
    case), None for a mode that names none of the four additive metrics; any other mode naming one (FLAT-L1-SQ8, IVF-L1, SPANN-CHEBYSHEV ...)
    is refused as the reference refuses an unknown index type (ValueError, InvalidArgument)."""
    u = str(mode).upper()
    if u in ADDITIVE_FLAT_MODES:
        return ADDITIVE_FLAT_MODES[u]
    try:
        m = metric_from_index_mode(u)
    except (ValueError, NotImplementedError):
        return None
    if m in ADDITIVE_METRICS:
        raise ValueError(f"Invalid argument: Unknown index type: {mode}")
    return None


def spann_build_options(params: Optional[dict]) -> dict:
    """IndexBuildOptions for a SPANN mode (src/index/mod.rs:502-542, :626-655): n_clusters (alias n_centroids) = 256, nprobe = 32,
    replica_count = 1; a value of 0 is refused with ValueError("Invalid argument: <name> must be greater than 0")."""
    p = dict(params or {})
    if "n_centroids" in p and "n_clusters" not in p:
        p["n_clusters"] = p.pop("n_centroids")
    out = {}
    for name, default in (("n_clusters", 256), ("nprobe", 32), ("replica_count", SPANN_DEFAULT_REPLICAS)):
        v = p.get(name)
        if v is not None and int(v) == 0:
            raise ValueError(f"Invalid argument: {name} must be greater than 0")
        out[name] = default if v is None else int(v)
    return out


HNSW_MODES = {"HNSW-IP": _lib.METRIC_IP, "HNSW-L2": _lib.METRIC_L2, "HNSW-COS": _lib.METRIC_COSINE, "HNSW-COSINE": _lib.METRIC_COSINE}
HNSW_DEFAULTS = {"m": 16, "ef_construction": 128, "ef_search": 50}   # src/index/mod.rs:503, :681-686
HNSW_SEED = 42
# IndexBuildOptions::is_known_key (src/index/mod.rs:572-592)
INDEX_BUILD_KEYS = ("n_clusters", "n_centroids", "m", "ef_construction", "ef_search", "max_level", "r", "l", "alpha", "max_degree", "nprobe",
                    "replica_count")


def hnsw_mode_of(mode: str) -> Optional[int]:
    """The metric id of HNSW-{IP,L2,COS,COSINE} (any letter case), None for every other mode — HNSW-*-SQ8 and HNSW over the domain
    metrics keep the answers they had (outside this path); the DiskANN modes are diskann_mode_of's."""
    return HNSW_MODES.get(str(mode).upper())


DISKANN_MODES = {"DISKANN-L2": _lib.METRIC_L2, "DISKANN-COS": _lib.METRIC_COSINE, "DISKANN-COSINE": _lib.METRIC_COSINE}
DISKANN_DEFAULTS = {"r": 16, "l": 64, "alpha": 1.2}   # src/index/mod.rs:504-506
DISKANN_SEED = 42


def diskann_mode_of(mode: str) -> Optional[int]:
    """The metric id of DISKANN-{L2,COS,COSINE} (any letter case), None for every other mode — DISKANN-IP (the reference leaves Vamana's
    rule for it) and the -PQ* / -SQ8 names keep the answers they had (outside this path)."""
    return DISKANN_MODES.get(str(mode).upper())


def diskann_build_options(params: Optional[dict]) -> dict:
    """IndexBuildOptions for a DiskANN mode (src/index/mod.rs:545-655): r = 16, l = 64, alpha = 1.2, max_degree = r.  An unknown key, a
    value of 0 and a bad alpha are refused in validate()'s order with the reference's messages (ValueError, InvalidArgument); keys of the
    other index families are ignored (filtered_for).  The bounds on r and l are the library's (LYNSE_ERR_UNSUPPORTED)."""
    p = dict(params or {})
    for key in p:
        if key not in INDEX_BUILD_KEYS:
            raise ValueError(f"Invalid argument: unknown index build parameter '{key}'; supported keys: {', '.join(INDEX_BUILD_KEYS)}")
    if "n_centroids" in p and "n_clusters" not in p:
        p["n_clusters"] = p.pop("n_centroids")
    for name in ("n_clusters", "m", "ef_construction", "ef_search", "r", "l", "max_degree", "nprobe", "replica_count"):   # validate()'s order
        if p.get(name) is not None and int(p[name]) == 0:
            raise ValueError(f"Invalid argument: {name} must be greater than 0")
    alpha = p.get("alpha")
    if alpha is not None and not (np.isfinite(np.float32(alpha)) and np.float32(alpha) >= 1.0):
        raise ValueError("Invalid argument: alpha must be a finite value >= 1.0")
    out = {name: (DISKANN_DEFAULTS[name] if p.get(name) is None else int(p[name])) for name in ("r", "l")}
    for name, v in out.items():
        if v < 0:
            raise ValueError(f"Invalid argument: invalid index build parameter value: {name} = {v}")
    out["alpha"] = float(np.float32(DISKANN_DEFAULTS["alpha"] if alpha is None else alpha))
    md = p.get("max_degree")
    if md is not None and int(md) < 0:
        raise ValueError(f"Invalid argument: invalid index build parameter value: max_degree = {md}")
    out["max_degree"] = out["r"] if md is None else int(md)
    return out


def hnsw_build_options(params: Optional[dict]) -> dict:
    """IndexBuildOptions for an HNSW mode (src/index/mod.rs:545-655): m = 16, ef_construction = 128, ef_search = 50, max_level = None
    (uncapped).  An unknown key and a value of 0 are refused with the reference's messages (ValueError, InvalidArgument); keys of the
    other index families are ignored (filtered_for).  The bounds on m and the ef values are the library's (LYNSE_ERR_UNSUPPORTED)."""
    p = dict(params or {})
    for key in p:
        if key not in INDEX_BUILD_KEYS:
            raise ValueError(f"Invalid argument: unknown index build parameter '{key}'; supported keys: {', '.join(INDEX_BUILD_KEYS)}")
    if "n_centroids" in p and "n_clusters" not in p:
        p["n_clusters"] = p.pop("n_centroids")
    for name in ("n_clusters", "m", "ef_construction", "ef_search", "r", "l", "max_degree", "nprobe", "replica_count"):   # validate()'s order
        if p.get(name) is not None and int(p[name]) == 0:
            raise ValueError(f"Invalid argument: {name} must be greater than 0")
    out = {name: (default if p.get(name) is None else int(p[name])) for name, default in HNSW_DEFAULTS.items()}
    for name, v in out.items():
        if v < 0:
            raise ValueError(f"Invalid argument: invalid index build parameter value: {name} = {v}")
    ml = p.get("max_level")
    if ml is not None and int(ml) < 0:
        raise ValueError(f"Invalid argument: invalid index build parameter value: max_level = {ml}")
    out["max_level"] = None if ml is None else int(ml)
    return out


def spann_posting_rule(ranks, replica_count: int) -> list:
    """posting_centroids_for_vector (src/index/spann.rs:130-186) over one row's centroid ranks (distance, negated for IP; f32): the
    lists the row sits in, the primary first.  The restatement the device kernels are checked against."""
    r = np.asarray(ranks, np.float32).reshape(-1)
    nc = r.size
    if nc == 0:
        return []
    keep = min(replica_count + 1, nc)
    best = [(np.float32(np.inf), None)] * keep
    for c in range(nc):
        rank = r[c]
        if rank >= best[keep - 1][0]:
            continue
        pos = keep - 1
        while pos > 0 and rank < best[pos - 1][0]:
            best[pos] = best[pos - 1]
            pos -= 1
        best[pos] = (rank, c)
    if best[0][1] is None:
        return [0]
    sel = [best[0][1]]
    if replica_count == 0:
        return sel
    p = np.float32(best[0][0])
    eps = np.float32(np.finfo(np.float32).eps)
    with np.errstate(all="ignore"):
        a = np.float32(abs(p))
        m = eps if np.isnan(a) else max(a, eps)   # f32::max ignores NaN
        slack = np.float32(m * (np.float32(1.35) - np.float32(1.0)))   # 0.35000002
        threshold = np.float32(p + slack)
    for rank, c in best[1:]:
        if c is None:
            continue
        if len(sel) <= replica_count and rank <= threshold:
            sel.append(c)
    return sel


def _f32(a, ndim: int, what: str) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.float32:
        a = a.astype(np.float32)
    if a.ndim != ndim:
        raise ValueError(f"{what} must be a {ndim}-D array")
    if not a.flags["C_CONTIGUOUS"]:
        if ndim == 2:
            raise ValueError("numpy array must be contiguous (C-order)")  # src/python/mod.rs:1393-1395
        a = np.ascontiguousarray(a)
    return a


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _sync_producer(tensor) -> None:
    """The library works on its own HIP stream: device inputs must be complete before the call.
    Synchronise the torch stream that (may have) produced `tensor`."""
    import torch

    torch.cuda.current_stream(tensor.device).synchronize()


class FlatIndex:
    """`lynse._core.FlatIndex` (src/python/mod.rs:1942-2047) on one MI355X.

    The reference opens an mmapped file at `path`; here rows live in HBM (`path` may be None).  If
    `path` names an existing raw little-endian f32 row file (the reference's segment format,
    flat_mmap.rs:89-109) it is loaded.
    """

    def __init__(self, path: Optional[str], dim: int, device: Optional[int] = None, dtype: str = "f32"):
        self._h = C.c_void_p()
        self._dim = int(dim)
        dev = default_device() if device is None else int(device)
        d = dtype.strip().lower()  # VectorDtype::parse (src/storage/dtype.rs:12-21)
        if d in ("f32", "float32", "float"):
            self.dtype = "f32"
        elif d in ("f16", "float16", "half", "fp16"):
            self.dtype = "f16"
        else:
            raise ValueError(f"unsupported vector dtype '{dtype}'; expected float32/f32 or float16/f16")
        check(lib.lynse_hip_flat_create(self._dim, dev, C.byref(self._h)))
        if self.dtype == "f16":
            check(lib.lynse_hip_flat_set_dtype(self._h, 1))
        self.path = path
        if path and os.path.exists(path) and os.path.getsize(path) > 0:
            if self.dtype == "f16":
                bits = np.fromfile(path, dtype="<u2")
                if bits.size % self._dim:
                    raise IOError("vector file size is not a multiple of the row size")
                self.write_f16_bits(bits.reshape(-1, self._dim))
            else:
                data = np.fromfile(path, dtype="<f4")
                if data.size % self._dim:
                    raise IOError("vector file size is not a multiple of the row size")
                self.write(data.reshape(-1, self._dim))

    def write_f16_bits(self, bits) -> None:
        """Append rows given as IEEE binary16 words — the bytes of an F16 segment file (flat_mmap.rs:187-221)."""
        b = np.ascontiguousarray(bits, dtype=np.uint16)
        if b.ndim != 2 or b.shape[1] != self._dim:
            raise ValueError(f"data dimension mismatch: expected {self._dim}")
        check(lib.lynse_hip_flat_append_f16_bits(self._h, _ptr(b), b.shape[0]))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.lynse_hip_flat_destroy(h)

    def __len__(self) -> int:
        return int(lib.lynse_hip_flat_len(self._h))

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def handle(self):
        return self._h

    def reserve(self, rows: int) -> None:
        check(lib.lynse_hip_flat_reserve(self._h, int(rows)))

    def write(self, data) -> None:
        """Append rows from a contiguous (n, dim) float32 array (FlatMmap::write)."""
        a = _f32(data, 2, "data")
        if a.shape[1] != self._dim:
            raise ValueError(f"data dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        check(lib.lynse_hip_flat_append_f32(self._h, _ptr(a), a.shape[0]))

    def write_device(self, tensor) -> None:
        """Append rows already resident in HBM (a contiguous float32 torch tensor on this device)."""
        if tensor.dim() != 2 or tensor.shape[1] != self._dim or not tensor.is_contiguous():
            raise ValueError("tensor must be a contiguous (n, dim) float32 device tensor")
        _sync_producer(tensor)
        check(lib.lynse_hip_flat_append_f32_device(self._h, C.c_void_p(tensor.data_ptr()), tensor.shape[0]))

    def write_packed(self, words) -> None:
        """Append pre-packed one-bit rows: (n, ceil(dim/64)) uint64, LSB-first (BinaryData layout)."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.ndim != 2 or w.shape[1] != (self._dim + 63) // 64:
            raise ValueError("packed rows must have ceil(dim/64) u64 words")
        check(lib.lynse_hip_flat_append_packed_u64(self._h, _ptr(w), w.shape[0]))

    def write_packed_device(self, tensor) -> None:
        _sync_producer(tensor)
        check(lib.lynse_hip_flat_append_packed_u64_device(self._h, C.c_void_p(tensor.data_ptr()), tensor.shape[0]))

    def finalize(self) -> None:
        check(lib.lynse_hip_flat_finalize(self._h))

    def set_row_map(self, stride: int, offset: int) -> None:
        check(lib.lynse_hip_flat_set_row_map(self._h, int(stride), int(offset)))

    def set_ip_form(self, form: int) -> None:
        check(lib.lynse_hip_flat_set_ip_form(self._h, int(form)))

    def set_fused_search(self, on: bool = True) -> None:
        """on=False forces the staged pipeline for small shards / few queries (the fused single-launch search is the default)."""
        check(lib.lynse_hip_flat_set_fused_search(self._h, 1 if on else 0))

    def set_plan(self, stage0_rows: int = 4096, growth: int = 8, cap: int = 8192) -> None:
        check(lib.lynse_hip_flat_set_plan(self._h, stage0_rows, growth, cap))

    def read_rows(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, self._dim), np.float32)
        check(lib.lynse_hip_flat_read_rows(self._h, first, n, _ptr(out)))
        return out

    def read_packed(self, first: int, n: int) -> np.ndarray:
        out = np.empty((n, (self._dim + 63) // 64), np.uint64)
        check(lib.lynse_hip_flat_read_packed(self._h, first, n, _ptr(out)))
        return out

    # -- row mutation (the ROW MUTATION block of include/lynse_hip.h) -----------------------------------------------------------
    def update_rows(self, rows, data) -> None:
        """Rewrite the listed shard rows in place (distinct, each < len); every derived copy and auxiliary index is dropped and
        built again from the final rows by the searches that need it."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint64)
        a = _f32(data, 2, "data")
        if a.shape[1] != self._dim:
            raise ValueError(f"data dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        if a.shape[0] != r.size:
            raise ValueError("rows length must match the number of vectors")
        check(lib.lynse_hip_flat_update_rows_f32(self._h, _ptr(r), _ptr(a), r.size))

    @staticmethod
    def _keep_words(keep) -> np.ndarray:
        if isinstance(keep, BitSet):
            return keep.words
        b = np.asarray(keep)
        if b.dtype != np.bool_ or b.ndim != 1:
            raise ValueError("keep must be a BitSet or a one-dimensional boolean array")
        return np.packbits(np.concatenate([b, np.zeros(-b.size % 64, np.bool_)]), bitorder="little").view(np.uint64)

    def compact(self, keep, window_rows: int = 0) -> int:
        """Drop the rows whose `keep` bit is clear, in place and in order (new row j = the j-th kept row) -> the new length.
        `keep` is a BitSet or a boolean array over the rows."""
        w = np.ascontiguousarray(self._keep_words(keep), dtype=np.uint64)
        out = C.c_uint64(0)
        check(lib.lynse_hip_flat_compact_rows(self._h, _ptr(w), w.size, int(window_rows), C.byref(out)))
        return int(out.value)

    def gather_rows(self, rows) -> np.ndarray:
        """The listed rows as f32, in the order given (repeats allowed)."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint64)
        out = np.empty((r.size, self._dim), np.float32)
        check(lib.lynse_hip_flat_gather_rows(self._h, _ptr(r), r.size, _ptr(out)))
        return out

    @staticmethod
    def compact_plan(keep, n: int, window_rows: int = 0, row_bytes: int = 0) -> dict:
        """What `compact` will do to a shard of n rows (host only): the live count, the window size, per 64-row word the destination of
        its first kept row, and per window (src, dst, live, path) with path 0 untouched / 1 direct / 2 staged."""
        w = np.ascontiguousarray(FlatIndex._keep_words(keep), dtype=np.uint64)
        live, wrows, nwin = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        args = (_ptr(w), w.size, int(n), int(window_rows), int(row_bytes), C.byref(live), C.byref(wrows), C.byref(nwin))
        check(lib.lynse_hip_compact_plan(*args, None, None))
        base = np.zeros((int(n) + 63) // 64, np.uint32)
        win = np.zeros((nwin.value, 4), np.uint64)
        check(lib.lynse_hip_compact_plan(*args, _ptr(base), _ptr(win)))
        return {"live": int(live.value), "window_rows": int(wrows.value), "word_base": base, "windows": win}

    # -- search -------------------------------------------------------------------------------
    def _search_f32(self, fn, queries, k: int, metric, *extra):
        """One `lynse_hip_flat_search_*_f32` entry over f32 queries; `extra` goes between the metric and the outputs."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(fn(self._h, _ptr(q), nq, k, m, *extra, _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_batch_arrays(self, queries, k: int, metric):
        """Batched search returning padded arrays (rows u64[nq,k], dists f32[nq,k], counts u32[nq])."""
        return self._search_f32(lib.lynse_hip_flat_search_f32, queries, k, metric)

    def search_sq8_batch_arrays(self, queries, k: int, metric):
        """`FlatMmap::search(.., use_sq8 = true, ..)` — the FLAT-*-SQ8 index modes (flat_mmap.rs:891-905, :5868-5926)."""
        return self._search_f32(lib.lynse_hip_flat_search_sq8_f32, queries, k, metric)

    def search_approx(self, query, k: int, metric, eps: Optional[float] = None):
        """The approximate flat search of one query (FlatMmap::search with an ApproxSearchConfig, flat_mmap.rs:847-889; the contract
        block of include/lynse_hip.h) -> rows u64[c], RAW distances f32[c] (round them last: round_distances_to_eps) and what ran:
        {"path": 1-4, "ip_case": 0 | "sum_desc" | "sum_asc" | "hybrid", "pool", "sample_dims", "fell_back", "eps"}."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(query, 1, "query")
        if q.shape[0] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[0]}")
        k = int(k)
        e = normalize_eps(eps)
        rows, dists = np.empty(max(k, 1), np.uint64), np.empty(max(k, 1), np.float32)
        count, info = C.c_uint32(0), _lib.ApproxInfo()
        check(lib.lynse_hip_flat_search_approx_f32(self._h, _ptr(q), k, m, e, _ptr(rows), _ptr(dists), C.byref(count), C.byref(info)))
        c = int(count.value)
        return rows[:c], dists[:c], {"path": int(info.path), "ip_case": (0, "sum_desc", "sum_asc", "hybrid")[int(info.ip_case)], "pool": int(info.pool),
                                     "sample_dims": int(info.sample_dims), "fell_back": bool(info.fell_back), "eps": e}

    def sq8_params(self):
        mins, scales = np.empty(self._dim, np.float32), np.empty(self._dim, np.float32)
        check(lib.lynse_hip_flat_sq8_params(self._h, _ptr(mins), _ptr(scales)))
        return mins, scales

    def _two_pass_stage_times(self, fn, reset: bool) -> dict:
        """The stage counters the PQ, RaBitQ and PolarVec searches share (CodedScratch::stage_times, csrc/coded_host.inc)."""
        out = np.zeros(3, np.float64)
        check(fn(self._h, _ptr(out), 1 if reset else 0))
        return {"searches": int(out[0]), "scan_us": float(out[1]), "rescore_us": float(out[2])}

    # -- FLAT-*-PQ (PQIndex, src/storage/pq_mmap.rs; include/lynse_hip.h states the contract) --------------------------------
    def build_pq(self, n_subspaces: int, n_clusters: int = 256) -> None:
        """Train the product quantiser on the rows held now and encode them (rows appended later stay outside the index)."""
        check(lib.lynse_hip_flat_build_pq(self._h, int(n_subspaces), int(n_clusters)))

    def load_pq(self, codebooks, codes) -> None:
        """Install a trained quantiser: codebooks f32 [M][K][ss], codes u8 [n][M] for the first n rows."""
        cb = np.ascontiguousarray(codebooks, dtype=np.float32)
        cd = np.ascontiguousarray(codes, dtype=np.uint8)
        if cb.ndim != 3 or cd.ndim != 2 or cd.shape[1] != cb.shape[0]:
            raise ValueError("codebooks must be [M][K][ss] and codes [n][M]")
        check(lib.lynse_hip_flat_load_pq(self._h, cb.shape[0], cb.shape[1], _ptr(cb), _ptr(cd), cd.shape[0]))

    def drop_pq(self) -> None:
        check(lib.lynse_hip_flat_drop_pq(self._h))

    def pq_params(self, arrays: bool = True) -> dict:
        """{"M", "K", "ss", "n"} and, with `arrays`, "codebooks" f32 [M][K][ss] and "codes" u8 [n][M]; M == 0 without an index."""
        mks = np.zeros(3, np.uint32)
        n = C.c_uint64(0)
        check(lib.lynse_hip_flat_pq_params(self._h, _ptr(mks), C.byref(n), None, None))
        m, k, ss = (int(x) for x in mks)
        out = {"M": m, "K": k, "ss": ss, "n": int(n.value)}
        if arrays and m:
            cb = np.empty((m, k, ss), np.float32)
            cd = np.empty((int(n.value), m), np.uint8)
            check(lib.lynse_hip_flat_pq_params(self._h, _ptr(mks), C.byref(n), _ptr(cb), _ptr(cd)))
            out["codebooks"], out["codes"] = cb, cd
        return out

    def search_pq_batch_arrays(self, queries, k: int, metric, oversample: int = PQ_OVERSAMPLE):
        """ADC scan over the codes, the N = min(k' * oversample, n_pq) best by (ADC score, row), exact rescore of those rows."""
        return self._search_f32(lib.lynse_hip_flat_search_pq_f32, queries, k, metric, int(oversample))

    def pq_stage_times(self, reset: bool = True) -> dict:
        """With profiling on: PQ searches timed and the summed microseconds of the scan stage and of the rescore."""
        return self._two_pass_stage_times(lib.lynse_hip_flat_pq_stage_times, reset)

    # -- FLAT-*-RABITQ (RaBitQIndex, src/storage/rabitq_mmap.rs; include/lynse_hip.h states the contract) ----------------------
    def build_rabitq(self) -> None:
        """Encode the rows held now into 1-bit codes and norms (no training; rows appended later stay outside the index)."""
        check(lib.lynse_hip_flat_build_rabitq(self._h))

    def load_rabitq(self, sign_words, codes, norms) -> None:
        """Install an index as rabitq_index.bin holds it: u64 sign words, codes u8 [n][code_bytes], norms f32 [n] for the first n rows."""
        sw = np.ascontiguousarray(sign_words, dtype=np.uint64).reshape(-1)
        cd = np.ascontiguousarray(codes, dtype=np.uint8)
        nm = np.ascontiguousarray(norms, dtype=np.float32).reshape(-1)
        padded = 1 << max(self._dim - 1, 0).bit_length()
        if cd.ndim != 2 or cd.shape[1] != (padded + 7) // 8 or nm.shape[0] != cd.shape[0]:
            raise ValueError("codes must be [n][ceil(next_pow2(dim) / 8)] and norms [n]")
        check(lib.lynse_hip_flat_load_rabitq(self._h, self._dim, _ptr(sw), sw.shape[0], _ptr(cd), _ptr(nm), cd.shape[0]))

    def drop_rabitq(self) -> None:
        check(lib.lynse_hip_flat_drop_rabitq(self._h))

    def rabitq_params(self, arrays: bool = True) -> dict:
        """{"dim", "padded_dim", "code_bytes", "n"} and, with `arrays`, "sign_words" u64, "codes" u8 [n][code_bytes] and "norms"
        f32 [n]; padded_dim == 0 without an index."""
        dims = np.zeros(3, np.uint32)
        n = C.c_uint64(0)
        check(lib.lynse_hip_flat_rabitq_params(self._h, _ptr(dims), C.byref(n), None, None, None))
        dim, padded, cb = (int(x) for x in dims)
        out = {"dim": dim, "padded_dim": padded, "code_bytes": cb, "n": int(n.value)}
        if arrays and padded:
            sw = np.empty((padded + 63) // 64, np.uint64)
            cd = np.empty((int(n.value), cb), np.uint8)
            nm = np.empty(int(n.value), np.float32)
            check(lib.lynse_hip_flat_rabitq_params(self._h, _ptr(dims), C.byref(n), _ptr(sw), _ptr(cd), _ptr(nm)))
            out["sign_words"], out["codes"], out["norms"] = sw, cd, nm
        return out

    def search_rabitq_batch_arrays(self, queries, k: int, metric, oversample: int = RABITQ_OVERSAMPLE):
        """Scan of the 1-bit codes, the N = min(k' * oversample, n_rbq) best by (score, row), exact rescore of those rows."""
        return self._search_f32(lib.lynse_hip_flat_search_rabitq_f32, queries, k, metric, int(oversample))

    def rabitq_stage_times(self, reset: bool = True) -> dict:
        """With profiling on: RaBitQ searches timed and the summed microseconds of the scan stage and of the rescore."""
        return self._two_pass_stage_times(lib.lynse_hip_flat_rabitq_stage_times, reset)

    # -- FLAT-*-POLARVEC<b> (PolarVecIndex, src/storage/polarvec_mmap.rs; include/lynse_hip.h states the contract) --------------
    def build_polarvec(self, bits: int, metric) -> None:
        """Fit the per-dimension grid on the rows held now and encode them into `bits`-bit codes (no training; rows appended later
        stay outside the index).  The metric decides which correction array is kept: residual_sq for l2, inv_v_hat_norms for cosine."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        bits = int(bits)
        if not 0 <= bits < 1 << 32:
            raise ValueError("bits must be in [1, 8]")
        check(lib.lynse_hip_flat_build_polarvec(self._h, bits, m))

    def load_polarvec(self, bits: int, sign_words, dim_mins, dim_scales, codes, residual_sq=None, inv_v_hat_norms=None) -> None:
        """Install an index as polarvec_index.bin holds it: u64 sign words, f32 dim_mins / dim_scales [padded_dim], codes u8
        [n][bytes_per_vec] for the first n rows and the optional f32 [n] correction arrays."""
        bits = int(bits)
        if not 1 <= bits <= 8:
            raise ValueError("bits must be in [1, 8]")
        sw = np.ascontiguousarray(sign_words, dtype=np.uint64).reshape(-1)
        mn = np.ascontiguousarray(dim_mins, dtype=np.float32).reshape(-1)
        sc = np.ascontiguousarray(dim_scales, dtype=np.float32).reshape(-1)
        cd = np.ascontiguousarray(codes, dtype=np.uint8)
        padded = 1 << max(self._dim - 1, 0).bit_length()
        if cd.ndim != 2 or cd.shape[1] != (padded * bits + 7) // 8 or mn.shape[0] != padded or sc.shape[0] != padded:
            raise ValueError("codes must be [n][ceil(next_pow2(dim) * bits / 8)], dim_mins and dim_scales [next_pow2(dim)]")
        opt = []
        for a in (residual_sq, inv_v_hat_norms):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
            if a is not None and a.shape[0] != cd.shape[0]:
                raise ValueError("a correction array holds one value per code row")
            opt.append(a)
        check(lib.lynse_hip_flat_load_polarvec(self._h, self._dim, bits, _ptr(sw), sw.shape[0], _ptr(mn), _ptr(sc), _ptr(cd),
                                               None if opt[0] is None else _ptr(opt[0]), None if opt[1] is None else _ptr(opt[1]),
                                               cd.shape[0]))

    def drop_polarvec(self) -> None:
        check(lib.lynse_hip_flat_drop_polarvec(self._h))

    def polarvec_params(self, arrays: bool = True) -> dict:
        """{"dim", "padded_dim", "bits", "bytes_per_vec", "flags", "n"} and, with `arrays`, "sign_words" u64, "dim_mins" / "dim_scales"
        f32 [padded_dim], "codes" u8 [n][bytes_per_vec], "residual_sq" and "inv_v_hat_norms" f32 [n] or None (flags 1 and 2);
        padded_dim == 0 without an index."""
        dims = np.zeros(5, np.uint32)
        n = C.c_uint64(0)
        check(lib.lynse_hip_flat_polarvec_params(self._h, _ptr(dims), C.byref(n), None, None, None, None, None, None))
        dim, padded, bits, bpv, flags = (int(x) for x in dims)
        out = {"dim": dim, "padded_dim": padded, "bits": bits, "bytes_per_vec": bpv, "flags": flags, "n": int(n.value)}
        if arrays and padded:
            nv = int(n.value)
            sw = np.empty((padded + 63) // 64, np.uint64)
            mn, sc = np.empty(padded, np.float32), np.empty(padded, np.float32)
            cd = np.empty((nv, bpv), np.uint8)
            rs = np.empty(nv, np.float32) if flags & 1 else None
            iv = np.empty(nv, np.float32) if flags & 2 else None
            check(lib.lynse_hip_flat_polarvec_params(self._h, _ptr(dims), C.byref(n), _ptr(sw), _ptr(mn), _ptr(sc), _ptr(cd),
                                                     None if rs is None else _ptr(rs), None if iv is None else _ptr(iv)))
            out.update(sign_words=sw, dim_mins=mn, dim_scales=sc, codes=cd, residual_sq=rs, inv_v_hat_norms=iv)
        return out

    def search_polarvec_batch_arrays(self, queries, k: int, metric, oversample: int = POLARVEC_OVERSAMPLE):
        """Table scan of the b-bit codes, the N = min(k' * oversample, n_plv) best by (score, row), exact rescore of those rows."""
        return self._search_f32(lib.lynse_hip_flat_search_polarvec_f32, queries, k, metric, int(oversample))

    def polarvec_stage_times(self, reset: bool = False) -> dict:
        """With profiling on: PolarVec searches timed and the summed microseconds of the scan stage and of the rescore."""
        return self._two_pass_stage_times(lib.lynse_hip_flat_polarvec_stage_times, reset)

    # -- HNSW-* (HNSWIndex, src/index/hnsw.rs; include/lynse_hip.h states the contract) ---------------------------------------
    def build_hnsw(self, metric, m: int = HNSW_DEFAULTS["m"], ef_construction: int = HNSW_DEFAULTS["ef_construction"],
                   ef_search: int = HNSW_DEFAULTS["ef_search"], max_level: Optional[int] = None, seed: int = HNSW_SEED) -> None:
        """Build the graph over the rows held now from their exact neighbour lists (rows appended later stay outside it until
        extend_hnsw takes them in)."""
        mt = metric if isinstance(metric, int) else metric_from_str(metric)
        check(lib.lynse_hip_flat_build_hnsw(self._h, mt, int(m), int(ef_construction), int(ef_search),
                                            -1 if max_level is None else int(max_level), int(seed)))

    def extend_hnsw(self, mode: int = 0) -> None:
        """Take the rows appended since the build into its graph: afterwards the graph equals a build over every row held now (rule 7).
        mode 0 picks between the incremental path and the plain build, mode 1 always takes the incremental path.  A loaded graph
        answers NotImplementedError."""
        check(lib.lynse_hip_flat_hnsw_extend(self._h, int(mode)))

    def hnsw_extend_stats(self) -> dict:
        """The last extend_hnsw: rows before and after, path (0 incremental, 1 plain build, 2 nothing to do), the new (node, level)
        items, the old ones searched again, the adjacency lists recomputed and those that went through the heuristic again, and the
        microseconds of the reverse scan, the candidate searches, the selection, the reverse edges and the whole call."""
        out = np.zeros(12, np.float64)
        check(lib.lynse_hip_flat_hnsw_extend_stats(self._h, _ptr(out)))
        names = ("rows_before", "rows_after", "path", "new_items", "researched", "dirty_lists", "reselected")
        d = {k: int(out[i]) for i, k in enumerate(names)}
        d.update({k: float(out[7 + i]) for i, k in enumerate(("scan_us", "cand_us", "select_us", "reverse_us", "total_us"))})
        return d

    def load_hnsw(self, metric, m: int, ef_search: int, levels, adj0, upper_node, upper_level, upper_adj, entry: int) -> None:
        """Install a graph as hnsw_params exports it: levels u32 [n], adj0 u32 [n][2 m], the upper lists u32 [n_upper][m] with their
        (node, level) in ascending order, lists padded with 0xFFFFFFFF."""
        mt = metric if isinstance(metric, int) else metric_from_str(metric)
        lv = np.ascontiguousarray(levels, dtype=np.uint32).reshape(-1)
        a0 = np.ascontiguousarray(adj0, dtype=np.uint32)
        un = np.ascontiguousarray(upper_node, dtype=np.uint32).reshape(-1)
        ul = np.ascontiguousarray(upper_level, dtype=np.uint32).reshape(-1)
        ua = np.ascontiguousarray(upper_adj, dtype=np.uint32).reshape(-1, int(m))
        if a0.ndim != 2 or a0.shape != (lv.shape[0], 2 * int(m)) or ul.shape != un.shape or ua.shape[0] != un.shape[0]:
            raise ValueError("adj0 must be [n][2 m], upper_adj [n_upper][m] with upper_node / upper_level [n_upper]")
        check(lib.lynse_hip_flat_load_hnsw(self._h, mt, int(m), int(ef_search), _ptr(lv), lv.shape[0], _ptr(a0), un.shape[0], _ptr(un), _ptr(ul),
                                           _ptr(ua), int(entry)))

    def drop_hnsw(self) -> None:
        check(lib.lynse_hip_flat_drop_hnsw(self._h))

    def hnsw_params(self, arrays: bool = True) -> dict:
        """{"metric", "m", "ef_search", "entry", "top_level", "n_upper", "n"} and, with `arrays`, "levels", "adj0", "upper_node",
        "upper_level", "upper_adj"; m == 0 without an index."""
        info = np.zeros(6, np.uint32)
        n = C.c_uint64(0)
        check(lib.lynse_hip_flat_hnsw_params(self._h, _ptr(info), C.byref(n), None, None, None, None, None))
        metric, m, efs, entry, top, nu = (int(x) for x in info)
        out = {"metric": metric, "m": m, "ef_search": efs, "entry": entry, "top_level": top, "n_upper": nu, "n": int(n.value)}
        if arrays and m:
            lv, a0 = np.empty(out["n"], np.uint32), np.empty((out["n"], 2 * m), np.uint32)
            un, ul, ua = np.empty(nu, np.uint32), np.empty(nu, np.uint32), np.empty((nu, m), np.uint32)
            check(lib.lynse_hip_flat_hnsw_params(self._h, _ptr(info), C.byref(n), _ptr(lv), _ptr(a0), _ptr(un), _ptr(ul), _ptr(ua)))
            out.update(levels=lv, adj0=a0, upper_node=un, upper_level=ul, upper_adj=ua)
        return out

    def search_hnsw_batch_arrays(self, queries, k: int, metric, ef: int = 0):
        """Greedy descent and the beam search at level 0 with ef = max(ef or the index's ef_search, k)."""
        return self._search_f32(lib.lynse_hip_flat_search_hnsw_f32, queries, k, metric, int(ef))

    def hnsw_stage_times(self, reset: bool = True) -> dict:
        """The stages of the last build (microseconds) and, with profiling on, the searches timed, their kernel microseconds and the
        distances they scored."""
        out = np.zeros(6, np.float64)
        check(lib.lynse_hip_flat_hnsw_stage_times(self._h, _ptr(out), 1 if reset else 0))
        return {"candidates_us": float(out[0]), "select_us": float(out[1]), "reverse_us": float(out[2]), "searches": int(out[3]),
                "search_us": float(out[4]), "scored": int(out[5])}

    # -- DISKANN-* (DiskANNIndex, src/index/diskann.rs; include/lynse_hip.h states the contract) --------------------------------
    def build_diskann(self, metric, r: int = DISKANN_DEFAULTS["r"], l: int = DISKANN_DEFAULTS["l"], alpha: float = DISKANN_DEFAULTS["alpha"],
                      max_degree: Optional[int] = None, seed: int = DISKANN_SEED, max_batches: int = 0) -> None:
        """The batched Vamana build over the rows held now (rows appended later stay outside the graph).  max_batches > 0 stops after
        that many batches, counted across both passes, and installs the graph as it stands: a test instrument."""
        mt = metric if isinstance(metric, int) else metric_from_str(metric)
        check(lib.lynse_hip_flat_build_diskann(self._h, mt, int(r), int(l), float(alpha), int(r if max_degree is None else max_degree), int(seed),
                                               int(max_batches)))

    def load_diskann(self, metric, r: int, l: int, adj, entry: int) -> None:
        """Install a graph as diskann_params exports it: adj u32 [n][r], lists padded with 0xFFFFFFFF."""
        mt = metric if isinstance(metric, int) else metric_from_str(metric)
        a = np.ascontiguousarray(adj, dtype=np.uint32)
        if a.ndim != 2 or a.shape[1] != int(r):
            raise ValueError("adj must be [n][r]")
        check(lib.lynse_hip_flat_load_diskann(self._h, mt, int(r), int(l), _ptr(a), a.shape[0], int(entry)))

    def drop_diskann(self) -> None:
        check(lib.lynse_hip_flat_drop_diskann(self._h))

    def diskann_params(self, arrays: bool = True) -> dict:
        """{"metric", "r", "l", "entry", "alpha", "n"} and, with `arrays`, "adj"; r == 0 without an index."""
        info = np.zeros(4, np.uint32)
        alpha, n = C.c_float(0.0), C.c_uint64(0)
        check(lib.lynse_hip_flat_diskann_params(self._h, _ptr(info), C.byref(alpha), C.byref(n), None))
        metric, r, l, entry = (int(x) for x in info)
        out = {"metric": metric, "r": r, "l": l, "entry": entry, "alpha": float(alpha.value), "n": int(n.value)}
        if arrays and r:
            adj = np.empty((out["n"], r), np.uint32)
            check(lib.lynse_hip_flat_diskann_params(self._h, _ptr(info), C.byref(alpha), C.byref(n), _ptr(adj)))
            out["adj"] = adj
        return out

    def search_diskann_batch_arrays(self, queries, k: int, metric, ef: int = 0):
        """The beam search from the entry and 8 anchors with ef = min(max(ef, the index's l, 10 k), n)."""
        return self._search_f32(lib.lynse_hip_flat_search_diskann_f32, queries, k, metric, int(ef))

    def diskann_stage_times(self, reset: bool = True) -> dict:
        """The last build (microseconds: the three stages only from a build that ran with profiling on, the host draws, the whole) and,
        with profiling on, the searches timed, their kernel microseconds and the distances they scored."""
        out = np.zeros(8, np.float64)
        check(lib.lynse_hip_flat_diskann_stage_times(self._h, _ptr(out), 1 if reset else 0))
        return {"build_search_us": float(out[0]), "build_prune_us": float(out[1]), "build_commit_us": float(out[2]), "build_draws_us": float(out[3]),
                "build_us": float(out[4]), "searches": int(out[5]), "search_us": float(out[6]), "scored": int(out[7])}

    def search_range_batch_arrays(self, queries, thresholds, max_results: int, metric, bitset_words=None):
        """Range search (Collection::search_range, engine.rs:6410-6483) for a batch, one threshold per query: the exact scan of every
        row (of the rows of `bitset_words`, the reference's BitSet words, when given), the rows with d <= threshold (ip: d >= threshold)
        -> (rows u64[nq, max_results], distances f32[nq, max_results], counts u32[nq], passed u64[nq]): the best
        counts[q] = min(passed[q], max_results) passers by (distance, row), best first, padded with row ~0 and the worst distance."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        nq, cap = q.shape[0], int(max_results)
        if cap < 0:
            raise ValueError("max_results must not be negative")
        thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
        if thr.size != nq:
            raise ValueError(f"one threshold per query: expected {nq}, got {thr.size}")
        rows = np.empty((nq, cap), np.uint64)
        dists = np.empty((nq, cap), np.float32)
        counts = np.zeros(nq, np.uint32)
        passed = np.zeros(nq, np.uint64)
        if cap == 0 or nq == 0:   # search_range's first early return: nothing is scanned
            return rows, dists, counts, passed
        words, n_words = None, 0
        if bitset_words is not None:
            words = np.ascontiguousarray(np.asarray(bitset_words).reshape(-1), dtype=np.uint64)
            n_words = int(words.size)
            if n_words == 0:   # an empty mask is still a mask (NULL would mean every row)
                words = np.zeros(1, np.uint64)
        check(lib.lynse_hip_flat_search_range_f32(self._h, _ptr(q), nq, _ptr(thr), cap, m, None if words is None else _ptr(words), n_words,
                                                  _ptr(rows), _ptr(dists), _ptr(counts), _ptr(passed)))
        return rows, dists, counts, passed

    def search_filtered_batch_arrays(self, queries, k: int, metric, subset_rows):
        """`FlatMmap::search_filtered` (flat_mmap.rs:491-815) for a batch sharing one subset of row indices."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        sub = np.ascontiguousarray(np.asarray(subset_rows).reshape(-1), dtype=np.uint64)
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_flat_search_filtered_f32(self._h, _ptr(q), nq, k, m, _ptr(sub) if sub.size else None, sub.size,
                                                     _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_filtered_bitset_batch_arrays(self, queries, k: int, metric, bitset_words):
        """Same with the subset given as the reference's BitSet words (u64, bit r of word r // 64)."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        words = np.ascontiguousarray(np.asarray(bitset_words).reshape(-1), dtype=np.uint64)
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_flat_search_filtered_bitset_f32(self._h, _ptr(q), nq, k, m, _ptr(words) if words.size else None,
                                                            words.size, _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_filtered_bitset_device_batch_arrays(self, queries, k: int, metric, d_words, n_words: int, count: int):
        """Same with the BitSet words already in this device's memory (`d_words`: a device pointer, FieldFilter.words_device) and
        their match count supplied by the caller (lynse_hip_flat_search_filtered_bitset_device_f32): a device copy, no upload."""
        return self._search_f32(lib.lynse_hip_flat_search_filtered_bitset_device_f32, queries, k, metric, d_words, int(n_words), int(count))

    def search_filtered(self, query, k: int, metric, subset_rows):
        """-> (rows u32[], distances f32[]) among `subset_rows` only."""
        q = _f32(query, 1, "query")
        rows, dists, counts = self.search_filtered_batch_arrays(q.reshape(1, -1), k, metric, subset_rows)
        c = int(counts[0])
        return rows[0, :c].astype(np.uint32), dists[0, :c].copy()

    def search_packed_arrays(self, query_words, k: int, metric):
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        qw = np.ascontiguousarray(query_words, dtype=np.uint64)
        if qw.ndim == 1:
            qw = qw.reshape(1, -1)
        nq, k = qw.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_flat_search_packed_u64(self._h, _ptr(qw), nq, k, m, _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search(self, query, k: int = 10, metric: str = "ip"):
        """Brute-force top-k -> (indices u32[k'], distances f32[k']) (src/python/mod.rs:1990-2006)."""
        m = metric_from_str(metric)
        q = _f32(query, 1, "query")
        rows, dists, counts = self.search_batch_arrays(q.reshape(1, -1), k, m)
        c = int(counts[0])
        return rows[0, :c].astype(np.uint32), dists[0, :c].copy()

    def batch_search(self, queries, k: int = 10, metric: str = "ip"):
        """list of (indices, distances) per query (src/python/mod.rs:2018-2046).  The reference loops
        queries sequentially, re-reading the collection each time; here the batch shares one pass."""
        m = metric_from_str(metric)
        rows, dists, counts = self.search_batch_arrays(queries, k, m)
        return [(rows[i, :int(c)].astype(np.uint32), dists[i, :int(c)].copy()) for i, c in enumerate(counts)]

    def search_device(self, d_queries, k: int, metric, d_rows, d_dists, d_counts, stream=None):
        """All buffers are torch tensors resident on this device (bench path: no PCIe in the timed region)."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        nq = d_queries.shape[0]
        _sync_producer(d_queries)
        check(lib.lynse_hip_flat_search_f32_device(
            self._h, C.c_void_p(d_queries.data_ptr()), nq, int(k), m, C.c_void_p(d_rows.data_ptr()),
            C.c_void_p(d_dists.data_ptr()), C.c_void_p(d_counts.data_ptr()),
            C.c_void_p(stream) if stream else None))

    def search_packed_device(self, d_qwords, k: int, metric, d_rows, d_dists, d_counts, stream=None):
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        nq = d_qwords.shape[0]
        _sync_producer(d_qwords)
        check(lib.lynse_hip_flat_search_packed_u64_device(
            self._h, C.c_void_p(d_qwords.data_ptr()), nq, int(k), m, C.c_void_p(d_rows.data_ptr()),
            C.c_void_p(d_dists.data_ptr()), C.c_void_p(d_counts.data_ptr()),
            C.c_void_p(stream) if stream else None))

    # -- searches in flight (lynse_hip_flat_search_submit_* / _wait) --------------------------------
    def search_submit(self, d_queries, k: int, metric, d_rows, d_dists, d_counts, comm=None) -> "SearchTicket":
        """Enqueue one batch (<= 256 queries, torch tensors on this device) on a search context of the index and return a
        ticket; `wait()` makes the results final in d_rows / d_dists / d_counts.  Up to LYNSE_HIP_CONTEXTS batches overlap on
        the device.  `comm`: the communicator handle of a row-sharded collection (a collective then)."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        if _lib.METRIC_HAMMING <= m <= _lib.METRIC_TANIMOTO and d_queries.is_floating_point():
            # float queries of a binary metric are packed by the blocking entry point (pack_binary_query); batches in flight
            # take packed words: answer this one now (only without a communicator: the sharded entry points are packed-only too)
            if comm is not None:
                raise ValueError("sharded searches of a binary metric take packed u64 query words")
            self.search_device(d_queries, k, m, d_rows, d_dists, d_counts)
            return SearchTicket(None, None)
        _sync_producer(d_queries)
        t = C.c_void_p()
        fn = lib.lynse_hip_flat_search_submit_packed_u64_device if _lib.METRIC_HAMMING <= m <= _lib.METRIC_TANIMOTO else lib.lynse_hip_flat_search_submit_f32_device
        check(fn(self._h, comm, C.c_void_p(d_queries.data_ptr()), d_queries.shape[0], int(k), m, C.c_void_p(d_rows.data_ptr()),
                 C.c_void_p(d_dists.data_ptr()), C.c_void_p(d_counts.data_ptr()), C.byref(t)))
        return SearchTicket(t, (d_queries, d_rows, d_dists, d_counts))

    # -- profiling ----------------------------------------------------------------------------
    def profile_enable(self, on=True) -> None:
        """True / 1: time every search; n > 1: every n-th search (HIP events between the kernels cost microseconds); False: off."""
        check(lib.lynse_hip_flat_profile_enable(self._h, int(on)))

    def profile_get(self, reset: bool = True) -> dict:
        p = _lib.Profile()
        check(lib.lynse_hip_flat_profile_get(self._h, C.byref(p), 1 if reset else 0))
        return {f: getattr(p, f) for f, _ in _lib.Profile._fields_}

    def prepare(self, metric, nq: int = 256) -> None:
        """Build the derived copies a batch of `nq` queries of `metric` reads now (SQ8 codes, +-1 bytes, packed words, shadow)."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        check(lib.lynse_hip_flat_prepare(self._h, m, int(nq)))

    def hbm_bytes(self) -> int:
        return int(lib.lynse_hip_flat_hbm_bytes(self._h))

    def coarse_scores(self, queries, metric, coarse: str = "i8"):
        """Diagnostics of the certified coarse pass (`lynse_hip_flat_coarse_scores`): for a shard of <= 16,384 rows and <= 256 queries the
        coarse score / distance of every (query, row) as the scan kernels compute it, the certified bound E per query, and the form bits."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        scores = np.empty((q.shape[0], len(self)), np.float32)
        bound = np.empty(q.shape[0], np.float32)
        form = C.c_int(0)
        check(lib.lynse_hip_flat_coarse_scores(self._h, _ptr(q), q.shape[0], m, 1 if coarse in ("i8", "int8", 1, True) else 0, _ptr(scores), _ptr(bound), C.byref(form)))
        return scores, bound, form.value

    def coarse_scores_sq7(self, queries):
        """`coarse_scores` for the SQ7 form of the FLAT-IP int8 pass (`lynse_hip_flat_coarse_scores_sq7`): 129..256 queries, LYNSE_HIP_SQ7 not 0."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        scores = np.empty((q.shape[0], len(self)), np.float32)
        bound = np.empty(q.shape[0], np.float32)
        form = C.c_int(0)
        check(lib.lynse_hip_flat_coarse_scores_sq7(self._h, _ptr(q), q.shape[0], _ptr(scores), _ptr(bound), C.byref(form)))
        return scores, bound, form.value

    def sq7_state(self) -> dict:
        """Rows covered by the non-negative 7-bit copy of the codes (0: not built) and the overflow strikes of its scan (3 = switched off)."""
        rows, strikes = C.c_uint64(0), C.c_int(0)
        check(lib.lynse_hip_flat_sq7_state(self._h, C.byref(rows), C.byref(strikes)))
        return {"sq7_rows": rows.value, "sq7_strikes": strikes.value}

    def predict_debug(self, queries, k: int, metric) -> dict:
        """Diagnostics of the predicted plan (`lynse_hip_flat_predict_debug`): the int8 image, B_q, s_q, m_q, v_q and the threshold the prep
        kernel computes for 129..256 queries at this k, z, and the column statistics (mu, var) of the code set it read."""
        q = np.ascontiguousarray(np.atleast_2d(queries), dtype=np.float32)
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        nq, cap = q.shape[0], (self.dim + 127) // 128 * 128
        u = np.zeros((nq, cap), np.int8)
        mu, var = np.zeros(cap, np.float64), np.zeros(cap, np.float64)
        bq, sq, thr = (np.zeros(nq, np.float32) for _ in range(3))
        mq, vq = np.zeros(nq, np.float64), np.zeros(nq, np.float64)
        z, cols = C.c_double(0.0), C.c_uint32(0)
        flat = np.zeros(nq * cap, np.int8)
        check(lib.lynse_hip_flat_predict_debug(self._h, _ptr(q), nq, int(k), m, _ptr(flat), _ptr(mu), _ptr(var), _ptr(bq), _ptr(sq), _ptr(mq), _ptr(vq),
                                               _ptr(thr), C.byref(z), C.byref(cols)))
        c = cols.value
        u = flat[:nq * c].reshape(nq, c).copy()
        return {"u": u, "mu": mu[:c].copy(), "var": var[:c].copy(), "bq": bq, "sq": sq, "m": mq, "v": vq, "thr": thr, "z": z.value, "cols": c}

    def predict_state(self) -> dict:
        """Strikes of the predicted plan (3 = switched off until the codes are fitted again) and the rows its column statistics cover."""
        strikes, r8, rc, r7 = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib.lynse_hip_flat_predict_state(self._h, C.byref(strikes), C.byref(r8), C.byref(rc), C.byref(r7)))
        return {"predict_strikes": strikes.value, "stats_rows_sq8": r8.value, "stats_rows_cos": rc.value, "stats_rows_sq7": r7.value}

    def coarse_state(self) -> dict:
        """State of the coarse-pass selection: overflow strikes of the certified int8 pass (3 = switched off, -1 = off because the
        rows are not finite) and the rows covered by the SQ8 codes built so far."""
        strikes, rows = C.c_int(0), C.c_uint64(0)
        check(lib.lynse_hip_flat_coarse_state(self._h, C.byref(strikes), C.byref(rows)))
        return {"i8c_strikes": strikes.value, "sq8_rows": rows.value, "bpm_rows": int(lib.lynse_hip_flat_bpm_rows(self._h))}


class SearchTicket:
    """A batch in flight (FlatIndex.search_submit).  Keeps the tensors of the batch alive until it is waited for."""

    def __init__(self, handle, keep, ivf: bool = False):
        self._t, self._keep, self._ivf = handle, keep, ivf

    def wait(self) -> None:
        t, self._t = self._t, None
        if t is not None:
            try:
                check((lib.lynse_hip_ivf_search_wait if self._ivf else lib.lynse_hip_flat_search_wait)(t))
            finally:
                self._keep = None

    def __del__(self):  # a ticket must not die with its batch in flight: it holds a search context and the reader lock
        try:
            self.wait()
        except Exception:  # noqa: BLE001
            pass


class IvfFlatIndex:
    """`lynse._core.IvfFlatIndex` (src/python/mod.rs:2056-2156): k-means partitions, rows stored as
    contiguous per-partition slabs in HBM, search scans the nprobe nearest slabs."""

    def __init__(self, handle, dim: int, sq8: bool = False):
        self._h = handle
        self._dim = dim
        self._sq8 = sq8

    def profile_enable(self, on=True) -> None:
        check(lib.lynse_hip_ivf_profile_enable(self._h, int(on)))

    def profile_get(self, reset: bool = True) -> dict:
        """The slab store's profile; `last_plan` bit 2 / bit 6: the last staged chunk ran / started on the certified int8 pass."""
        p = _lib.Profile()
        check(lib.lynse_hip_ivf_profile_get(self._h, C.byref(p), 1 if reset else 0))
        return {f: getattr(p, f) for f, _ in _lib.Profile._fields_}

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.lynse_hip_ivf_destroy(h)

    @staticmethod
    def build(path, data, dim: int, n_partitions: int = 256, n_iters: int = 20, metric: str = "ip",
              device: Optional[int] = None, l2_partitions: bool = True, quantizer: Optional[str] = None) -> "IvfFlatIndex":
        """`quantizer="sq8"`: the IVF-{IP,L2,COS}-SQ8 IVFIndex (ivf.rs:132-337 with QuantizerType::Scalar) — k-means and the list scans
        on the decoded rows, an exact rerank of a 10 k pool against the original rows (ip / l2 / cosine)."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        a = _f32(data, 2, "data")
        if a.shape[1] != dim:
            raise ValueError(f"data dimension mismatch: expected {dim}, got {a.shape[1]}")
        if n_partitions <= 0:
            raise IOError("IVF partition count must be greater than zero")
        if quantizer is not None and str(quantizer).lower() != "sq8":
            raise NotImplementedError(f"IVF quantizer {quantizer!r} is outside this path (sq8 and the binary metrics are built)")
        if a.shape[0] < n_partitions and quantizer is None:
            raise IOError("IVF requires at least as many vectors as partitions")
        h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        if quantizer is not None:   # an IVFIndex mode: k-means clamps the list count to the rows (kmeans.rs:74-139)
            check(lib.lynse_hip_ivf_build_sq8(_ptr(a), a.shape[0], dim, n_partitions, n_iters, m, dev, C.byref(h)))
            return IvfFlatIndex(h, dim, sq8=True)
        if m >= 3:  # IVF-HAMMING/JACCARD-BINARY (src/index/mod.rs:376-385) is an IVFIndex mode: no IvfFlat L2 cells
            l2_partitions = False
        check(lib.lynse_hip_ivf_build(_ptr(a), a.shape[0], dim, n_partitions, n_iters, m,
                                      1 if l2_partitions else 0, dev, C.byref(h)))
        return IvfFlatIndex(h, dim)

    @staticmethod
    def build_device(d_rows, dim: int, n_partitions: int = 256, n_iters: int = 20, metric: str = "ip",
                     l2_partitions: bool = True) -> "IvfFlatIndex":
        """`build` over rows already resident in HBM (a contiguous float32 torch tensor on the target device): k-means, slab
        reordering and the store never stage row data through host memory.  Float metrics."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        if d_rows.dim() != 2 or d_rows.shape[1] != dim or not d_rows.is_contiguous():
            raise ValueError("rows must be a contiguous (n, dim) float32 device tensor")
        _sync_producer(d_rows)
        h = C.c_void_p()
        check(lib.lynse_hip_ivf_build_device(C.c_void_p(d_rows.data_ptr()), d_rows.shape[0], dim, n_partitions, n_iters, m,
                                             1 if l2_partitions else 0, d_rows.device.index or 0, C.byref(h)))
        return IvfFlatIndex(h, dim)

    @staticmethod
    def load_device(d_rows, centroids, assignments, metric: str = "ip", ivfflat_routing: bool = False) -> "IvfFlatIndex":
        """`load` with the rows in HBM; centroids / assignments are host arrays."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        c = _f32(centroids, 2, "centroids")
        asg = np.ascontiguousarray(assignments, dtype=np.uint32)
        _sync_producer(d_rows)
        h = C.c_void_p()
        check(lib.lynse_hip_ivf_load_device(C.c_void_p(d_rows.data_ptr()), d_rows.shape[0], d_rows.shape[1], _ptr(c), c.shape[0], _ptr(asg), m,
                                            d_rows.device.index or 0, C.byref(h)))
        idx = IvfFlatIndex(h, d_rows.shape[1])
        if ivfflat_routing:
            check(lib.lynse_hip_ivf_set_routing(h, 1))
        return idx

    def search_submit(self, d_queries, k: int, nprobe: int, d_rows, d_dists, d_counts, comm=None) -> "SearchTicket":
        """One batch IN FLIGHT (lynse_hip_ivf_search_submit_f32_device): <= 256 queries, torch tensors on the index's device; `wait()`
        of the ticket makes d_rows / d_dists / d_counts final — the results of `search_device`.  Up to LYNSE_HIP_CONTEXTS - 1 batches
        overlap on the device.  `comm`: the communicator handle of a row-sharded index (a collective then)."""
        _sync_producer(d_queries)
        t = C.c_void_p()
        check(lib.lynse_hip_ivf_search_submit_f32_device(self._h, comm, C.c_void_p(d_queries.data_ptr()), d_queries.shape[0], int(k), int(nprobe),
                                                         C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_dists.data_ptr()),
                                                         C.c_void_p(d_counts.data_ptr()), C.byref(t)))
        return SearchTicket(t, (d_queries, d_rows, d_dists, d_counts), ivf=True)

    def ticket_stats(self) -> dict:
        """Tickets of this index so far: enqueued without a host synchronisation / answered inside submit / re-answered inside wait."""
        out = np.zeros(3, np.uint64)
        check(lib.lynse_hip_ivf_ticket_stats(self._h, _ptr(out)))
        return {"in_flight": int(out[0]), "inside_submit": int(out[1]), "redone_in_wait": int(out[2])}

    def set_fused_search(self, on: bool = True) -> None:
        """on=False forces the staged pipeline for few-query searches too (tests, A/B); results are identical."""
        check(lib.lynse_hip_ivf_set_fused_search(self._h, 1 if on else 0))

    def search_device(self, d_queries, k: int, nprobe: int, d_rows, d_dists, d_counts) -> None:
        """Queries and outputs are torch tensors on the index's device (rows i64[nq,k] holding u64 bits, dists f32[nq,k],
        counts i32[nq])."""
        _sync_producer(d_queries)
        check(lib.lynse_hip_ivf_search_f32_device(self._h, C.c_void_p(d_queries.data_ptr()), d_queries.shape[0], int(k), int(nprobe),
                                                  C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_dists.data_ptr()),
                                                  C.c_void_p(d_counts.data_ptr())))

    @staticmethod
    def load(data, centroids, assignments, metric: str = "ip", device: Optional[int] = None,
             ivfflat_routing: bool = False, thresholds=None) -> "IvfFlatIndex":
        """Assemble from given centroids + assignments (parity tests feed the oracle's k-means output).
        Binary metrics also take the BinaryQuantizer thresholds (`data` = the raw rows)."""
        m = metric_from_str(metric)
        a = _f32(data, 2, "data")
        c = _f32(centroids, 2, "centroids")
        asg = np.ascontiguousarray(assignments, dtype=np.uint32)
        h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        if m >= 3:
            if thresholds is None:
                raise ValueError("binary metrics need the BinaryQuantizer thresholds")
            t = _f32(thresholds, 1, "thresholds")
            if t.size != a.shape[1]:
                raise ValueError("thresholds dimension mismatch")
            check(lib.lynse_hip_ivf_load_binary(_ptr(a), a.shape[0], a.shape[1], _ptr(c), c.shape[0], _ptr(asg), m, _ptr(t),
                                                dev, C.byref(h)))
            return IvfFlatIndex(h, a.shape[1])
        check(lib.lynse_hip_ivf_load(_ptr(a), a.shape[0], a.shape[1], _ptr(c), c.shape[0], _ptr(asg), m, dev, C.byref(h)))
        idx = IvfFlatIndex(h, a.shape[1])
        if ivfflat_routing:
            check(lib.lynse_hip_ivf_set_routing(h, 1))
        return idx

    @staticmethod
    def load_sq8(data, centroids, assignments, mins, scales, metric: str = "ip", device: Optional[int] = None) -> "IvfFlatIndex":
        """The twin of `load` for IVF-*-SQ8: `data` are the ORIGINAL rows, (`mins`, `scales`) the ScalarQuantizer state
        (`sq8_params()` of a built index); the index stores decode(encode(data)) in the lists given by `assignments`."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        a = _f32(data, 2, "data")
        c = _f32(centroids, 2, "centroids")
        asg = np.ascontiguousarray(assignments, dtype=np.uint32)
        mn, sc = _f32(mins, 1, "mins"), _f32(scales, 1, "scales")
        if mn.size != a.shape[1] or sc.size != a.shape[1]:
            raise ValueError("quantizer dimension mismatch")
        h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        check(lib.lynse_hip_ivf_load_sq8(_ptr(a), a.shape[0], a.shape[1], _ptr(c), c.shape[0], _ptr(asg), _ptr(mn), _ptr(sc), m, dev,
                                         C.byref(h)))
        return IvfFlatIndex(h, a.shape[1], sq8=True)

    def sq8_params(self):
        """SQ8 index: the fitted ScalarQuantizer (min_val f32[dim], scale f32[dim]; scale = range / 255, 1.0 for a constant dimension)."""
        mn = np.empty(self._dim, np.float32)
        sc = np.empty(self._dim, np.float32)
        check(lib.lynse_hip_ivf_sq8_params(self._h, _ptr(mn), _ptr(sc)))
        return mn, sc

    def sq8_stage_times(self, reset: bool = True) -> dict:
        """SQ8 index with profiling on (`profile_enable`): searches timed and the summed microseconds of the pool stage and of the
        rerank, from HIP events on the search stream (`lynse_hip_ivf_sq8_stage_times`)."""
        out = np.zeros(3, np.float64)
        check(lib.lynse_hip_ivf_sq8_stage_times(self._h, _ptr(out), 1 if reset else 0))
        return {"searches": int(out[0]), "pool_us": float(out[1]), "rerank_us": float(out[2])}

    @property
    def is_sq8(self) -> bool:
        return self._sq8

    def __len__(self) -> int:
        return int(lib.lynse_hip_ivf_len(self._h))

    @property
    def dim(self) -> int:
        return self._dim

    @property
    def n_partitions(self) -> int:
        return int(lib.lynse_hip_ivf_nlist(self._h))

    def insert(self, data) -> None:
        """`IVFIndex::insert` (ivf.rs:392-441): assign the new rows to the existing centroids, append them (no retraining)."""
        a = _f32(data, 2, "data")
        if a.shape[1] != self._dim:
            raise ValueError(f"dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        check(lib.lynse_hip_ivf_insert_f32(self._h, _ptr(a), a.shape[0]))

    def delete(self, rows) -> None:
        """`IVFIndex::delete` (ivf.rs:350-390): drop the listed rows; the rest are renumbered in order and reassigned."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint64)
        check(lib.lynse_hip_ivf_delete_rows(self._h, _ptr(r) if r.size else None, r.size))

    def assign(self, data) -> np.ndarray:
        a = _f32(data, 2, "data")
        out = np.zeros(a.shape[0], np.uint32)
        check(lib.lynse_hip_ivf_assign_f32(self._h, _ptr(a), a.shape[0], _ptr(out)))
        return out

    def export(self):
        n, nl = len(self), self.n_partitions
        cen = np.empty((nl, self._dim), np.float32)
        asg = np.empty(n, np.uint32)
        off = np.empty(nl + 1, np.uint64)
        orig = np.empty(n, np.uint32)
        check(lib.lynse_hip_ivf_export(self._h, _ptr(cen), _ptr(asg), _ptr(off), _ptr(orig)))
        return cen, asg, off, orig

    def thresholds(self):
        """Binary index: (BinaryQuantizer thresholds f32[dim], already_binary)."""
        t = np.empty(self._dim, np.float32)
        ab = C.c_int(0)
        check(lib.lynse_hip_ivf_thresholds(self._h, _ptr(t), C.byref(ab)))
        return t, bool(ab.value)

    def search_batch_arrays(self, queries, k: int, nprobe: int):
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_ivf_search_f32(self._h, _ptr(q), nq, k, int(nprobe), _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_filtered_batch_arrays(self, queries, k: int, nprobe: int, subset_rows):
        """`IVFIndex::search` with `SearchParams.subset` (ivf.rs:251-265), one subset for the batch."""
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        sub = np.ascontiguousarray(np.asarray(subset_rows).reshape(-1), dtype=np.uint64)
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_ivf_search_filtered_f32(self._h, _ptr(q), nq, k, int(nprobe), _ptr(sub) if sub.size else None, sub.size,
                                                    _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_metric_batch_arrays(self, queries, k: int, nprobe: int, metric):
        """`IvfFlatMmap::search(query, k, nprobe, metric)` (ivf_flat_mmap.rs:225-305): the metric of the CALL drives the
        centroid routing, the scoring and the sort direction — the partitions are metric-agnostic."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_ivf_search_metric_f32(self._h, _ptr(q), nq, k, int(nprobe), m, _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search(self, query, k: int = 10, nprobe: int = 10, metric: str = "ip"):
        """PyIvfFlatIndex.search (src/python/mod.rs:2130-2155): `metric` is the metric of this search."""
        m = metric_from_str(metric)  # ValueError on unknown names, like the reference
        q = _f32(query, 1, "query")
        if q.size != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.size}")
        rows, dists, counts = self.search_metric_batch_arrays(q.reshape(1, -1), k, nprobe, m)
        c = int(counts[0])
        return rows[0, :c].astype(np.uint32), dists[0, :c].copy()


class SpannIndex:
    """`SPANNIndex` (src/index/spann.rs): k-means centroids, every row in up to replica_count + 1 posting lists (boundary replicas),
    the lists as contiguous slabs in HBM; search scans the nprobe nearest lists and keeps the best k DISTINCT rows.  SQ8: lists of
    decoded rows, an exact rerank of a 10 k pool against the original rows.  The contract is in include/lynse_hip.h."""

    def __init__(self, handle, dim: int, sq8: bool, nprobe: int = 32):
        self._h = handle
        self._dim = dim
        self._sq8 = sq8
        self.nprobe = int(nprobe)   # the build default of a search with nprobe == 0

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.lynse_hip_ivf_destroy(h)

    @staticmethod
    def build(data, dim: int, n_clusters: int = 256, n_iters: int = 20, metric: str = "ip", replica_count: int = SPANN_DEFAULT_REPLICAS,
              sq8: bool = False, nprobe: int = 32, device: Optional[int] = None) -> "SpannIndex":
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        a = _f32(data, 2, "data")
        if a.shape[1] != dim:
            raise ValueError(f"data dimension mismatch: expected {dim}, got {a.shape[1]}")
        h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        check(lib.lynse_hip_spann_build(_ptr(a), a.shape[0], dim, int(n_clusters), int(n_iters), m, int(replica_count), 1 if sq8 else 0, dev,
                                        C.byref(h)))
        return SpannIndex(h, dim, bool(sq8), nprobe)

    @staticmethod
    def load(data, centroids, list_offsets, list_rows, replica_count: int, metric: str = "ip", mins=None, scales=None,
             device: Optional[int] = None, nprobe: int = 32) -> "SpannIndex":
        """`data`: the ORIGINAL rows; the lists as list-major CSR (`postings()` of a built index); (`mins`, `scales`) make it SQ8."""
        m = metric if isinstance(metric, int) else metric_from_str(metric)
        a = _f32(data, 2, "data")
        c = _f32(centroids, 2, "centroids")
        off = np.ascontiguousarray(np.asarray(list_offsets).reshape(-1), dtype=np.uint64)
        rows = np.ascontiguousarray(np.asarray(list_rows).reshape(-1), dtype=np.uint32)
        if off.size != c.shape[0] + 1:
            raise ValueError("list_offsets needs n_lists + 1 entries")
        sq8 = mins is not None
        mn = _f32(mins, 1, "mins") if sq8 else None
        sc = _f32(scales, 1, "scales") if sq8 else None
        h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        check(lib.lynse_hip_spann_load(_ptr(a), a.shape[0], a.shape[1], _ptr(c), c.shape[0], _ptr(off), _ptr(rows) if rows.size else None,
                                       int(replica_count), m, _ptr(mn) if sq8 else None, _ptr(sc) if sq8 else None, dev, C.byref(h)))
        return SpannIndex(h, a.shape[1], sq8, nprobe)

    def postings(self):
        """The posting lists as list-major CSR: (offsets u64[n_lists + 1], rows u32[postings]), rows ascending inside a list."""
        n = C.c_uint64(0)
        check(lib.lynse_hip_spann_postings(self._h, None, None, C.byref(n)))
        off = np.zeros(self.n_partitions + 1, np.uint64)
        rows = np.zeros(max(n.value, 1), np.uint32)
        check(lib.lynse_hip_spann_postings(self._h, _ptr(off), _ptr(rows), C.byref(n)))
        return off, rows[:n.value]

    @property
    def replica_count(self) -> int:
        out = C.c_uint32(0)
        check(lib.lynse_hip_spann_replica_count(self._h, C.byref(out)))
        return int(out.value)

    @property
    def is_sq8(self) -> bool:
        return self._sq8

    @property
    def dim(self) -> int:
        return self._dim

    def __len__(self) -> int:
        return int(lib.lynse_hip_ivf_len(self._h))

    @property
    def n_partitions(self) -> int:
        return int(lib.lynse_hip_ivf_nlist(self._h))

    def profile_enable(self, on=True) -> None:
        check(lib.lynse_hip_ivf_profile_enable(self._h, int(on)))

    def profile_get(self, reset: bool = True) -> dict:
        p = _lib.Profile()
        check(lib.lynse_hip_ivf_profile_get(self._h, C.byref(p), 1 if reset else 0))
        return {f: getattr(p, f) for f, _ in _lib.Profile._fields_}

    def sq8_params(self):
        mn = np.empty(self._dim, np.float32)
        sc = np.empty(self._dim, np.float32)
        check(lib.lynse_hip_ivf_sq8_params(self._h, _ptr(mn), _ptr(sc)))
        return mn, sc

    def sq8_stage_times(self, reset: bool = True) -> dict:
        out = np.zeros(3, np.float64)
        check(lib.lynse_hip_ivf_sq8_stage_times(self._h, _ptr(out), 1 if reset else 0))
        return {"searches": int(out[0]), "pool_us": float(out[1]), "rerank_us": float(out[2])}

    def insert(self, data) -> None:
        """`SPANNIndex::insert` (spann.rs:459-509): posting rule against the unchanged centroids, appended to the end of each list."""
        a = _f32(data, 2, "data")
        if a.shape[1] != self._dim:
            raise ValueError(f"dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        check(lib.lynse_hip_ivf_insert_f32(self._h, _ptr(a), a.shape[0]))

    def delete(self, rows) -> None:
        """`SPANNIndex::delete` (spann.rs:435-457): drop the rows, renumber the rest in order, rebuild every list."""
        r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint64)
        check(lib.lynse_hip_ivf_delete_rows(self._h, _ptr(r) if r.size else None, r.size))

    def _nprobe(self, nprobe) -> int:
        return self.nprobe if not nprobe else int(nprobe)

    def search_batch_arrays(self, queries, k: int, nprobe: int = 0):
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_ivf_search_f32(self._h, _ptr(q), nq, k, self._nprobe(nprobe), _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts

    def search_filtered_batch_arrays(self, queries, k: int, nprobe: int, subset_rows):
        q = _f32(queries, 2, "queries")
        if q.shape[1] != self._dim:
            raise ValueError(f"query dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        sub = np.ascontiguousarray(np.asarray(subset_rows).reshape(-1), dtype=np.uint64)
        nq, k = q.shape[0], int(k)
        rows = np.empty((nq, max(k, 1)), np.uint64)
        dists = np.empty((nq, max(k, 1)), np.float32)
        counts = np.zeros(nq, np.uint32)
        check(lib.lynse_hip_ivf_search_filtered_f32(self._h, _ptr(q), nq, k, self._nprobe(nprobe), _ptr(sub) if sub.size else None, sub.size,
                                                    _ptr(rows), _ptr(dists), _ptr(counts)))
        return rows[:, :k], dists[:, :k], counts


# ---------------------------------------------------------------------------------------------
# Sparse vectors (SparseVectorStore, src/engine.rs:550-718; index mode SPARSE-FLAT-IP)
# ---------------------------------------------------------------------------------------------
SPARSE_INDEX_MODE = "SPARSE-FLAT-IP"
SPARSE_VECTORS_FILE = "sparse_vectors.jsonl"


def normalize_sparse_vector(vector) -> list:
    """`_normalize_sparse_vector` (python/lynse/_backend.py:31-43): a dict {index: value} or an iterable of (index, value) pairs ->
    [(int index, float value)], in input order.  The values are cast to f32 and an index has to fit the core's u32."""
    items = vector.items() if isinstance(vector, dict) else vector
    out = []
    for item in items:
        if len(item) != 2:
            raise ValueError("sparse vector entries must be (index, value) pairs")
        index, value = item
        index = int(index)
        if index < 0:
            raise ValueError("sparse vector indices must be non-negative")
        if index > 0xFFFFFFFF:
            raise OverflowError("sparse vector index does not fit in u32")
        out.append((index, float(np.float32(value))))
    return out


def _sparse_csr(vectors) -> tuple:
    """[(index, value) lists] -> the raw CSR arrays (indptr u64, indices u32, values f32), entries as given"""
    lens = np.fromiter((len(v) for v in vectors), dtype=np.uint64, count=len(vectors))
    indptr = np.zeros(len(vectors) + 1, np.uint64)
    np.cumsum(lens, out=indptr[1:])
    flat = [e for v in vectors for e in v]
    indices = np.fromiter((e[0] for e in flat), dtype=np.uint32, count=len(flat))
    values = np.fromiter((e[1] for e in flat), dtype=np.float32, count=len(flat))
    return indptr, indices, values


def sparse_normalize_arrays(indptr, indices, values) -> tuple:
    """`normalize_sparse_entries` (engine.rs:6925-6943) for a batch in CSR, by lynse_hip_sparse_normalize (host code, no device): a
    non-finite value raises ValueError("sparse vector values must be finite"); zeros skipped, duplicates summed in input order,
    zero sums dropped, ascending indices -> (indptr, indices, values)."""
    indptr = np.ascontiguousarray(np.asarray(indptr).reshape(-1), dtype=np.uint64)
    indices = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.uint32)
    values = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.float32)
    if indptr.size == 0 or int(indptr[-1]) != indices.size or indices.size != values.size:
        raise ValueError("sparse CSR arrays do not match: indptr[-1], len(indices) and len(values) must agree")
    n = indptr.size - 1
    o_ptr = np.zeros(n + 1, np.uint64)
    o_idx = np.zeros(max(indices.size, 1), np.uint32)
    o_val = np.zeros(max(indices.size, 1), np.float32)
    check(lib.lynse_hip_sparse_normalize(_ptr(indptr), _ptr(indices), _ptr(values), n, _ptr(o_ptr), _ptr(o_idx), _ptr(o_val)))
    m = int(o_ptr[-1])
    return o_ptr, o_idx[:m].copy(), o_val[:m].copy()


class SparseIndex:
    """A CSR matrix of sparse rows in HBM and its exact inner-product scan (include/lynse_hip.h, SPARSE VECTORS): this build's
    device half of the reference's SparseVectorStore.  Rows and queries are NORMALISED vectors (sparse_normalize_arrays)."""

    def __init__(self, device: Optional[int] = None):
        self._h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        check(lib.lynse_hip_sparse_create(dev, C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.lynse_hip_sparse_destroy(h)

    @property
    def handle(self):
        return self._h

    @staticmethod
    def _csr(indptr, indices, values):
        indptr = np.ascontiguousarray(np.asarray(indptr).reshape(-1), dtype=np.uint64)
        indices = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.uint32)
        values = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.float32)
        if indptr.size == 0:
            indptr = np.zeros(1, np.uint64)
        if indices.size != values.size or int(indptr.max()) > indices.size:
            raise ValueError("sparse CSR arrays do not match: indptr must stay within len(indices) == len(values)")
        return indptr, indices, values

    def set_rows(self, indptr, indices, values) -> None:
        """Replaces the whole store with the rows of the CSR arrays (indptr u64[n + 1], indices u32, values f32)."""
        indptr, indices, values = self._csr(indptr, indices, values)
        check(lib.lynse_hip_sparse_set_rows(self._h, _ptr(indptr), _ptr(indices), _ptr(values), indptr.size - 1))

    def _len(self) -> tuple:
        rows, nnz = C.c_uint64(0), C.c_uint64(0)
        check(lib.lynse_hip_sparse_len(self._h, C.byref(rows), C.byref(nnz)))
        return int(rows.value), int(nnz.value)

    def __len__(self) -> int:
        return self._len()[0]

    @property
    def nnz(self) -> int:
        return self._len()[1]

    def hbm_bytes(self) -> int:
        return int(lib.lynse_hip_sparse_hbm_bytes(self._h))

    def search_batch_arrays(self, q_indptr, q_indices, q_values, k: int, words=None):
        """The rows with a non-zero inner product, best first by (score descending, row ascending) -> (rows u64[nq, k], scores
        f32[nq, k], counts u32[nq], passed u64[nq]): counts[q] = min(passed[q], k) entries valid, the rest row ~0 and -inf.  `words`
        are BitSet words over the sparse rows (None = every row)."""
        q_indptr, q_indices, q_values = self._csr(q_indptr, q_indices, q_values)
        nq, k = q_indptr.size - 1, int(k)
        if k < 0:
            raise ValueError("k must not be negative")
        rows = np.full((nq, k), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        scores = np.full((nq, k), -np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        passed = np.zeros(nq, np.uint64)
        if nq == 0:
            return rows, scores, counts, passed
        n_words = 0
        if words is not None:
            words = np.ascontiguousarray(np.asarray(words).reshape(-1), dtype=np.uint64)
            n_words = int(words.size)
            if n_words == 0:   # an empty mask is still a mask (NULL would mean every row)
                words = np.zeros(1, np.uint64)
        check(lib.lynse_hip_sparse_search(self._h, _ptr(q_indptr), _ptr(q_indices), _ptr(q_values), nq, k,
                                          None if words is None else _ptr(words), n_words, _ptr(rows), _ptr(scores), _ptr(counts), _ptr(passed)))
        return rows, scores, counts, passed

    def profile_enable(self, on=True) -> None:
        check(lib.lynse_hip_sparse_profile_enable(self._h, int(bool(on))))

    def profile_get(self, reset: bool = True) -> dict:
        p = _lib.Profile()
        check(lib.lynse_hip_sparse_profile_get(self._h, C.byref(p), 1 if reset else 0))
        return {f: getattr(p, f) for f, _ in _lib.Profile._fields_}


# ---------------------------------------------------------------------------------------------
# Text search (InvertedTextIndex, src/engine.rs:720-1118; index modes BM25-INVERTED, HYBRID-RRF, HYBRID-WEIGHTED)
# ---------------------------------------------------------------------------------------------
TEXT_INDEX_MODE = "BM25-INVERTED"
TEXT_SCAN_MODE = "BM25-SCAN"      # what the reference reports while no document holds text (engine.rs:5219-5223)
TEXT_MAX_TERMS = 256              # include/lynse_hip.h, TEXT SEARCH rule 3h


def tokenize_text(text: str) -> list:
    """`tokenize_text` / `normalize_text_token` (engine.rs:7031-7049): split at every character that is not alphanumeric, drop the
    empty pieces, keep an ASCII token without an upper-case letter as it is and lower-case any other.  `str.isalnum` stands for
    Rust's `char::is_alphanumeric`: equal on ASCII and wherever Alphabetic ∪ N* coincides with it (DESIGN §20 names the divergence)."""
    out, cur = [], []
    for ch in text:
        if ch.isalnum():
            cur.append(ch)
        elif cur:
            out.append("".join(cur))
            cur = []
    if cur:
        out.append("".join(cur))
    return [t if t.isascii() and not any("A" <= c <= "Z" for c in t) else t.lower() for t in out]


def text_term_counts(value, counts: Optional[dict] = None) -> dict:
    """`append_searchable_json_terms` (engine.rs:7051-7068): the term counts of the strings in a JSON-like value, lists and dict
    values followed; None, bool, int and float contribute nothing."""
    counts = {} if counts is None else counts
    if isinstance(value, str):
        for t in tokenize_text(value):
            counts[t] = counts.get(t, 0) + 1
    elif isinstance(value, (list, tuple)):
        for v in value:
            text_term_counts(v, counts)
    elif isinstance(value, dict):
        for v in value.values():
            text_term_counts(v, counts)
    return counts   # (None, bool — tested before int by not being tested at all —, int, float: nothing)


def index_text_document(fields: dict) -> dict:
    """`index_document` (engine.rs:1077-1107): {field: {term: tf}} for the top-level fields of length > 0; {} = not indexed."""
    doc = {}
    for name, value in fields.items():
        counts = text_term_counts(value)
        if counts:
            doc[str(name)] = counts
    return doc


def text_weights(docs: int, total: int, df, count, k: int) -> tuple:
    """Rules b, d and e of TEXT SEARCH by lynse_hip_text_weights (host code, no device) -> (avg f32, w f32[T], cand u32[T])."""
    df = np.ascontiguousarray(np.asarray(df).reshape(-1), dtype=np.uint64)
    count = np.ascontiguousarray(np.asarray(count).reshape(-1), dtype=np.uint32)
    if df.size != count.size:
        raise ValueError("df and count must have one entry per term")
    avg = C.c_float(0.0)
    w, cand = np.zeros(max(df.size, 1), np.float32), np.zeros(max(df.size, 1), np.uint32)
    check(lib.lynse_hip_text_weights(int(docs), int(total), _ptr(df), _ptr(count), df.size, int(k), C.byref(avg), _ptr(w), _ptr(cand)))
    return np.float32(avg.value), w[:df.size], cand[:df.size]


def normalize_scores(scores, ascending: bool) -> np.ndarray:
    """`normalize_scores` (engine.rs:7188-7217) on f32: min and max over the finite scores; all 1.0 when there is none or
    |max - min| <= FLT_EPSILON; else clamp((s - min) / (max - min), 0, 1), and 1 - x for an ascending metric."""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    fin = s[np.isfinite(s)]
    if s.size == 0:
        return s.copy()
    if fin.size == 0 or np.abs(np.float32(fin.max() - fin.min())) <= np.finfo(np.float32).eps:
        return np.ones(s.size, np.float32)
    lo, span = fin.min(), np.float32(fin.max() - fin.min())
    with np.errstate(all="ignore"):
        x = np.clip(((s - lo) / span).astype(np.float32), np.float32(0.0), np.float32(1.0))
        return (np.float32(1.0) - x).astype(np.float32) if ascending else x


def hybrid_fuse(vector_leg, text_leg, k: int, fusion: str = "rrf", vector_weight: float = 1.0, text_weight: float = 1.0,
                rrf_k: float = 60.0, ascending: bool = False) -> tuple:
    """The fusion of `hybrid_search` (engine.rs:5100-5145; add_fused_scores, :7219-7237) on numpy f32 scalars in the reference's
    operation order.  A leg is (ids, scores) best first, or None; the vector leg is normalised with `ascending`, the text leg never
    is ascending.  Rank r (from 0) of a leg adds score * weight ("weighted", case-insensitive) or weight / ((max(rrf_k, 1) + r) + 1)
    to its id; sums start at 0 and take the vector leg first.  Order: fused descending, id ascending (the reference leaves ties to
    hash order); cut at k -> (ids i64, fused f32)."""
    f32 = np.float32
    weighted = str(fusion).lower() == "weighted"
    fused: dict = {}
    for leg, weight, asc in ((vector_leg, vector_weight, ascending), (text_leg, text_weight, False)):
        if leg is None:
            continue
        ids, scores = leg
        norm = normalize_scores(scores, asc)
        wt = max(f32(weight), f32(0.0))
        base = max(f32(rrf_k), f32(1.0))
        for r, i in enumerate(np.asarray(ids).reshape(-1)):
            c = f32(norm[r] * wt) if weighted else f32(wt / f32(f32(base + f32(r)) + f32(1.0)))
            fused[int(i)] = f32(fused.get(int(i), f32(0.0)) + c)
    order = sorted(fused.items(), key=lambda e: (-float(e[1]), e[0]))[:max(int(k), 0)]
    return np.array([e[0] for e in order], np.int64), np.array([e[1] for e in order], np.float32)


class TextIndex:
    """The posting lists of one field selection in HBM and their BM25 scan (include/lynse_hip.h, TEXT SEARCH): this build's device
    half of the reference's InvertedTextIndex.  Rows are documents, terms are ids; tokenising and field selection are the caller's."""

    def __init__(self, device: Optional[int] = None):
        self._h = C.c_void_p()
        dev = default_device() if device is None else int(device)
        check(lib.lynse_hip_text_create(dev, C.byref(self._h)))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            lib.lynse_hip_text_destroy(h)

    @property
    def handle(self):
        return self._h

    def set(self, doc_len, term_ptr, post_row, post_tf) -> None:
        """Replaces the whole store: doc_len u32[n], and the postings in CSC form (term_ptr u64[V + 1], post_row u32, post_tf u32)."""
        doc_len = np.ascontiguousarray(np.asarray(doc_len).reshape(-1), dtype=np.uint32)
        term_ptr = np.ascontiguousarray(np.asarray(term_ptr).reshape(-1), dtype=np.uint64)
        post_row = np.ascontiguousarray(np.asarray(post_row).reshape(-1), dtype=np.uint32)
        post_tf = np.ascontiguousarray(np.asarray(post_tf).reshape(-1), dtype=np.uint32)
        if term_ptr.size == 0:
            term_ptr = np.zeros(1, np.uint64)
        if post_row.size != post_tf.size or int(term_ptr.max()) > post_row.size:
            raise ValueError("text postings do not match: term_ptr must stay within len(post_row) == len(post_tf)")
        check(lib.lynse_hip_text_set(self._h, _ptr(doc_len), doc_len.size, _ptr(term_ptr), term_ptr.size - 1, _ptr(post_row), _ptr(post_tf)))

    def _len(self) -> tuple:
        rows, terms, nnz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        check(lib.lynse_hip_text_len(self._h, C.byref(rows), C.byref(terms), C.byref(nnz)))
        return int(rows.value), int(terms.value), int(nnz.value)

    def __len__(self) -> int:
        return self._len()[0]

    @property
    def terms(self) -> int:
        return self._len()[1]

    @property
    def nnz(self) -> int:
        return self._len()[2]

    def hbm_bytes(self) -> int:
        return int(lib.lynse_hip_text_hbm_bytes(self._h))

    def search_batch_arrays(self, q_ptr, q_terms, q_counts, k: int, words=None):
        """BM25 for nq queries in CSR of (term id, count) in slot order -> (rows u64[nq, k], scores f32[nq, k], counts u32[nq],
        passed u64[nq]): counts[q] = min(passed[q], k) entries valid, best first by (score descending, row ascending), the rest row
        ~0 and -inf.  `words` are BitSet words over the text rows (None = every row)."""
        q_ptr = np.ascontiguousarray(np.asarray(q_ptr).reshape(-1), dtype=np.uint64)
        q_terms = np.ascontiguousarray(np.asarray(q_terms).reshape(-1), dtype=np.uint32)
        q_counts = np.ascontiguousarray(np.asarray(q_counts).reshape(-1), dtype=np.uint32)
        if q_ptr.size == 0:
            q_ptr = np.zeros(1, np.uint64)
        if q_terms.size != q_counts.size or int(q_ptr.max()) > q_terms.size:
            raise ValueError("text query arrays do not match: q_ptr must stay within len(q_terms) == len(q_counts)")
        nq, k = q_ptr.size - 1, int(k)
        if k < 0:
            raise ValueError("k must not be negative")
        rows = np.full((nq, k), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        scores = np.full((nq, k), -np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        passed = np.zeros(nq, np.uint64)
        if nq == 0:
            return rows, scores, counts, passed
        n_words = 0
        if words is not None:
            words = np.ascontiguousarray(np.asarray(words).reshape(-1), dtype=np.uint64)
            n_words = int(words.size)
            if n_words == 0:   # an empty mask is still a mask (NULL would mean every row)
                words = np.zeros(1, np.uint64)
        check(lib.lynse_hip_text_search(self._h, _ptr(q_ptr), _ptr(q_terms), _ptr(q_counts), nq, k,
                                        None if words is None else _ptr(words), n_words, _ptr(rows), _ptr(scores), _ptr(counts), _ptr(passed)))
        return rows, scores, counts, passed

    def profile_enable(self, on=True) -> None:
        check(lib.lynse_hip_text_profile_enable(self._h, int(bool(on))))

    def profile_get(self, reset: bool = True) -> dict:
        p = _lib.Profile()
        check(lib.lynse_hip_text_profile_get(self._h, C.byref(p), 1 if reset else 0))
        return {f: getattr(p, f) for f, _ in _lib.Profile._fields_}


def py_compute_distance(a, b, metric: str) -> float:
    """src/python/mod.rs:2161-2185."""
    m = metric_from_str(metric)
    a = _f32(a, 1, "a")
    b = _f32(b, 1, "b")
    if a.size != b.size:
        raise ValueError("Vector dimensions must match")
    out = C.c_float(0.0)
    check(lib.lynse_hip_compute_distance(_ptr(a), _ptr(b), a.size, m, default_device(), C.byref(out)))
    return float(out.value)


def py_top_k_search(query, candidates, metric: str, k: int):
    """src/python/mod.rs:2189-2223 -> (indices u32[], distances f32[])."""
    m = metric_from_str(metric)
    q = _f32(query, 1, "query")
    c = _f32(candidates, 2, "candidates")
    if q.size != c.shape[1]:
        raise ValueError("Query dimension must match candidate dimension")
    k = int(k)
    idx = np.empty(max(k, 1), np.uint32)
    dist = np.empty(max(k, 1), np.float32)
    cnt = C.c_uint32(0)
    check(lib.lynse_hip_top_k_search(_ptr(q), _ptr(c), c.shape[0], c.shape[1], k, m, default_device(),
                                     _ptr(idx), _ptr(dist), C.byref(cnt)))
    return idx[:cnt.value].copy(), dist[:cnt.value].copy()


def merge_topk(ids, dists, counts, k: int, metric) -> tuple:
    """VectorStore::merge_results (vector_store.rs:953-970) over per-shard blocks [n_lists, stride]."""
    m = metric if isinstance(metric, int) else metric_from_str(metric)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    dists = np.ascontiguousarray(dists, dtype=np.float32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n_lists, stride = ids.shape
    out_i = np.empty(max(k, 1), np.uint64)
    out_d = np.empty(max(k, 1), np.float32)
    cnt = C.c_uint32(0)
    check(lib.lynse_hip_merge_topk(_ptr(ids), _ptr(dists), _ptr(counts), n_lists, stride, int(k), m,
                                   _ptr(out_i), _ptr(out_d), C.byref(cnt)))
    return out_i[:cnt.value].copy(), out_d[:cnt.value].copy()


# ---------------------------------------------------------------------------------------------
# Minimal engine glue: only what `benchmarks/flat_search_bench.py:43-96` and the reference's
# search tests drive.  Storage/WAL/fields/filters are out of scope.
# ---------------------------------------------------------------------------------------------
class SearchResult:
    """src/python/mod.rs:1876-1921 / engine.rs:6895-6902."""

    def __init__(self, ids: np.ndarray, distances: np.ndarray, index_mode: str, dimension: int, k: int):
        self._ids = np.asarray(ids, dtype=np.int64)
        self._d = np.asarray(distances, dtype=np.float32)
        self._mode, self._dim, self._k = index_mode, dimension, k

    def ids(self) -> np.ndarray:
        return self._ids

    def distances(self) -> np.ndarray:
        return self._d

    def fields(self) -> list:
        return []

    def index_mode(self) -> str:
        return self._mode

    def to_tuple(self):
        return self._ids, self._d, []

    def __len__(self) -> int:
        return int(self._ids.size)

    def __repr__(self) -> str:
        return f"SearchResult(n={len(self)}, k={self._k}, dim={self._dim}, index={self._mode})"


PENDING_INGEST_FLUSH_ROWS = 10_000              # src/engine.rs:93
PENDING_INGEST_FLUSH_BYTES = 32 * 1024 * 1024   # src/engine.rs:94


class BitSet:
    """Row subset in the reference's layout (src/storage/bitset.rs): u64 words, bit r of word r // 64 = row r."""

    def __init__(self, n_rows: int, words: Optional[np.ndarray] = None):
        self.n_rows = int(n_rows)
        nw = (self.n_rows + 63) // 64
        self.words = np.zeros(nw, np.uint64) if words is None else np.ascontiguousarray(words, dtype=np.uint64)
        if self.words.size != nw:
            raise ValueError("BitSet words do not match the row count")

    @staticmethod
    def from_rows(rows, n_rows: int) -> "BitSet":
        b = BitSet(n_rows)
        r = np.unique(np.asarray(rows, dtype=np.uint64).reshape(-1))
        r = r[r < np.uint64(n_rows)]
        np.bitwise_or.at(b.words, (r >> np.uint64(6)).astype(np.int64), np.uint64(1) << (r & np.uint64(63)))
        return b

    def count(self) -> int:
        return int(np.unpackbits(self.words.view(np.uint8)).sum())

    def contains(self, row: int) -> bool:
        return 0 <= row < self.n_rows and bool((int(self.words[row >> 6]) >> (row & 63)) & 1)

    def to_vec(self) -> np.ndarray:
        bits = np.unpackbits(self.words.view(np.uint8), bitorder="little")
        return np.nonzero(bits)[0].astype(np.uint64)


class ResolvedWhere:
    """A `where=` evaluated against a collection: the predicate, the flushed rows it was evaluated over (their BitSet words are in
    the collection's FieldFilter until its next filter), the matches among them, the matching pending rows, and the time it took."""
    __slots__ = ("pred", "n_flat", "count", "pending", "us", "rows")

    def __init__(self, pred, n_flat: int, count: int, pending: np.ndarray, us: int):
        self.pred, self.n_flat, self.count, self.pending, self.us, self.rows = pred, n_flat, count, pending, us, None


class Collection:
    """The search-path subset of `lynse._core.Collection` (engine.rs Collection): buffered ingest, commit, index build
    and `search / batch_search` = `search_with_precomputed_filter` (src/engine.rs:4718-4833): k inflated by the
    tombstone count, the index / flat / subset-filtered search over the flushed rows on the GPU, the pending (not yet
    flushed) rows scored with `top_k_search`, `merge_row_results`, row -> user id, `filter_tombstoned_limit`.

    The reference resolves `where_expr` to a row BitSet through its field store; the precomputed filter is passed here as `subset=` (a
    `BitSet` or an array of row indices), and the reference's indexed filter dialect as `where=` (lynsedb_amd/fields.py):
    the `fields` of add_items / upsert_items are kept as typed columns, row-aligned with the shard, the predicate is evaluated for the
    flushed rows by k_field_filter on the device and for the pending rows on the host.  A search with `where=` returns exactly what
    the same search returns with `subset=` set to the rows the filter selects.  `where=` together with `subset=` is an error.
    `where_expr=` keeps the answer existing tests pin (NotImplementedError): `where=` is the name python/lynse/api/local_client.py
    gives the filter, and the name this build answers."""

    def __init__(self, name: str, dim: int, device: Optional[int] = None, path=None):
        self._name, self._dim = name, int(dim)
        self._device = device
        self._path = None if path is None else Path(path)   # where the auxiliary index file (rabitq_index.bin, polarvec_index.bin) persists; None = nowhere
        self._flat = FlatIndex(None, dim, device)
        self._id_arrays: list = []     # row -> user id (engine.rs:3071-3073)
        self._index_mode = "FLAT-IP"   # resolve_metric default IP (engine.rs:5529-5534)
        self._metric = _lib.METRIC_IP
        self._ivf = None                # IvfFlatIndex, or SpannIndex for the SPANN-* modes
        self._ivf_rows = 0              # rows the IVF index was built over
        self._ivf_params: dict = {}
        self._ivf_nprobe = 32           # IndexBuildOptions default (src/index/mod.rs:498-655)
        self._pending_vecs: list = []   # PendingIngestBuffer (engine.rs:125, :190-245)
        self._pending_ids: list = []
        self._pending_rows = 0
        self._tombstone: set = set()    # user ids (engine.rs:3182-3194)
        self._pq = False                # FLAT-*-PQ built over the rows flushed at build time (FlatIndex.build_pq)
        self._pq_clusters = 256         # the n_clusters it was built with (a rebuild after a mutation uses it again)
        self._index_dirty = False       # rows changed under an index while the shard was empty: rebuilt by the first search over rows
        self._rabitq = False            # FLAT-*-RABITQ, likewise (FlatIndex.build_rabitq); at most one of the two exists
        self._polarvec = 0              # FLAT-*-POLARVEC<b>, likewise: the bit count (FlatIndex.build_polarvec), 0 = none
        self._hnsw = False              # HNSW-*: a graph over the flushed rows (FlatIndex.build_hnsw); replaces and is replaced by the two above
        self._hnsw_rows = 0             # rows the graph was built over
        self._hnsw_opts: dict = {}
        self._approx_info = None        # what the last approximate flat search ran (FlatIndex.search_approx), for search_profile
        self._diskann = False           # DISKANN-*: likewise (FlatIndex.build_diskann); at most one of the four exists
        self._diskann_rows = 0
        self._diskann_opts: dict = {}
        self._sparse: dict = {}         # user id -> (indices u32, values f32), normalised (SparseVectorStore.vectors)
        self._sparse_ids = np.zeros(0, np.int64)   # the ids of the uploaded sparse rows, ascending: sparse row -> user id
        self._sparse_index = None       # SparseIndex, created by the first sparse search
        self._sparse_dirty = False      # the store changed since the last upload
        self._docs: dict = {}           # user id -> {field: {term: tf}} (InvertedTextIndex.postings / doc_lengths), flushed or pending rows alike
        self._text_index = None         # TextIndex, created by the first text search
        self._text_key = None           # the field selection the device store holds: () = all fields, else the sorted names
        self._text_dirty = True         # the documents changed since the last upload
        self._text_ids = np.zeros(0, np.int64)   # the ids of the uploaded text rows, ascending: text row -> user id
        self._text_vocab: dict = {}     # term -> term id of the uploaded store
        self._fields = FieldTable()     # the fields of every row as typed columns, flushed and pending rows alike (the host copy is authoritative)
        self._field_filter = None       # FieldFilter (the device copy of the columns + k_field_filter), created by the first `where=`
        self._vfields: dict = {}        # name -> NamedVectorField (the named vector fields)
        self._row_stamp = 0             # bumped when the id -> row resolution may have changed (flush, upsert, compact): the fields' row_of follow

    def name(self) -> str:
        return self._name

    # -- ingest -------------------------------------------------------------------------------
    def add_items(self, vectors, ids: Sequence[int], fields=None) -> None:
        """Buffered like the reference (engine.rs:3886-3900): rows wait in the pending buffer until it holds
        PENDING_INGEST_FLUSH_ROWS rows / PENDING_INGEST_FLUSH_BYTES bytes, or until commit(); searches see them through
        `pending_search`."""
        a = _f32(vectors, 2, "vectors")
        if a.shape[1] != self._dim:
            raise RuntimeError(f"Dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        if len(ids) != a.shape[0]:
            raise RuntimeError("ids length must match the number of vectors")
        if fields is not None:   # the text index (insert_documents, engine.rs:882-908) and the field columns of `where=`
            fields = list(fields)
            if len(fields) != len(ids):
                raise RuntimeError(f"Invalid argument: ids length ({len(ids)}) must match field count ({len(fields)})")
            if not all(isinstance(f, dict) for f in fields):
                raise TypeError("fields must be a list of dicts, one per id")
            self._index_docs(ids, fields)
        if a.shape[0] == 0:
            return
        id_arr = np.asarray(ids, dtype=np.int64).copy()
        self._fields.append(fields, a.shape[0])   # the columns grow with the rows (a row added without fields has every field missing)
        self._pending_vecs.append(np.array(a, dtype=np.float32, copy=True))
        self._pending_ids.append(id_arr)
        self._pending_rows += a.shape[0]
        if self._pending_rows >= PENDING_INGEST_FLUSH_ROWS or self._pending_rows * self._dim * 4 >= PENDING_INGEST_FLUSH_BYTES:
            self._flush_pending()

    def _index_docs(self, ids, fields) -> None:
        """The text documents of a batch (insert_documents / upsert_documents): one document per id replaces the id's earlier one."""
        for i, f in zip(ids, fields):
            doc = index_text_document(f)
            if doc:
                self._docs[int(i)] = doc
                self._text_dirty = True
            elif self._docs.pop(int(i), None) is not None:   # a document with no text field left is not indexed: a re-added id loses its old one
                self._text_dirty = True

    def pending_len(self) -> int:
        return self._pending_rows

    def _flush_pending(self) -> None:  # Collection::flush_pending_ingest (engine.rs:3573-3590)
        for a, i in zip(self._pending_vecs, self._pending_ids):
            self._flat.write(a)
            self._id_arrays.append(i)
        self._pending_vecs, self._pending_ids, self._pending_rows = [], [], 0
        self._row_stamp += 1

    def commit(self) -> None:
        self._flush_pending()
        self._flat.finalize()

    def shape(self):
        return (len(self._flat) + self._pending_rows, self._dim)

    def _id_map(self) -> np.ndarray:
        if len(self._id_arrays) != 1:
            self._id_arrays = [np.concatenate(self._id_arrays) if self._id_arrays else np.zeros(0, np.int64)]
        return self._id_arrays[0]

    # -- soft deletes (engine.rs:3182-3284) -----------------------------------------------------
    def delete_items(self, ids: Iterable[int]) -> None:
        self._tombstone.update(int(i) for i in ids)

    def restore_items(self, ids: Iterable[int]) -> None:
        self._tombstone.difference_update(int(i) for i in ids)

    def list_deleted_ids(self) -> list:
        return sorted(self._tombstone)

    # -- mutation (engine.rs:5880-6103, :6353-6401, :6494-6596) ---------------------------------
    def _rows_of_ids(self, ids: np.ndarray) -> np.ndarray:
        """The flushed row of each id, -1 for an id without one.  This mirror's add_items accepts an id twice (the reference does
        not, engine.rs:3505-3512): an id of the call that is stored in more than one row is an error here."""
        id_map = self._id_map()
        order = np.argsort(id_map, kind="stable")
        sorted_ids = id_map[order]
        lo, hi = np.searchsorted(sorted_ids, ids, "left"), np.searchsorted(sorted_ids, ids, "right")
        twice = np.nonzero(hi - lo > 1)[0]
        if twice.size:
            raise RuntimeError(f"Invalid argument: id {int(ids[twice[0]])} is stored in more than one row")
        rows = np.full(ids.size, -1, np.int64)
        hit = hi > lo
        rows[hit] = order[lo[hit]]
        return rows

    @staticmethod
    def _unique_ids(ids) -> np.ndarray:
        ids = np.asarray([int(i) for i in ids], dtype=np.int64)   # validate_unique_ids
        seen = set()
        for i in ids.tolist():
            if i in seen:
                raise RuntimeError(f"Invalid argument: duplicate id {i} within the same insert batch")
            seen.add(i)
        return ids

    def _rebuild_index(self) -> None:
        """Whatever index the collection holds, built again over the flushed rows with the mode and options it was built with: a search
        after a mutation equals a search on a collection that was given the final rows.  Over an empty shard nothing can be built:
        the first search that finds rows does it."""
        self._index_dirty = len(self._flat) == 0 and (self._ivf is not None or self._pq or self._rabitq or self._polarvec or self._hnsw or self._diskann)
        if len(self._flat) == 0:
            return
        if self._ivf is not None:
            self._build_ivf()
        elif self._hnsw:
            self._build_hnsw()
        elif self._diskann:
            self._build_diskann()
        elif self._pq:
            self._flat.build_pq(parse_n_subspaces(self._index_mode, self._dim), self._pq_clusters)
        elif self._rabitq:
            self._flat.build_rabitq()
            self._save_rabitq()
        elif self._polarvec:   # (the reference rebuilds it after a mutation too: engine.rs:5921-5934)
            self._flat.build_polarvec(self._polarvec, self._metric)
            self._save_polarvec()

    def upsert_items(self, vectors, ids: Sequence[int], fields=None) -> None:
        """Collection::upsert_items (engine.rs:5949-6066): existing ids are rewritten in place on the device and leave the tombstone
        set, new ids are appended and flushed.  With `fields`, an id's text document is replaced by the rule of add_items.  When an
        existing row changed, the index of the collection is built again (the reference rebuilds the quantised modes only and leaves
        IVF and HNSW on the old vectors: DESIGN.md §22)."""
        self._flush_pending()
        a = _f32(vectors, 2, "vectors")
        if a.shape[1] != self._dim:
            raise RuntimeError(f"Dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        if len(ids) != a.shape[0]:
            raise RuntimeError("Invalid argument: ids length must match n_vectors")
        if fields is not None:
            fields = list(fields)
            if len(fields) != len(ids):
                raise RuntimeError(f"Invalid argument: fields length ({len(fields)}) must match n_vectors ({len(ids)})")
            if not all(isinstance(f, dict) for f in fields):
                raise TypeError("fields must be a list of dicts, one per id")
        ids = self._unique_ids(ids)
        rows = self._rows_of_ids(ids)
        old, new = np.nonzero(rows >= 0)[0], np.nonzero(rows < 0)[0]
        if old.size:
            self._flat.update_rows(rows[old].astype(np.uint64), a[old])
            self._tombstone.difference_update(ids[old].tolist())
            if fields is not None:   # fields replace the row's fields only when given
                self._index_docs(ids[old].tolist(), [fields[j] for j in old.tolist()])
                for j in old.tolist():
                    self._fields.set_row(int(rows[j]), fields[j])
        if new.size:
            self.add_items(a[new], ids[new], None if fields is None else [fields[j] for j in new.tolist()])
            self._flush_pending()
        self._row_stamp += 1   # (the named fields keep their vectors: the reference's upsert paths never touch named_vector_fields)
        if old.size:
            self._rebuild_index()

    def update_items(self, vectors, ids: Sequence[int], fields=None) -> None:
        """Collection::update_items (engine.rs:6072-6103): every id must exist; then upsert_items."""
        self._flush_pending()
        a = _f32(vectors, 2, "vectors")
        if a.shape[1] != self._dim:
            raise RuntimeError(f"Dimension mismatch: expected {self._dim}, got {a.shape[1]}")
        if len(ids) != a.shape[0]:
            raise RuntimeError("Invalid argument: ids length must match n_vectors")
        uids = self._unique_ids(ids)
        missing = np.nonzero(self._rows_of_ids(uids) < 0)[0]
        if missing.size:
            raise RuntimeError(f"Invalid argument: id {int(uids[missing[0]])} does not exist; use upsert_items to insert missing IDs")
        self.upsert_items(a, uids, fields)

    def compact(self) -> int:
        """Collection::compact (engine.rs:6494-6596): every flushed row of a tombstoned id is dropped on the device, in place; the id
        map follows, the ids leave the sparse store and the text documents, the tombstone set is cleared (an id without a row is
        simply forgotten) and the index is built again.  Returns the rows removed; 0, and no change, without tombstones."""
        self._flush_pending()
        if not self._tombstone:
            return 0
        dead_ids = np.fromiter(self._tombstone, dtype=np.int64, count=len(self._tombstone))
        id_map = self._id_map()
        keep = ~np.isin(id_map, dead_ids)
        removed = int(id_map.size - np.count_nonzero(keep))
        if removed:
            new_len = self._flat.compact(keep)
            self._id_arrays = [id_map[keep]]
            assert new_len == self._id_arrays[0].size
            self._fields.keep(keep)
        for i in self._tombstone:
            if self._sparse.pop(i, None) is not None:
                self._sparse_dirty = True
            if self._docs.pop(i, None) is not None:
                self._text_dirty = True
        if self._sparse_dirty and self._path is not None:
            from .storage import save_sparse_vectors

            save_sparse_vectors(self._path / SPARSE_VECTORS_FILE, self._sparse)
        if self._vfields:
            self._compact_vector_fields(dead_ids)
        self._row_stamp += 1
        self._tombstone.clear()
        self._rebuild_index()
        return removed

    def read_vectors_by_ids(self, ids: Sequence[int]) -> np.ndarray:
        """read_vectors_by_ids_only (engine.rs:6353-6401): the vector of each id, flushed rows gathered on the device, pending rows from
        the buffer."""
        ids = np.asarray([int(i) for i in ids], dtype=np.int64)
        rows = self._rows_of_ids(ids)
        out = np.empty((ids.size, self._dim), np.float32)
        flushed = np.nonzero(rows >= 0)[0]
        if flushed.size:
            out[flushed] = self._flat.gather_rows(rows[flushed].astype(np.uint64))
        rest = np.nonzero(rows < 0)[0]
        if rest.size:
            p_ids = np.concatenate(self._pending_ids) if self._pending_ids else np.zeros(0, np.int64)
            p_vecs = np.concatenate(self._pending_vecs) if self._pending_vecs else np.zeros((0, self._dim), np.float32)
            for j in rest.tolist():
                at = np.nonzero(p_ids == ids[j])[0]
                if at.size == 0:
                    raise RuntimeError(f"Invalid argument: vector id {int(ids[j])} does not exist")
                if at.size > 1:
                    raise RuntimeError(f"Invalid argument: id {int(ids[j])} is stored in more than one row")
                out[j] = p_vecs[at[0]]
        return out

    # -- index --------------------------------------------------------------------------------
    def build_index(self, index_type: str, params: Optional[dict] = None) -> None:
        """Collection::build_index_with_build_options (engine.rs:4515-4655): flushes the pending rows (:4521); FLAT-*
        keeps no index object (engine.rs:4559-4567; `FLAT-*-SQ8` switches the flat scan to the SQ8 two-pass mode,
        flat_mmap.rs:891-905); IVF-* trains a k-means IVFIndex (engine.rs:4616-4627), `IVF-{HAMMING,JACCARD}-BINARY`
        the binary-quantised one (src/index/mod.rs:376-385)."""
        mode = str(index_type).upper()
        additive = additive_mode_of(mode)   # (refuses every other mode that names one of the four additive metrics)
        try:
            metric = metric_from_index_mode(mode)
        except NotImplementedError:
            raise
        except ValueError as e:
            raise RuntimeError(str(e))
        params = dict(params or {})
        self._flush_pending()
        if additive is not None:   # FLAT-L1 ... FLAT-BRAYCURTIS: no index object, no auxiliary index, the exact scan of the metric
            self._ivf = None
            self._drop_aux()
            metric = additive
        elif mode.startswith("FLAT"):
            rabitq = flat_rabitq_mode(mode)   # (refuses the bare POLARVEC token)
            pq = flat_pq_mode(mode)
            polarvec = flat_polarvec_mode(mode)
            self._ivf = None
            self._drop_aux()   # building any mode drops an earlier PQ / RaBitQ index (engine.rs:4476, :4552, :4559-4600)
            if pq and len(self._flat) > 0:   # over 0 rows nothing is built and searches stay exact
                self._pq_clusters = int(params.get("n_clusters", 256))
                self._flat.build_pq(parse_n_subspaces(mode, self._dim), self._pq_clusters)
                self._pq = True
            elif rabitq and len(self._flat) > 0:
                self._flat.build_rabitq()
                self._rabitq = True
                self._save_rabitq()
            elif polarvec and len(self._flat) > 0:   # PQ, then RaBitQ, then PolarVec (engine.rs:4559-4600)
                self._flat.build_polarvec(polarvec, metric)
                self._polarvec = polarvec
                self._save_polarvec()
        elif hnsw_mode_of(mode) is not None:   # HNSW-{IP,L2,COS,COSINE}; every other HNSW-* name falls through to the refusal below
            opts = hnsw_build_options(params)
            self._ivf = None
            self._drop_aux()
            if len(self._flat) == 0:   # graph / partition indexes need data (engine.rs:4606-4612)
                raise ValueError("Empty database")
            self._hnsw_opts = opts
            self._metric = metric
            self._build_hnsw()
        elif diskann_mode_of(mode) is not None:   # DISKANN-{L2,COS,COSINE}; DISKANN-IP and the -PQ* / -SQ8 names fall through to the refusal below
            opts = diskann_build_options(params)
            self._ivf = None
            self._drop_aux()
            if len(self._flat) == 0:   # graph / partition indexes need data (engine.rs:4606-4612)
                raise ValueError("Empty database")
            self._diskann_opts = opts
            self._metric = metric
            self._build_diskann()
        elif mode.startswith("SPANN"):
            metric, sq8 = spann_mode_of(mode)
            opts = spann_build_options(params)
            self._drop_aux()
            if len(self._flat) == 0:   # graph / partition indexes need data (engine.rs:4606-4612)
                raise ValueError("Empty database")
            self._ivf_params = {"n_clusters": opts["n_clusters"], "spann": (opts["replica_count"], sq8)}
            self._ivf_nprobe = opts["nprobe"]
            self._index_mode, self._metric = mode, metric
            self._build_ivf()
        elif mode.startswith("IVF"):
            quantizer = ivf_quantizer_of(mode)
            self._drop_aux()
            self._ivf_params = {"n_clusters": int(params.get("n_clusters", 256)), "quantizer": quantizer}
            self._ivf_nprobe = int(params.get("nprobe", 32))
            self._index_mode, self._metric = mode, metric
            self._build_ivf()
        else:
            raise NotImplementedError(f"index type {index_type} is outside the FLAT/IVF hot path")
        self._index_mode, self._metric = mode, metric
        self._index_dirty = False

    def _drop_aux(self) -> None:
        """At most one auxiliary quantised index exists: whatever is built next, the earlier one and its file go."""
        self._flat.drop_pq()
        self._flat.drop_rabitq()
        self._flat.drop_polarvec()
        self._flat.drop_hnsw()
        self._flat.drop_diskann()
        self._pq = self._rabitq = self._hnsw = self._diskann = False
        self._polarvec = 0
        if self._path is not None:
            (self._path / RABITQ_INDEX_FILE).unlink(missing_ok=True)
            (self._path / POLARVEC_INDEX_FILE).unlink(missing_ok=True)

    def _save_rabitq(self) -> None:
        if self._path is None:
            return
        from .storage import RabitqIndexFile, save_rabitq_index

        p = self._flat.rabitq_params()
        save_rabitq_index(self._path / RABITQ_INDEX_FILE, RabitqIndexFile(p["dim"], p["padded_dim"], p["sign_words"], p["codes"], p["norms"]))

    def try_load_rabitq(self, index_type: str) -> bool:
        """try_load_pq_rabitq's RaBitQ half for a reopened collection whose rows are back in place: `index_type` is the stored
        mode; rabitq_index.bin under the collection's path is installed when the mode names RaBitQ, the file is there, its dim is
        the collection's and it covers no more rows than are flushed.  False (and exact search) otherwise."""
        from .storage import load_rabitq_index

        mode = str(index_type).upper()
        if self._path is None or not flat_rabitq_mode(mode):
            return False
        f = self._path / RABITQ_INDEX_FILE
        if not f.exists():
            return False
        idx = load_rabitq_index(f)
        if idx.dim != self._dim or idx.n_vectors == 0 or idx.n_vectors > len(self._flat):
            return False
        self._flat.drop_pq()
        self._pq = False
        self._flat.load_rabitq(idx.sign_words, idx.codes, idx.norms)
        self._ivf = None
        self._rabitq = True
        self._index_mode, self._metric = mode, metric_from_index_mode(mode)
        return True

    def _save_polarvec(self) -> None:
        if self._path is None:
            return
        from .storage import PolarvecIndexFile, save_polarvec_index

        p = self._flat.polarvec_params()
        save_polarvec_index(self._path / POLARVEC_INDEX_FILE,
                            PolarvecIndexFile(p["dim"], p["padded_dim"], p["bits"], p["sign_words"], p["dim_mins"], p["dim_scales"], p["codes"],
                                              p["residual_sq"], p["inv_v_hat_norms"]))

    def try_load_polarvec(self, index_type: str) -> bool:
        """try_load_rabitq's rules for polarvec_index.bin: installed when the stored mode names PolarVec with the file's bit count, the
        file is there, its dim is the collection's and it covers no more rows than are flushed.  False (and exact search) otherwise."""
        from .storage import load_polarvec_index

        mode = str(index_type).upper()
        if self._path is None or flat_pq_mode(mode) or flat_rabitq_mode(mode):
            return False
        bits = flat_polarvec_mode(mode)
        f = self._path / POLARVEC_INDEX_FILE
        if not bits or not f.exists():
            return False
        idx = load_polarvec_index(f)
        if idx.dim != self._dim or idx.bits != bits or idx.n_vectors == 0 or idx.n_vectors > len(self._flat):
            return False
        self._flat.drop_pq()
        self._flat.drop_rabitq()
        self._pq = self._rabitq = False
        self._flat.load_polarvec(idx.bits, idx.sign_words, idx.dim_mins, idx.dim_scales, idx.codes, idx.residual_sq, idx.inv_v_hat_norms)
        self._ivf = None
        self._polarvec = bits
        self._index_mode, self._metric = mode, metric_from_index_mode(mode)
        return True

    def _build_hnsw(self) -> None:
        """The graph over every flushed row.  There is no on-disk form: a reopened collection builds it again.  Rows flushed after a
        build are linked in by _extend_hnsw; mutations go through _rebuild_index."""
        o = self._hnsw_opts
        self._flat.build_hnsw(self._metric, o["m"], o["ef_construction"], o["ef_search"], o["max_level"], HNSW_SEED)
        self._hnsw, self._hnsw_rows = True, len(self._flat)

    def _extend_hnsw(self) -> None:
        """Rows were flushed after the build: the graph is brought up to date in place (FlatIndex.extend_hnsw, equal to a build over
        every row); a handle that cannot extend its graph builds it again."""
        try:
            self._flat.extend_hnsw()
        except NotImplementedError:
            self._build_hnsw()
        self._hnsw_rows = len(self._flat)

    def _build_diskann(self) -> None:
        """The graph over every flushed row.  It has no on-disk form and, unlike the HNSW graph, no incremental insert: the batched
        Vamana build depends on its batch order, so rows flushed after a build build it again."""
        o = self._diskann_opts
        self._flat.build_diskann(self._metric, o["r"], o["l"], o["alpha"], o["max_degree"], DISKANN_SEED)
        self._diskann, self._diskann_rows = True, len(self._flat)

    def _build_ivf(self) -> None:
        n = len(self._flat)
        data = self._flat.read_rows(0, n)
        if "spann" in self._ivf_params:   # SPANNIndex: train_for_metric clamps the list count to the rows
            replicas, sq8 = self._ivf_params["spann"]
            self._ivf = SpannIndex.build(data, self._dim, self._ivf_params["n_clusters"], 20, int(self._metric), replicas, sq8,
                                         self._ivf_nprobe, device=self._device)
            self._ivf_rows = n
            return
        nlist = min(self._ivf_params["n_clusters"], max(n, 1))
        # the metric id goes through as it is: binary metrics build the IVF-*-BINARY mode, float metrics an IVFIndex
        # trained with its routing metric (ivf.rs:163-170)
        self._ivf = IvfFlatIndex.build(None, data, self._dim, nlist, 20, int(self._metric), device=self._device, l2_partitions=False,
                                       quantizer=self._ivf_params.get("quantizer"))
        self._ivf_rows = n

    def _use_sq8(self) -> bool:  # Collection::resolve_use_sq8 (engine.rs:4684-4689)
        return "SQ8" in self._index_mode.upper()

    # -- search -------------------------------------------------------------------------------
    def _subset_rows(self, subset) -> Optional[np.ndarray]:
        if subset is None:
            return None
        if isinstance(subset, BitSet):
            return subset.to_vec()
        return np.unique(np.asarray(subset, dtype=np.uint64).reshape(-1))

    # -- field filters (`where=`, lynsedb_amd/fields.py) ---------------------------
    def _resolve_where(self, where) -> ResolvedWhere:
        """The predicate over every row: the flushed rows by k_field_filter over the device copy of the columns it names (uploaded
        whole when they changed), the pending rows by the same compiled predicate on the host."""
        if isinstance(where, ResolvedWhere):
            return where
        import time

        t0 = time.perf_counter()
        pred = parse_where(where)
        n = len(self._flat)
        assert self._fields.n == n + self._pending_rows, "the field columns are not aligned with the rows"
        count = 0
        if n:
            if self._field_filter is None:
                self._field_filter = FieldFilter(self._device)
            count = self._field_filter.filter(self._fields, pred, n)
        pending = np.zeros(0, np.uint64)
        if self._pending_rows:
            pending = (np.nonzero(self._fields.evaluate(pred, n, n + self._pending_rows))[0] + n).astype(np.uint64)
        return ResolvedWhere(pred, n, count, pending, int((time.perf_counter() - t0) * 1e6))

    def _where_rows(self, rw: ResolvedWhere) -> np.ndarray:
        """The rows a resolved filter selects, ascending: the words of the flushed rows read back, then the pending rows.  What the
        searches that keep their host-side subset plumbing take as `subset=`."""
        if rw.rows is None:
            flushed = BitSet(rw.n_flat, self._field_filter.words()).to_vec() if rw.n_flat and rw.count else np.zeros(0, np.uint64)
            rw.rows = np.concatenate([flushed, rw.pending])
        return rw.rows

    def _where_subset(self, where, subset):
        """`subset` as it was given, or the rows `where` selects; both together are an error."""
        if where is None:
            return subset
        if subset is not None:
            raise ValueError("pass the filter either as where= or as subset=, not both")
        return self._where_rows(self._resolve_where(where))

    def where_subset(self, where) -> BitSet:
        """The rows a field filter selects, flushed and pending, as the BitSet every `subset=` accepts (the words of the flushed rows
        read back from the device).  What `where=` does inside the searches that keep their host-side subset plumbing, and the way a
        filter reaches `search_range`."""
        return BitSet.from_rows(self._where_rows(self._resolve_where(where)), len(self._flat) + self._pending_rows)

    def query_fields(self, where: str) -> list:
        """`Collection.query_fields` (FieldStore::query over query_from_index + filter_current_external_ids): the user ids of the rows
        the filter selects, flushed or pending, ascending, tombstoned ids excluded."""
        rows = self._where_rows(self._resolve_where(where)).astype(np.int64)
        if rows.size == 0:
            return []
        ids = self._user_ids(rows)
        if self._tombstone:
            ids = ids[~np.isin(ids, np.fromiter(self._tombstone, dtype=np.int64, count=len(self._tombstone)))]
        return [int(i) for i in np.unique(ids)]

    def _pending_search(self, query: np.ndarray, k: int, subset_rows: Optional[np.ndarray]):
        """Collection::pending_search (engine.rs:3310-3361): the un-flushed rows, scored with `top_k_search`."""
        if k == 0 or self._pending_rows == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.float32)
        data = np.concatenate(self._pending_vecs) if len(self._pending_vecs) > 1 else self._pending_vecs[0]
        row_offsets = np.arange(len(self._flat), len(self._flat) + data.shape[0], dtype=np.uint64)
        if subset_rows is not None:
            keep = np.isin(row_offsets, subset_rows)
            data, row_offsets = np.ascontiguousarray(data[keep]), row_offsets[keep]
        if row_offsets.size == 0:
            return np.zeros(0, np.uint64), np.zeros(0, np.float32)
        idx, dists = py_top_k_search(query, data, _METRIC_NAMES[self._metric], k)
        return row_offsets[idx.astype(np.int64)], dists

    def _user_ids(self, rows: np.ndarray) -> np.ndarray:
        """row_to_user_id (engine.rs:3071-3073) over flushed and pending rows."""
        rows = rows.astype(np.int64)
        n_flat = len(self._flat)
        if self._pending_rows == 0:
            return self._id_map()[rows]
        ids = np.concatenate([self._id_map()] + self._pending_ids)
        assert ids.size == n_flat + self._pending_rows
        return ids[rows]

    def _base_search(self, q: np.ndarray, search_k: int, nprobe: int, subset_rows: Optional[np.ndarray], where_dev: Optional[ResolvedWhere] = None,
                     approx_eps: Optional[float] = None):
        """The device part of search_with_precomputed_filter for a batch sharing one subset -> rows, dists, counts.  `where_dev`: the
        subset is the words the field filter left on the device (the exact filtered scan takes them without a round trip).
        `approx_eps` (from _approx_eps: one unfiltered query on a plain flat collection): the approximate flat search, raw distances."""
        nq = q.shape[0]
        if len(self._flat) == 0 or search_k == 0:
            return np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32)
        if self._index_dirty:
            self._rebuild_index()
        if self._ivf is not None:
            if self._ivf_rows != len(self._flat):
                # rows were committed after the build: Collection::flush hands them to idx.insert (engine.rs:3642-3645, :3858) —
                # assigned to the existing centroids, no retraining
                n_new = len(self._flat) - self._ivf_rows
                self._ivf.insert(self._flat.read_rows(self._ivf_rows, n_new))
                self._ivf_rows = len(self._flat)
            np_ = self._ivf_nprobe if not nprobe else int(nprobe)  # nprobe == 0 -> the build default (engine.rs:4743-4746)
            if subset_rows is not None:
                if subset_rows.size == 0:
                    return np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32)
                return self._ivf.search_filtered_batch_arrays(q, search_k, np_, subset_rows)
            return self._ivf.search_batch_arrays(q, search_k, np_)
        if where_dev is not None:   # the same exact filtered scan, its BitSet words already on the device
            if where_dev.count == 0:
                return np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32)
            d_words, n_words = self._field_filter.words_device()
            return self._flat.search_filtered_bitset_device_batch_arrays(q, search_k, self._metric, d_words, n_words, where_dev.count)
        if subset_rows is not None:  # brute_force_search_filtered (engine.rs:5541-5566): always the exact filtered scan
            if subset_rows.size == 0:
                return np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32)
            return self._flat.search_filtered_batch_arrays(q, search_k, self._metric, subset_rows)
        if self._hnsw:   # nprobe > 0 is the query-time ef (engine.rs:4743-4745); a subset took the exact filtered scan above
            if self._hnsw_rows != len(self._flat):   # rows were flushed after the build
                self._extend_hnsw()
            return self._flat.search_hnsw_batch_arrays(q, search_k, self._metric, int(nprobe))
        if self._diskann:   # nprobe > 0 is ef_query; the store rescore of the candidates is the identity: the beam scored the full-precision rows
            if self._diskann_rows != len(self._flat):   # rows were flushed after the build
                self._build_diskann()
            return self._flat.search_diskann_batch_arrays(q, search_k, self._metric, int(nprobe))
        if self._pq:   # search_auxiliary_quantized (engine.rs:5504-5526): rows committed after the build are not in the index
            return self._flat.search_pq_batch_arrays(q, search_k, self._metric, PQ_OVERSAMPLE)
        if self._rabitq:
            return self._flat.search_rabitq_batch_arrays(q, search_k, self._metric, RABITQ_OVERSAMPLE)
        if self._polarvec:
            return self._flat.search_polarvec_batch_arrays(q, search_k, self._metric, POLARVEC_OVERSAMPLE)
        if approx_eps is not None:   # before the SQ8 branch, as in FlatMmap::search
            rows, dists, self._approx_info = self._flat.search_approx(q[0], search_k, self._metric, approx_eps)
            return rows.reshape(1, -1), dists.reshape(1, -1), np.array([rows.size], np.uint32)
        if self._use_sq8() and self._metric in (_lib.METRIC_IP, _lib.METRIC_L2, _lib.METRIC_COSINE):
            return self._flat.search_sq8_batch_arrays(q, search_k, self._metric)
        return self._flat.search_batch_arrays(q, search_k, self._metric)

    def search(self, vector, k: Optional[int] = None, where_expr: Optional[str] = None,
               nprobe: Optional[int] = None, approx: Optional[bool] = None, eps: Optional[float] = None,
               subset=None, where=None) -> SearchResult:
        """`Collection.search` (src/python/mod.rs:1171-1193 over engine.rs:4718-4833).  `approx=True` takes the approximate flat search
        (FlatIndex.search_approx) where the reference does — a metric of APPROX_FLAT_METRICS, no IVF / SPANN / HNSW / DiskANN index, no PQ /
        RaBitQ / PolarVec index, no `subset=` / `where=` (FLAT-*-SQ8 does not stand in its way) — and is ignored everywhere else, as on an
        F16 collection (a gap).  Pending rows and tombstones merge on the raw scores; the distances that come back are rounded
        to multiples of eps (None, non-finite or <= 0: 1e-4; at least 1e-8), half away from zero."""
        res = self._batch_search(np.asarray(vector, dtype=np.float32).reshape(1, -1), k, where_expr, nprobe, subset=subset, where=where,
                                 approx=approx, eps=eps)
        return res[0]

    def _approx_eps(self, approx, eps, filtered: bool) -> Optional[float]:
        """The normalised eps when the approximate flat search answers this collection's searches (engine.rs:4757-4798), else None."""
        if (not approx or filtered or self._metric not in APPROX_FLAT_METRICS or self._flat.dtype == "f16" or self._ivf is not None
                or self._hnsw or self._diskann or self._pq or self._rabitq or self._polarvec):
            return None
        return normalize_eps(eps)

    def search_profile(self, vector, k: Optional[int] = None, where_expr: Optional[str] = None, nprobe: Optional[int] = None,
                       approx: Optional[bool] = None, eps: Optional[float] = None, subset=None, where=None) -> dict:
        """`Collection.search_profile` (src/python/mod.rs:1240-1271 over Collection::search_with_profile, src/engine.rs:5005-5054): the
        search + a `QueryProfile` (engine.rs:6906-6919) with the reference's field names — query_kind, vector_field, index_path
        ("ann_index" / "flat_mmap_filtered" / "flat_mmap", engine.rs:5163-5177), total_vectors, filter_expression, filter_matches,
        scanned_vectors (= filter_matches or total_vectors, as estimate_scanned_vectors does, :5179-5193), result_count, filter_us, search_us,
        rerank_us, total_us.  `device` is this build's addition: what `lynse_hip_flat_profile_get` / `lynse_hip_ivf_profile_get` measured for the
        search with HIP events on the search stream (pipeline_us, scan_us, scan_launches, rows and bytes the scan launches streamed,
        rescored_candidates, fallback_queries).  The precomputed filter is `subset=`; with `where=` filter_expression is the string,
        filter_matches the rows it selects (flushed and pending), filter_us the time of the filter (column upload, kernel, count read-back
        and the host pass over the pending rows), and index_path "flat_mmap_filtered" unless an IVF index answers."""
        import time

        started = time.perf_counter()
        filter_us, filter_matches = 0, None
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the resolved row filter as subset=")
        if where is not None and subset is not None:
            raise ValueError("pass the filter either as where= or as subset=, not both")
        if subset is not None:
            t0 = time.perf_counter()
            filter_matches = int(self._subset_rows(subset).size)
            filter_us = int((time.perf_counter() - t0) * 1e6)
        rw = None
        if where is not None:
            rw = self._resolve_where(where)
            filter_matches, filter_us = int(rw.count + rw.pending.size), rw.us
        unfiltered = subset is None and rw is None
        target = self._ivf if self._ivf is not None else self._flat
        sq8 = self._ivf is not None and self._ivf.is_sq8
        pq = self._ivf is None and self._pq and unfiltered
        rabitq = self._ivf is None and self._rabitq and unfiltered
        polarvec = self._ivf is None and bool(self._polarvec) and unfiltered
        hnsw = self._ivf is None and self._hnsw and unfiltered
        diskann = self._ivf is None and self._diskann and unfiltered
        target.profile_enable(True)
        target.profile_get(reset=True)
        if sq8:
            self._ivf.sq8_stage_times(reset=True)
        if pq:
            self._flat.pq_stage_times(reset=True)
        if rabitq:
            self._flat.rabitq_stage_times(reset=True)
        if polarvec:
            self._flat.polarvec_stage_times(reset=True)
        if hnsw:
            self._flat.hnsw_stage_times(reset=True)
        if diskann:
            self._flat.diskann_stage_times(reset=True)
        stage_us = plv_us = hnsw_us = diskann_us = None
        t0 = time.perf_counter()
        try:
            self._approx_info = None
            res = self.search(vector, k, None, nprobe, approx, eps, subset=subset, where=rw)
        finally:
            dev = target.profile_get(reset=True)
            # IVF-*-SQ8 / SPANN-*-SQ8: the exact rerank of the pool (HIP events on the search stream); 0 for the modes without one
            rerank_us = int(self._ivf.sq8_stage_times(reset=True)["rerank_us"]) if sq8 else 0
            if pq:   # FLAT-*-PQ: the exact rescore of the ADC pool
                rerank_us = int(self._flat.pq_stage_times(reset=True)["rescore_us"])
            if rabitq:   # FLAT-*-RABITQ: both stages of the two-pass search
                t = self._flat.rabitq_stage_times(reset=True)
                rerank_us, stage_us = int(t["rescore_us"]), {"scan_us": float(t["scan_us"]), "rescore_us": float(t["rescore_us"])}
            if polarvec:   # FLAT-*-POLARVEC<b>: likewise
                t = self._flat.polarvec_stage_times(reset=True)
                rerank_us, plv_us = int(t["rescore_us"]), {"scan_us": float(t["scan_us"]), "rescore_us": float(t["rescore_us"])}
            if hnsw:
                t = self._flat.hnsw_stage_times(reset=True)
                hnsw_us = {"search_us": float(t["search_us"]), "scored": int(t["scored"])}
            if diskann:
                t = self._flat.diskann_stage_times(reset=True)
                diskann_us = {"search_us": float(t["search_us"]), "scored": int(t["scored"])}
            target.profile_enable(False)
        search_us = int((time.perf_counter() - t0) * 1e6)
        total = int(self.shape()[0])
        profile = {"query_kind": "vector", "vector_field": "default",
                   "index_path": "ann_index" if self._ivf is not None or hnsw or diskann else ("flat_mmap_filtered" if not unfiltered else
                                                                            ("pq_two_pass" if pq else ("rabitq_two_pass" if rabitq else ("polarvec_two_pass" if polarvec else "flat_mmap")))),
                   "total_vectors": total, "filter_expression": None if rw is None else rw.pred.expr, "filter_matches": filter_matches,
                   "scanned_vectors": filter_matches if filter_matches is not None else total, "result_count": len(res),
                   "filter_us": filter_us, "search_us": search_us, "rerank_us": rerank_us, "total_us": int((time.perf_counter() - started) * 1e6),
                   "device": {"pipeline_us": float(dev["total_us"]), "scan_us": float(dev["scan_us"]), "scan_launches": int(dev["scan_launches"]),
                              "scan_rows": int(dev["scan_rows"]), "scan_bytes": int(dev["scan_bytes"]), "rescored_candidates": int(dev["pool_entries"]),
                              "fallback_queries": int(dev["fallback_queries"]), "plan": int(dev["last_plan"])}}
        if stage_us is not None:
            profile["device"]["rabitq_stages"] = stage_us
        if plv_us is not None:
            profile["device"]["polarvec_stages"] = plv_us
        if hnsw_us is not None:
            profile["device"]["hnsw"] = hnsw_us
        if diskann_us is not None:
            profile["device"]["diskann"] = diskann_us
        if self._approx_info is not None:   # the approximate flat search answered the flushed rows
            profile["device"]["approx"] = self._approx_info
        return {"items": {"k": res._k, "ids": [int(x) for x in res.ids()], "scores": [float(x) for x in res.distances()], "index": res.index_mode()},
                "profile": profile}

    def batch_search(self, vectors, k: Optional[int] = None, where_expr: Optional[str] = None,
                     nprobe: Optional[int] = None, subset=None, where=None) -> list:
        """Collection::batch_search (engine.rs:5352-5498): one shared filter, every query through
        `search_with_precomputed_filter`; the flushed rows of the whole batch are scanned in ONE pass on the GPU.  `where=` is the
        filter as a string of the indexed dialect (class docstring): the exact filtered scan takes its BitSet words on the device, an
        IVF / SPANN index takes them read back as the `subset=` it accepts.  `where_expr=` keeps its refusal (existing tests pin it)."""
        return self._batch_search(vectors, k, where_expr, nprobe, subset=subset, where=where)

    def _batch_search(self, vectors, k, where_expr, nprobe, subset=None, where=None, approx=None, eps=None) -> list:
        """batch_search; `approx` / `eps` are `search`'s (one query: the reference's batch_search has neither)."""
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the resolved "
                                      "row filter as subset=BitSet | row indices (search_with_precomputed_filter)")
        k = 10 if k is None else int(k)
        q = _f32(vectors, 2, "vectors")
        if q.shape[1] != self._dim:  # engine.rs:4707-4712 -> wrapped as RuntimeError (src/python/mod.rs:1190)
            raise RuntimeError(f"Dimension mismatch: expected {self._dim}, got {q.shape[1]}")
        from .shard_node import filter_tombstoned_limit, merge_row_results

        if where is not None and subset is not None:
            raise ValueError("pass the filter either as where= or as subset=, not both")
        subset_rows = self._subset_rows(subset)
        where_dev = None
        if where is not None:
            rw = self._resolve_where(where)
            if self._ivf is not None:
                subset_rows = self._where_rows(rw)
            else:
                where_dev, subset_rows = rw, rw.pending   # (the pending rows the filter selects: what _pending_search keeps)
        tomb = np.fromiter(self._tombstone, dtype=np.uint64, count=len(self._tombstone))
        search_k = k if tomb.size == 0 else k + int(tomb.size)   # engine.rs:4735-4747
        approx_eps = self._approx_eps(approx, eps, subset is not None or where is not None)
        rows, dists, counts = self._base_search(q, search_k, int(nprobe or 0), subset_rows, where_dev, approx_eps)
        out = []
        for i in range(q.shape[0]):
            c = int(counts[i])
            r_i, d_i = rows[i, :c].astype(np.uint64), dists[i, :c]
            if self._pending_rows:
                p_r, p_d = self._pending_search(q[i], search_k, subset_rows)
                r_i, d_i = merge_row_results(r_i, d_i, p_r, p_d, search_k, self._metric)   # engine.rs:4800-4813
            ids = self._user_ids(r_i).astype(np.uint64)
            ids, d_i = filter_tombstoned_limit(ids, d_i, tomb, k)                              # engine.rs:4819-4820
            if approx_eps is not None:                                                         # engine.rs:4821-4823: rounded last
                d_i = round_distances_to_eps(d_i, approx_eps)
            out.append(SearchResult(ids.astype(np.int64), np.asarray(d_i, np.float32), self._index_mode, self._dim, k))
        return out

    # -- named vector fields (engine.rs:4042-4420, :4836-4960; lynsedb_amd/vector_fields.py) ---------------------
    def remove_index(self) -> None:
        """Collection::remove_index (engine.rs:6106-6143): whatever index the collection holds goes, and with it the index mode —
        searches are the exact inner-product scan the reference falls back to without one."""
        self._flush_pending()
        self._ivf = None
        self._drop_aux()
        self._index_mode, self._metric = "FLAT-IP", _lib.METRIC_IP
        self._index_dirty = False

    def _vector_field(self, field_name: str) -> NamedVectorField:
        name = validate_vector_field_name(field_name)
        f = self._vfields.get(name)
        if f is None:
            raise RuntimeError(f"Invalid argument: vector field '{name}' does not exist")
        return f

    def create_vector_field(self, name: str, dimension: int, metric: Optional[str] = None, index_mode: Optional[str] = None,
                            dtypes: Optional[str] = None) -> dict:
        """`Collection.create_vector_field` (create_vector_field_with_dtype, engine.rs:4052-4121) -> the field's config.  A field takes
        the exact FLAT modes and HNSW-{IP,L2,COS,COSINE} (an HNSW mode is built by build_vector_field_index, as in the reference);
        every other mode the reference knows is NotImplementedError."""
        if int(dimension) == 0:
            raise RuntimeError("Invalid argument: vector field dimension must be greater than zero")
        name = validate_vector_field_name(name)
        m = resolve_named_vector_metric(metric, index_mode)
        mode = normalize_field_index_mode(index_mode, m)
        dtype = vector_dtype_name(dtypes, "float16" if self._flat.dtype == "f16" else "float32")
        field_mode_kind(mode)
        old = self._vfields.get(name)
        if old is not None:
            if (old.dimension, old.metric, old.index_mode, old.dtypes) == (int(dimension), m, mode, dtype):
                return old.config()
            raise RuntimeError(f"Invalid argument: vector field '{name}' already exists with a different configuration")
        f = self._vfields[name] = NamedVectorField(name, int(dimension), m, mode, dtype, self._device)
        return f.config()

    def list_vector_fields(self) -> list:
        """`Collection.list_vector_fields` (engine.rs:4125-4144): the primary vector as `default`, then the named fields by name."""
        out = [{"name": DEFAULT_VECTOR_FIELD_NAME, "dimension": self._dim, "metric": _METRIC_NAMES[self._metric], "index_mode": self._index_mode,
                "dtypes": "float16" if self._flat.dtype == "f16" else "float32"}]
        return out + [self._vfields[n].config() for n in sorted(self._vfields)]

    def vector_field_shape(self, field_name: str):
        if field_name == DEFAULT_VECTOR_FIELD_NAME or not str(field_name).strip():
            return self.shape()
        f = self._vector_field(field_name)
        return (len(f), f.dimension)

    def _rows_of_all_ids(self, ids: np.ndarray) -> np.ndarray:
        """The collection row of each id over flushed and pending rows (the pending rows are numbered after the flushed ones), -1 for
        an id without one: the sorted-id lookup of update_items (_rows_of_ids) over both.  This mirror's add_items accepts an id twice
        (the reference does not, engine.rs:3505-3512); where update_items refuses such an id, a search must still answer, so an id
        stored in more than one row resolves to its FIRST row (the stable sort keeps the rows of one id in order)."""
        all_ids = np.concatenate([self._id_map()] + self._pending_ids) if self._pending_rows else self._id_map()
        rows = np.full(ids.size, -1, np.int64)
        if all_ids.size == 0 or ids.size == 0:
            return rows
        order = np.argsort(all_ids, kind="stable")
        sorted_ids = all_ids[order]
        lo = np.minimum(np.searchsorted(sorted_ids, ids, "left"), all_ids.size - 1)
        hit = sorted_ids[lo] == ids
        rows[hit] = order[lo[hit]]
        return rows

    def add_named_vectors(self, field_name: str, vectors, ids: Sequence[int]) -> None:
        """`Collection.add_named_vectors` (engine.rs:4181-4248): attaches one vector of the field to ids that exist, flushed or
        pending.  The rows go straight to the field's shard (the reference has no pending buffer for named vectors); a failed call
        changes nothing."""
        f = self._vector_field(field_name)
        a = _f32(vectors, 2, "vectors")
        n_ids = len(ids)
        if a.shape[1] != f.dimension:
            raise RuntimeError(f"Dimension mismatch: expected {f.dimension}, got {a.shape[1]}")
        if n_ids != a.shape[0]:
            raise RuntimeError(f"Invalid argument: ids length ({n_ids}) must match n_vectors ({a.shape[0]})")
        id_arr = np.asarray([int(i) for i in ids], dtype=np.int64)
        seen, known = set(), self._ids_known(id_arr)
        for i, ok in zip(id_arr.tolist(), known.tolist()):
            if i in seen:
                raise RuntimeError(f"Invalid argument: duplicate id {i} within named vector batch")
            seen.add(i)
            if not ok:
                raise RuntimeError(f"Invalid argument: cannot add named vector for unknown id {i}")
            if i in f.reverse:
                raise RuntimeError(f"Invalid argument: id {i} already has a vector for field '{f.name}'")
        if id_arr.size:
            f.append(np.ascontiguousarray(a), id_arr)

    def _field_rowmap(self, f: NamedVectorField) -> RowMap:
        """The field's row_of on the device, rebuilt whole when the collection's rows or the field's rows changed since the last one."""
        stamp = (self._row_stamp, len(f))
        if f.rowmap is None:
            f.rowmap = RowMap(self._device)
        if f.rowmap_stamp != stamp:
            rows = self._rows_of_all_ids(f.id_map())
            row_of = np.where(rows < 0, ROWMAP_NONE, rows).astype(np.uint32)
            f.rowmap.set(row_of)
            f.rowmap_stamp = stamp
        return f.rowmap

    def _field_mask(self, f: NamedVectorField, where, subset):
        """The filter over collection rows as BitSet words over the field's rows, on the device -> (d_words, n_words, count).
        `where=`: k_field_filter over the flushed rows exactly as `search` resolves it, the pending rows evaluated on the host and
        uploaded as the tail; `subset=`: its words uploaded.  Then k_bitset_remap."""
        n_flat, n_pend = len(self._flat), self._pending_rows
        rm = self._field_rowmap(f)
        if where is not None:
            rw = self._resolve_where(where)
            tail = words_of_rows(rw.pending - np.uint64(n_flat), n_pend) if n_pend else None
            if n_flat:
                d_src, n_src_words = self._field_filter.words_device()
                return rm.remap(d_src, n_flat, tail, n_pend, src_count=rw.count, n_src_words=n_src_words)
            return rm.remap(np.zeros(0, np.uint64), 0, tail, n_pend)
        rows = self._subset_rows(subset)
        n = n_flat + n_pend
        return rm.remap(words_of_rows(rows[rows < np.uint64(n)], n), n)

    def batch_search_vector_field(self, field_name: str, vectors, k: Optional[int] = None, where=None, subset=None,
                                  nprobe: Optional[int] = None, where_expr: Optional[str] = None) -> list:
        return self._batch_search_vector_field(field_name, vectors, k, where, subset, nprobe, where_expr)

    def _batch_search_vector_field(self, field_name: str, vectors, k, where, subset, nprobe, where_expr, approx=None, eps=None) -> list:
        """`search_vector_field` (engine.rs:4836-4960) for a batch sharing one filter.  Without a filter and without tombstones the
        field's graph answers if it has one, else the exact scan of the field's shard.  With `where=` / `subset=` (collection rows) the
        mask is rewritten into field-row space on the device (k_bitset_remap) and the exact filtered scan of the field's shard takes the
        words without a round trip; for the additive metrics and a k beyond a quarter of the candidate capacity that entry reads the
        REMAPPED words back itself and takes its host-side path.  Tombstones: k grows by the tombstoned ids that carry a vector in this
        field, the host drops them and cuts to k (the reference ranks every row of the field instead).  Ties: (distance, field row)."""
        if field_name == DEFAULT_VECTOR_FIELD_NAME or not str(field_name).strip():
            return self._batch_search(vectors, k, where_expr, nprobe, subset=subset, where=where, approx=approx, eps=eps)
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the filter as where= or as "
                                      "subset=BitSet | row indices")
        f = self._vector_field(field_name)
        k = 10 if k is None else int(k)
        q = _f32(vectors, 2, "vectors")
        if q.shape[1] != f.dimension:
            raise RuntimeError(f"Dimension mismatch: expected {f.dimension}, got {q.shape[1]}")
        if where is not None and subset is not None:
            raise ValueError("pass the filter either as where= or as subset=, not both")
        from .shard_node import filter_tombstoned_limit

        nq = q.shape[0]
        tomb = np.array(sorted(i for i in self._tombstone if i in f.reverse), dtype=np.uint64)
        search_k = k + int(tomb.size)
        empty = (np.zeros((nq, 0), np.uint64), np.zeros((nq, 0), np.float32), np.zeros(nq, np.uint32))
        # the approximate flat search of the field's shard (engine.rs:4908-4924): no filter, the field's graph not in use, an f32 field
        approx_eps = None
        if (approx and where is None and subset is None and not (f.hnsw and not self._tombstone) and f.metric in APPROX_FLAT_METRICS
                and f.flat.dtype != "f16"):
            approx_eps = normalize_eps(eps)
        if len(f) == 0 or k == 0:
            rows, dists, counts = empty
        elif where is not None or subset is not None:
            d_words, n_words, count = self._field_mask(f, where, subset)
            if count == 0:
                rows, dists, counts = empty
            else:
                rows, dists, counts = f.flat.search_filtered_bitset_device_batch_arrays(q, search_k, f.metric, d_words, n_words, count)
        elif f.hnsw and not self._tombstone:   # use_field_index (engine.rs:4880): no filter and no tombstone
            if f.hnsw_rows != len(f.flat):     # vectors were added after the build
                f.extend_hnsw()
            rows, dists, counts = f.flat.search_hnsw_batch_arrays(q, search_k, f.metric, int(nprobe or 0))
        elif approx_eps is not None:
            r, d, _ = f.flat.search_approx(q[0], search_k, f.metric, approx_eps)
            rows, dists, counts = r.reshape(1, -1), d.reshape(1, -1), np.array([r.size], np.uint32)
        else:
            rows, dists, counts = f.flat.search_batch_arrays(q, search_k, f.metric)
        id_map = f.id_map()
        out = []
        for i in range(nq):
            c = int(counts[i])
            ids = id_map[rows[i, :c].astype(np.int64)].astype(np.uint64)
            ids, d_i = filter_tombstoned_limit(ids, dists[i, :c], tomb, k)
            if approx_eps is not None:
                d_i = round_distances_to_eps(d_i, approx_eps)
            out.append(SearchResult(ids.astype(np.int64), np.asarray(d_i, np.float32), f.index_mode, f.dimension, k))
        return out

    def search_vector_field(self, field_name: str, vector, k: Optional[int] = None, where=None, subset=None,
                            nprobe: Optional[int] = None, where_expr: Optional[str] = None, *, approx: Optional[bool] = None,
                            eps: Optional[float] = None) -> SearchResult:
        """`Collection.search_vector_field` (src/python/mod.rs:1199 over engine.rs:4836-4960); `default` or a blank name is `search`.
        `approx` / `eps`: as `search`, on the field's shard."""
        return self._batch_search_vector_field(field_name, np.asarray(vector, dtype=np.float32).reshape(1, -1), k, where, subset, nprobe,
                                               where_expr, approx, eps)[0]

    def build_vector_field_index(self, field_name: str, index_type: str, params: Optional[dict] = None) -> None:
        """`Collection.build_vector_field_index` (engine.rs:4303-4385).  A FLAT mode of a metric the exact scan serves changes the
        field's metric and mode and drops its graph; HNSW-{IP,L2,COS,COSINE} builds the graph over the field's rows (it is built again
        by the first search after vectors were added).  `default` or a blank name is `build_index`."""
        if field_name == DEFAULT_VECTOR_FIELD_NAME or not str(field_name).strip():
            return self.build_index(index_type, params)
        name = validate_vector_field_name(field_name)
        mode = str(index_type).strip().upper()
        if mode not in KNOWN_INDEX_MODES:
            raise RuntimeError(f"Invalid argument: unknown vector field index mode '{mode}'")
        kind = field_mode_kind(mode)
        metric = resolve_named_vector_metric(None, mode)
        opts = hnsw_build_options(params)   # (IndexBuildOptions::validate for every mode)
        f = self._vector_field(name)
        f.drop_hnsw()
        if kind == "hnsw":
            if len(f) == 0:
                raise ValueError("Empty database")
            f.build_hnsw(metric, opts)   # (a failed build leaves the field's metric, options and mode as they were, without a graph)
        f.metric, f.index_mode = metric, mode

    def remove_vector_field_index(self, field_name: str) -> None:
        """`Collection.remove_vector_field_index` (engine.rs:4388-4422): the field's graph goes, its mode is its metric's flat mode."""
        if field_name == DEFAULT_VECTOR_FIELD_NAME or not str(field_name).strip():
            return self.remove_index()
        f = self._vector_field(field_name)
        f.drop_hnsw()
        f.index_mode = normalize_field_index_mode(None, f.metric)

    def _compact_vector_fields(self, dead_ids: np.ndarray) -> None:
        """compact's part for the named fields (engine.rs:6543-...): the field rows of the dropped ids go, through the field handle's
        own compact; id_map follows and a field's graph is built again."""
        for f in self._vfields.values():
            keep = ~np.isin(f.id_map(), dead_ids)
            if keep.all():
                continue
            f.keep(keep)
            if f.hnsw:
                f.drop_hnsw()
                if len(f):
                    f.build_hnsw()
                else:
                    f.index_mode = normalize_field_index_mode(None, f.metric)

    # -- sparse vectors (engine.rs:4250-4279, :4962-5002) ---------------------------------------
    def _ids_known(self, ids: np.ndarray) -> np.ndarray:
        """is_id_exists for a batch: which of `ids` name a flushed or a pending row"""
        known = np.zeros(ids.size, bool)
        for a in list(self._id_arrays) + self._pending_ids:
            known |= np.isin(ids, a)
        return known

    def add_sparse_vectors(self, vectors, ids: Sequence[int]) -> None:
        """`Collection.add_sparse_vectors` (src/python/mod.rs:1115-1120 over engine.rs:4252-4279): attaches sparse vectors (dicts or
        lists of (index, value) pairs) to ids that exist, flushed or pending.  An id seen again is replaced, a vector that normalises
        to empty removes its id, a failed call leaves the store as it was.  With `path=` the store is rewritten to
        <path>/sparse_vectors.jsonl.  The device copy is refreshed by the next sparse search."""
        vecs = [normalize_sparse_vector(v) for v in vectors]
        ids = [int(i) for i in ids]
        if len(ids) != len(vecs):
            raise RuntimeError(f"Invalid argument: ids length ({len(ids)}) must match sparse vector count ({len(vecs)})")
        seen, known = set(), self._ids_known(np.asarray(ids, dtype=np.int64))
        for i, ok in zip(ids, known):
            if i in seen:
                raise RuntimeError(f"Invalid argument: duplicate id {i} within sparse vector batch")
            seen.add(i)
            if not ok:
                raise RuntimeError(f"Invalid argument: cannot add sparse vector for unknown id {i}")
        try:
            ptr, idx, val = sparse_normalize_arrays(*_sparse_csr(vecs))
        except ValueError as e:
            raise RuntimeError(f"Invalid argument: {e}") from None
        nxt = dict(self._sparse)
        for r, i in enumerate(ids):
            a, b = int(ptr[r]), int(ptr[r + 1])
            if a == b:
                nxt.pop(i, None)
            else:
                nxt[i] = (idx[a:b].copy(), val[a:b].copy())
        if self._path is not None:
            from .storage import save_sparse_vectors

            save_sparse_vectors(self._path / SPARSE_VECTORS_FILE, nxt)
        self._sparse, self._sparse_dirty = nxt, True

    def try_load_sparse(self) -> bool:
        """SparseVectorStore::load for a reopened collection: <path>/sparse_vectors.jsonl replaces the store.  False without a path
        or a file."""
        from .storage import load_sparse_vectors

        if self._path is None or not (self._path / SPARSE_VECTORS_FILE).exists():
            return False
        self._sparse, self._sparse_dirty = load_sparse_vectors(self._path / SPARSE_VECTORS_FILE), True
        return True

    def sparse_len(self) -> int:
        return len(self._sparse)

    def _sparse_upload(self) -> None:
        """the CSR of the store in ascending id order, so that (score, row ascending) is the reference's (score, id ascending)"""
        if self._sparse_index is None:
            self._sparse_index = SparseIndex(self._device)
        if not self._sparse_dirty:
            return
        ids = np.array(sorted(self._sparse), dtype=np.int64)
        lens = np.fromiter((self._sparse[int(i)][0].size for i in ids), dtype=np.uint64, count=ids.size)
        indptr = np.zeros(ids.size + 1, np.uint64)
        np.cumsum(lens, out=indptr[1:])
        indices = np.concatenate([self._sparse[int(i)][0] for i in ids]) if ids.size else np.zeros(0, np.uint32)
        values = np.concatenate([self._sparse[int(i)][1] for i in ids]) if ids.size else np.zeros(0, np.float32)
        self._sparse_index.set_rows(indptr, indices, values)
        self._sparse_ids, self._sparse_dirty = ids, False

    def _sparse_words(self, subset) -> Optional[np.ndarray]:
        """the BitSet words over sparse rows of a dense-row subset minus the tombstoned ids; None = every row"""
        n = int(self._sparse_ids.size)
        words = None
        if subset is not None:
            rows = self._subset_rows(subset).astype(np.int64)
            rows = rows[rows < len(self._flat) + self._pending_rows]
            allowed = self._user_ids(rows)
            words = BitSet.from_rows(np.nonzero(np.isin(self._sparse_ids, allowed))[0], n).words
        if self._tombstone:
            dead = np.nonzero(np.isin(self._sparse_ids, np.fromiter(self._tombstone, dtype=np.int64, count=len(self._tombstone))))[0]
            if dead.size:
                if words is None:
                    words = BitSet.from_rows(np.arange(n, dtype=np.uint64), n).words
                words = words & ~BitSet.from_rows(dead, n).words
        return words

    def batch_search_sparse(self, vectors, k: Optional[int] = None, subset=None, where=None) -> list:
        """`search_sparse` for a batch of query vectors sharing one subset, in ONE device call (this build's addition).  `where=`: the
        rows the field filter selects, read back and used as the subset."""
        subset = self._where_subset(where, subset)
        k = 10 if k is None else int(k)
        if k < 0:
            raise OverflowError("can't convert negative int to unsigned")
        vecs = [normalize_sparse_vector(v) for v in vectors]
        try:
            ptr, idx, val = sparse_normalize_arrays(*_sparse_csr(vecs))
        except ValueError as e:
            raise RuntimeError(f"Invalid argument: {e}") from None
        empty = lambda: SearchResult(np.zeros(0, np.int64), np.zeros(0, np.float32), SPARSE_INDEX_MODE, 0, k)   # noqa: E731
        if k == 0 or idx.size == 0 or not self._sparse:   # (engine.rs:4971-4980): the device is not touched
            return [empty() for _ in vecs]
        self._sparse_upload()
        rows, scores, counts, _ = self._sparse_index.search_batch_arrays(ptr, idx, val, k, self._sparse_words(subset))
        out = []
        for i in range(len(vecs)):
            c = int(counts[i])
            out.append(SearchResult(self._sparse_ids[rows[i, :c].astype(np.int64)], scores[i, :c].copy(), SPARSE_INDEX_MODE, 0, k))
        return out

    def search_sparse(self, vector, k: Optional[int] = None, where_expr: Optional[str] = None, subset=None, where=None) -> SearchResult:
        """`Collection.search_sparse` (src/python/mod.rs:1221-1237 over engine.rs:4964-5002): the ids whose sparse vector has a
        non-zero inner product with `vector`, by (score descending, id ascending), at most k (default 10); the scores are in
        `distances()`, the mode is SPARSE-FLAT-IP, the dimension 0.  Tombstoned ids are left out before the cut.  `subset=` (a BitSet
        or dense row indices) stands in for the resolved `where_expr`, as on `search`."""
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the resolved row filter as subset=")
        return self.batch_search_sparse([vector], k, subset=subset, where=where)[0]

    # -- text search (engine.rs:5056-5161, :927-1054) -------------------------------------------
    def text_len(self) -> int:
        return len(self._docs)

    def _text_upload(self, text_fields) -> None:
        """The postings of the documents under one field selection (TextFieldSelection, engine.rs:6967-6989: None or [] = all fields),
        rows in ascending id order so that (score, row ascending) is the reference's (score, id ascending); rebuilt when the
        selection or the documents changed."""
        key = tuple(sorted({str(f) for f in text_fields})) if text_fields else ()
        if self._text_index is None:
            self._text_index = TextIndex(self._device)
        if not self._text_dirty and key == self._text_key:
            return
        ids, lens, triples, vocab = [], [], [], {}
        for i in sorted(self._docs):
            tf: dict = {}
            for name, counts in self._docs[i].items():
                if not key or name in key:
                    for t, c in counts.items():
                        tf[t] = tf.get(t, 0) + c
            if not tf:   # selected length 0: the document does not exist for this selection
                continue
            row = len(ids)
            ids.append(i)
            lens.append(sum(tf.values()))
            for t, c in tf.items():
                triples.append((vocab.setdefault(t, len(vocab)), row, c))
        tr = np.array(triples, dtype=np.int64).reshape(-1, 3)
        tr = tr[np.lexsort((tr[:, 1], tr[:, 0]))]
        term_ptr = np.zeros(len(vocab) + 1, np.uint64)
        np.cumsum(np.bincount(tr[:, 0], minlength=len(vocab)), out=term_ptr[1:])
        self._text_index.set(np.array(lens, np.uint32), term_ptr, tr[:, 1].astype(np.uint32), tr[:, 2].astype(np.uint32))
        self._text_ids, self._text_vocab, self._text_key, self._text_dirty = np.array(ids, np.int64), vocab, key, False

    def _text_words(self, subset) -> Optional[np.ndarray]:
        """the BitSet words over text rows of a dense-row subset minus the tombstoned ids; None = every row"""
        n = int(self._text_ids.size)
        words = None
        if subset is not None:
            rows = self._subset_rows(subset).astype(np.int64)
            rows = rows[rows < len(self._flat) + self._pending_rows]
            allowed = self._user_ids(rows)
            words = BitSet.from_rows(np.nonzero(np.isin(self._text_ids, allowed))[0], n).words
        if self._tombstone:
            dead = np.nonzero(np.isin(self._text_ids, np.fromiter(self._tombstone, dtype=np.int64, count=len(self._tombstone))))[0]
            if dead.size:
                if words is None:
                    words = BitSet.from_rows(np.arange(n, dtype=np.uint64), n).words
                words = words & ~BitSet.from_rows(dead, n).words
        return words

    def batch_text_search(self, texts, text_fields=None, k: Optional[int] = None, subset=None, where=None) -> list:
        """`text_search` for a batch of query texts sharing one field selection and one subset, in ONE device call (this build's
        addition).  `where=`: the rows the field filter selects, read back and used as the subset."""
        subset = self._where_subset(where, subset)
        k = 10 if k is None else int(k)
        if k < 0:
            raise OverflowError("can't convert negative int to unsigned")
        texts = [str(t) for t in texts]
        if not self._docs:   # no document holds text: the reference's scan fallback over nothing
            return [SearchResult(np.zeros(0, np.int64), np.zeros(0, np.float32), TEXT_SCAN_MODE, self._dim, k) for _ in texts]
        empty = lambda: SearchResult(np.zeros(0, np.int64), np.zeros(0, np.float32), TEXT_INDEX_MODE, self._dim, k)   # noqa: E731
        if k == 0 or not texts:
            return [empty() for _ in texts]
        self._text_upload(text_fields)
        q_ptr, q_terms, q_counts = [0], [], []
        for text in texts:   # the distinct known terms in the order of their first occurrence, with their counts
            counts: dict = {}
            for t in tokenize_text(text):
                tid = self._text_vocab.get(t)
                if tid is not None:   # a term the store has never seen has df = 0: no effect
                    counts[tid] = counts.get(tid, 0) + 1
            q_terms.extend(counts.keys())
            q_counts.extend(counts.values())
            q_ptr.append(len(q_terms))
        if not q_terms or self._text_ids.size == 0:
            return [empty() for _ in texts]
        rows, scores, counts_, _ = self._text_index.search_batch_arrays(q_ptr, q_terms, q_counts, k, self._text_words(subset))
        out = []
        for i in range(len(texts)):
            c = int(counts_[i])
            out.append(SearchResult(self._text_ids[rows[i, :c].astype(np.int64)], scores[i, :c].copy(), TEXT_INDEX_MODE, self._dim, k))
        return out

    def text_search(self, text: str, text_fields=None, k: Optional[int] = 10, where_expr: Optional[str] = None, subset=None,
                    where=None) -> SearchResult:
        """`Collection.bm25_search` / `text_search` (src/python/mod.rs:1273-1300 over engine.rs:5060-5076 and InvertedTextIndex::search,
        :927-1054): BM25 over the `fields` given to add_items, by (score descending, id ascending), at most k; the scores are in
        `distances()`, the mode is BM25-INVERTED (BM25-SCAN and empty while no document holds text), the dimension the collection's.
        Tombstoned ids leave the corpus statistics too.  `subset=` (a BitSet or dense row indices) stands in for the resolved
        `where_expr`, as on `search`.  The sums run in the order of the terms' first occurrence in `text` (include/lynse_hip.h, TEXT
        SEARCH rule 3f)."""
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the resolved row filter as subset=")
        return self.batch_text_search([text], text_fields, k, subset=subset, where=where)[0]

    def hybrid_search(self, vector=None, text: Optional[str] = None, k: Optional[int] = 10, where_expr: Optional[str] = None, text_fields=None,
                      fusion: str = "rrf", vector_weight: float = 1.0, text_weight: float = 1.0, rrf_k: float = 60.0,
                      candidate_limit: Optional[int] = None, nprobe: int = 10, subset=None, where=None) -> SearchResult:
        """`Collection.hybrid_search` (src/python/mod.rs:1302-1340 over engine.rs:5079-5161): the vector search and the text search,
        each with k = candidate_limit (default max(4k, k), at least k and 1), fused by reciprocal rank ("rrf") or by normalised
        weighted scores ("weighted") — `hybrid_fuse`.  A blank text with a vector is the vector leg alone.  The mode is HYBRID-RRF or
        HYBRID-WEIGHTED."""
        if where_expr:
            raise NotImplementedError("`where_expr` needs the field store (out of scope, SURVEY.md §2); pass the resolved row filter as subset=")
        k = 10 if k is None else int(k)
        if k < 0:
            raise OverflowError("can't convert negative int to unsigned")
        has_text = text is not None and bool(str(text).strip())
        if vector is None and not has_text:
            raise RuntimeError("Invalid argument: hybrid_search requires a vector, text, or both")
        limit = max(int(candidate_limit) if candidate_limit else max(4 * k, k), k, 1)
        v_leg = t_leg = None
        if where is not None:   # one filter for both legs: its rows are read back before either runs
            if subset is not None:
                raise ValueError("pass the filter either as where= or as subset=, not both")
            where = self._resolve_where(where)
            subset, t_subset = None, self._where_rows(where)
        else:
            t_subset = subset
        if vector is not None:
            r = self.search(vector, limit, None, nprobe, subset=subset, where=where)
            v_leg = (r.ids(), r.distances())
        if has_text:
            r = self.text_search(str(text), text_fields, limit, subset=t_subset)
            t_leg = (r.ids(), r.distances())
        ascending = bool(lib.lynse_hip_metric_is_ascending(self._metric))
        ids, fused = hybrid_fuse(v_leg, t_leg, k, fusion, vector_weight, text_weight, rrf_k, ascending)
        mode = "HYBRID-WEIGHTED" if str(fusion).lower() == "weighted" else "HYBRID-RRF"
        return SearchResult(ids, fused, mode, self._dim, k)

    def search_range(self, vector, threshold: float, max_results: int = 1000, subset=None):
        """`Collection.search_range` (src/python/mod.rs:1784-1795 over Collection::search_range, src/engine.rs:6410-6483): the exact scan
        of every flushed, non-deleted row with the collection's metric, whatever index is built; the rows with distance <= threshold
        (ip: score >= threshold), at most `max_results` of them, best first -> (ids, distances) as a list of ints and a list of floats.
        Rows still in the pending buffer are not searched (the reference reads the vector store only).  Ties at the cut and in the
        order go by ascending row.  `subset=` (a BitSet or row indices) is this build's addition, as on `search`.  This method's
        parameter list is pinned (tests/test_range_search_modes.py), so it has no `where=` keyword of its own: a field filter goes in
        as `subset=collection.where_subset("...")`."""
        max_results = int(max_results)
        if max_results == 0:   # engine.rs:6416-6418, before the dimension check
            return [], []
        if max_results < 0:
            raise OverflowError("can't convert negative int to unsigned")
        q = np.ascontiguousarray(np.asarray(vector, dtype=np.float32).reshape(-1))
        if q.size != self._dim:   # engine.rs:6421-6426 -> wrapped as RuntimeError, as on search
            raise RuntimeError(f"Dimension mismatch: expected {self._dim}, got {q.size}")
        n = len(self._flat)
        if n == 0:
            return [], []
        words = None
        if subset is not None:
            words = BitSet.from_rows(self._subset_rows(subset), n).words
        if self._tombstone:   # tombstoned rows leave before the cap (:6439-6441): they are cleared from the row mask
            ids = self._id_map()[:n]
            dead = np.nonzero(np.isin(ids, np.fromiter(self._tombstone, dtype=np.int64, count=len(self._tombstone))))[0].astype(np.uint64)
            if dead.size:
                if words is None:
                    words = BitSet.from_rows(np.arange(n, dtype=np.uint64), n).words
                words = words & ~BitSet.from_rows(dead, n).words
        rows, dists, counts, _ = self._flat.search_range_batch_arrays(q.reshape(1, -1), [threshold], max_results, self._metric, words)
        c = int(counts[0])
        return [int(x) for x in self._id_map()[rows[0, :c].astype(np.int64)]], [float(x) for x in dists[0, :c]]


_METRIC_NAMES = {_lib.METRIC_IP: "ip", _lib.METRIC_L2: "l2", _lib.METRIC_COSINE: "cosine", _lib.METRIC_HAMMING: "hamming",
                 _lib.METRIC_JACCARD: "jaccard", _lib.METRIC_DICE: "dice", _lib.METRIC_TANIMOTO: "tanimoto",
                 _lib.METRIC_L1: "l1", _lib.METRIC_CHEBYSHEV: "chebyshev", _lib.METRIC_CANBERRA: "canberra",
                 _lib.METRIC_BRAY_CURTIS: "bray_curtis"}


class DatabaseManager:
    """src/python/mod.rs:2235-2418 — in-memory registry (persistence is out of scope)."""

    def __init__(self, root: str):
        self.root = root
        self._dbs: dict = {}

    def create_database(self, name: str) -> None:
        self._dbs.setdefault(name, {})

    def require_collection(self, db: str, coll: str, dim: int) -> None:
        self._dbs.setdefault(db, {})
        if coll not in self._dbs[db]:
            self._dbs[db][coll] = Collection(coll, dim)

    def get_collection(self, db: str, coll: str, dim: int) -> Collection:
        self.require_collection(db, coll, dim)
        c = self._dbs[db][coll]
        if c._dim != dim:
            raise RuntimeError(f"Dimension mismatch: expected {c._dim}, got {dim}")
        return c
