"""Named vector fields: a second, third, ... vector per record, each with its own dimension, metric and dtype.

The reference keeps a `NamedVectorField` per name — a vector store of its own, `id_map` (field row -> user id) and an optional index —
and searches it with the collection's `where` filter and tombstones (src/engine.rs:4042-4420, :4836-4960).  This module holds

    validate_vector_field_name / resolve_named_vector_metric / normalize_field_index_mode / vector_dtype_name
                        the reference's resolvers (engine.rs:2017-2091, src/storage/dtype.rs:12-21) with its messages; they need no device
    RowMap              `lynse_hip_rowmap`: row_of (field row -> collection row) in HBM and k_bitset_remap, which rewrites the BitSet
                        words of a filter over collection rows into words over field rows on the device
    NamedVectorField    one field: its FlatIndex shard, id_map and the reverse map, its config, its graph options, its lazily rebuilt
                        row_of

`Collection` (core.py) carries the surface: create_vector_field, list_vector_fields, vector_field_shape, add_named_vectors,
search_vector_field, batch_search_vector_field, build_vector_field_index, remove_vector_field_index.  include/lynse_hip.h NAMED VECTOR
FIELDS states the device half of the contract.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import check, lib

DEFAULT_VECTOR_FIELD_NAME = "default"
ROWMAP_NONE = 0xFFFFFFFF

_METRIC_NAME = {_lib.METRIC_IP: "ip", _lib.METRIC_L2: "l2", _lib.METRIC_COSINE: "cosine", _lib.METRIC_HAMMING: "hamming",
                _lib.METRIC_JACCARD: "jaccard", _lib.METRIC_DICE: "dice", _lib.METRIC_TANIMOTO: "tanimoto", _lib.METRIC_L1: "l1",
                _lib.METRIC_CHEBYSHEV: "chebyshev", _lib.METRIC_CANBERRA: "canberra", _lib.METRIC_BRAY_CURTIS: "bray_curtis"}
# DistanceMetric::flat_index_mode (src/distance/mod.rs:139-158)
_FLAT_MODE = {_lib.METRIC_IP: "FLAT-IP", _lib.METRIC_L2: "FLAT-L2", _lib.METRIC_COSINE: "FLAT-COS", _lib.METRIC_HAMMING: "FLAT-HAMMING-BINARY",
              _lib.METRIC_JACCARD: "FLAT-JACCARD-BINARY", _lib.METRIC_DICE: "FLAT-DICE-BINARY", _lib.METRIC_TANIMOTO: "FLAT-TANIMOTO-BINARY",
              _lib.METRIC_L1: "FLAT-L1", _lib.METRIC_CHEBYSHEV: "FLAT-CHEBYSHEV", _lib.METRIC_CANBERRA: "FLAT-CANBERRA",
              _lib.METRIC_BRAY_CURTIS: "FLAT-BRAY-CURTIS"}

_DENSE = ("IP", "L2", "COS", "COSINE")
_BINARY_SUFFIXES = ("HAMMING", "JACCARD", "TANIMOTO", "DICE", "SORENSEN", "SORENSEN-DICE")
_DOMAIN_SUFFIXES = ("L1", "MANHATTAN", "CITYBLOCK", "HAVERSINE", "HAVERSINE-M", "GEO", "CORRELATION", "PEARSON", "HELLINGER", "WASSERSTEIN",
                    "WASSERSTEIN-1D", "WASSERSTEIN1D", "EMD", "JENSEN-SHANNON", "JENSENSHANNON", "JS", "CHEBYSHEV", "CHEBYCHEV", "LINF",
                    "CANBERRA", "BRAY-CURTIS", "BRAYCURTIS")


def _known_index_modes() -> frozenset:
    """Every alias index::resolve_index_type answers (src/index/mod.rs:227-496), upper case."""
    m = set()
    for fam in ("FLAT", "HNSW", "IVF", "SPANN", "DISKANN"):
        for d in _DENSE:
            m.update((f"{fam}-{d}", f"{fam}-{d}-SQ8"))
    for fam in ("FLAT", "IVF"):
        for b in ("JACCARD", "HAMMING"):
            m.update((f"{fam}-{b}", f"{fam}-{b}-BINARY"))
    m.update(f"DISKANN-{d}-PQ{s}" for d in ("IP", "L2") for s in ("", "8", "16"))
    m.update(("DISKANN-COS-PQ", "DISKANN-COSINE-PQ"))
    for b in _BINARY_SUFFIXES:
        m.update((f"FLAT-{b}", f"FLAT-{b}-BINARY"))
    for s in _DOMAIN_SUFFIXES:
        m.add(f"FLAT-{s}")
        if s not in ("CANBERRA", "BRAY-CURTIS", "BRAYCURTIS"):
            m.add(f"HNSW-{s}")
    return frozenset(m)


KNOWN_INDEX_MODES = _known_index_modes()


def _invalid(msg: str) -> RuntimeError:
    return RuntimeError(f"Invalid argument: {msg}")


def validate_vector_field_name(name: str) -> str:
    """validate_vector_field_name (engine.rs:2017-2043) -> the trimmed name."""
    trimmed = str(name).strip()
    if not trimmed:
        raise _invalid("vector field name cannot be empty")
    if trimmed == DEFAULT_VECTOR_FIELD_NAME:
        raise _invalid("'default' is reserved for the primary collection vector")
    if len(trimmed.encode("utf-8")) > 128:   # (str::len counts bytes)
        raise _invalid("vector field name cannot exceed 128 characters")
    if not all(c.isascii() and (c.isalnum() or c in "_-") for c in trimmed):
        raise _invalid("vector field name may only contain ASCII letters, digits, '_' and '-'")
    return trimmed


def _metric_of_str(metric: str) -> int:
    from .core import metric_from_str

    try:
        return metric_from_str(metric)   # (NotImplementedError, not a ValueError, for a metric of the reference this library does not build)
    except ValueError:
        raise _invalid(f"unsupported vector field metric '{metric}'") from None


def _metric_of_mode(mode: str) -> int:
    """metric_from_mode_str (engine.rs:4679-4681): the metric token of the mode, inner product without one."""
    from .core import metric_from_index_mode

    try:
        return metric_from_index_mode(mode)
    except ValueError:
        return _lib.METRIC_IP


def resolve_named_vector_metric(metric: Optional[str], index_mode: Optional[str]) -> int:
    """resolve_named_vector_metric (engine.rs:2063-2091) -> the metric id: with an index mode the mode's metric (a `metric` that
    disagrees is an error), with only a metric that metric, with neither inner product."""
    if index_mode is not None:
        index_metric = _metric_of_mode(index_mode)
        if metric is not None and _metric_of_str(metric) != index_metric:
            raise _invalid(f"vector field metric '{metric}' does not match index mode '{index_mode}'")
        return index_metric
    if metric is not None:
        return _metric_of_str(metric)
    return _lib.METRIC_IP


def normalize_field_index_mode(index_mode: Optional[str], metric: int) -> str:
    """normalize_field_index_mode (engine.rs:2045-2061): trimmed and upper-cased; the metric's flat mode by default; a mode
    index::resolve_index_type does not know is refused."""
    mode = (index_mode or "").strip().upper() or _FLAT_MODE[metric]
    if mode not in KNOWN_INDEX_MODES:
        raise _invalid(f"unknown vector field index mode '{mode}'")
    return mode


def vector_dtype_name(dtypes: Optional[str], default: str = "float32") -> str:
    """VectorDtype::parse + storage_name (src/storage/dtype.rs:12-37): "float32" | "float16"."""
    if dtypes is None:
        return default
    d = str(dtypes).strip().lower()
    if d in ("f32", "float32", "float"):
        return "float32"
    if d in ("f16", "float16", "half", "fp16"):
        return "float16"
    raise _invalid(f"unsupported vector dtype '{dtypes}'; expected float32/f32 or float16/f16")


def metric_name(metric: int) -> str:
    return _METRIC_NAME[metric]


def field_mode_kind(mode: str) -> str:
    """What a (known, upper-case) index mode means for a named field here: "flat" = no index object, the exact scan of the mode's
    metric (ip / l2 / cosine, the four binary and the four additive metrics); "hnsw" = HNSW-{IP,L2,COS,COSINE}; every other mode the
    reference knows is NotImplementedError (out of scope)."""
    from .core import ADDITIVE_FLAT_MODES, HNSW_MODES

    if mode in HNSW_MODES:
        return "hnsw"
    if mode in ADDITIVE_FLAT_MODES:
        return "flat"
    parts = mode.split("-")
    if parts[0] == "FLAT" and "SQ8" not in parts:
        _metric_of_mode(mode)   # (NotImplementedError for the domain metrics this library does not build)
        return "flat"
    raise NotImplementedError(f"index mode '{mode}' on a named vector field is out of scope (DESIGN.md §26: a field takes the exact FLAT "
                              "modes and HNSW-{IP,L2,COS,COSINE})")


def words_of_rows(rows: np.ndarray, n: int) -> np.ndarray:
    """BitSet words over n rows with the bits of `rows` (each < n) set"""
    w = np.zeros((n + 63) // 64, np.uint64)
    r = np.asarray(rows, dtype=np.uint64).reshape(-1)
    if r.size:
        np.bitwise_or.at(w, (r >> np.uint64(6)).astype(np.int64), np.uint64(1) << (r & np.uint64(63)))
    return w


class RowMap:
    """`lynse_hip_rowmap`: row_of in HBM and k_bitset_remap.  `remap` returns (device pointer, n_words, count) of the words over field
    rows; when row_of is the identity over n_out == n_src rows, the source words are on the device and there is no tail, they ARE the
    answer and are handed on without a launch (`force_kernel` runs the kernel all the same)."""

    def __init__(self, device: Optional[int] = None):
        from .core import default_device

        self._h = C.c_void_p()
        self.n_out = 0
        self.identity = False
        self.last_kernel_us = 0.0
        self.last_shortcut = False
        self._destroy = lib.lynse_hip_rowmap_destroy   # bound now: module globals may be gone when __del__ runs at interpreter shutdown
        check(lib.lynse_hip_rowmap_create(default_device() if device is None else int(device), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._destroy(self._h)
            self._h = None

    def hbm_bytes(self) -> int:
        return int(lib.lynse_hip_rowmap_hbm_bytes(self._h))

    def set(self, row_of) -> None:
        """Uploads the whole map: u32[n_out], ROWMAP_NONE = the field row belongs to no collection row."""
        r = np.ascontiguousarray(np.asarray(row_of).reshape(-1), dtype=np.uint32)
        self.n_out, self.identity = 0, False
        check(lib.lynse_hip_rowmap_set(self._h, r.ctypes.data_as(C.c_void_p) if r.size else None, r.size))
        self.n_out = int(r.size)
        self.identity = bool(np.array_equal(r, np.arange(r.size, dtype=np.uint32)))

    def remap(self, src_words, n_src: int, tail_words=None, n_tail: int = 0, src_count: Optional[int] = None, n_src_words: Optional[int] = None,
              force_kernel: bool = False):
        """`src_words`: a device pointer (ctypes.c_void_p, with `n_src_words` and, for the identity shortcut, `src_count`) or a host
        u64 array covering n_src bits; `tail_words`: a host u64 array covering n_tail bits.  -> (d_words, n_words, count)."""
        on_device = isinstance(src_words, C.c_void_p)
        tail = np.zeros(0, np.uint64) if tail_words is None else np.ascontiguousarray(np.asarray(tail_words).reshape(-1), dtype=np.uint64)
        if on_device:
            src_ptr, nsw = src_words, int(n_src_words)
        else:
            src = np.ascontiguousarray(np.asarray(src_words).reshape(-1), dtype=np.uint64)
            src_ptr, nsw = (src.ctypes.data_as(C.c_void_p) if src.size else None), int(src.size)
        self.last_shortcut = False
        if (on_device and not force_kernel and self.identity and self.n_out == int(n_src) and int(n_tail) == 0 and src_count is not None
                and nsw == (int(n_src) + 63) // 64):
            self.last_shortcut, self.last_kernel_us = True, 0.0
            return (src_ptr if nsw else C.c_void_p()), nsw, int(src_count)
        count, us = C.c_uint64(0), C.c_float(0.0)
        check(lib.lynse_hip_rowmap_remap(self._h, src_ptr, nsw, int(n_src), 1 if on_device else 0,
                                         tail.ctypes.data_as(C.c_void_p) if tail.size else None, tail.size, int(n_tail), C.byref(count), C.byref(us)))
        self.last_kernel_us = float(us.value)
        ptr, nw = C.c_void_p(), C.c_uint64(0)
        check(lib.lynse_hip_rowmap_words_device(self._h, C.byref(ptr), C.byref(nw)))
        return ptr, int(nw.value), int(count.value)

    def words(self) -> np.ndarray:
        """The words of the last remap the kernel ran, read back."""
        ptr, nw = C.c_void_p(), C.c_uint64(0)
        check(lib.lynse_hip_rowmap_words_device(self._h, C.byref(ptr), C.byref(nw)))
        out = np.zeros(int(nw.value), np.uint64)
        check(lib.lynse_hip_rowmap_words(self._h, out.ctypes.data_as(C.c_void_p) if out.size else None, out.size))
        return out


class NamedVectorField:
    """One named field (NamedVectorField, engine.rs): the shard, id_map / reverse map, the config, and row_of with its stamp."""

    def __init__(self, name: str, dimension: int, metric: int, index_mode: str, dtypes: str, device: Optional[int]):
        from .core import FlatIndex

        self.name, self.dimension, self.metric, self.index_mode, self.dtypes = name, int(dimension), int(metric), index_mode, dtypes
        self.device = device
        self.flat = FlatIndex(None, self.dimension, device, "f16" if dtypes == "float16" else "f32")
        self.id_chunks: list = []     # field row -> user id
        self.reverse: dict = {}       # user id -> field row
        self.hnsw = False             # a graph over the field's rows (FlatIndex.build_hnsw)
        self.hnsw_rows = 0
        self.hnsw_opts: dict = {}
        self.rowmap: Optional[RowMap] = None
        self.rowmap_stamp = None      # (the collection's row stamp, the field's row count) row_of was built for

    def config(self) -> dict:
        return {"name": self.name, "dimension": self.dimension, "metric": metric_name(self.metric), "index_mode": self.index_mode,
                "dtypes": self.dtypes}

    def id_map(self) -> np.ndarray:
        if len(self.id_chunks) != 1:
            self.id_chunks = [np.concatenate(self.id_chunks) if self.id_chunks else np.zeros(0, np.int64)]
        return self.id_chunks[0]

    def __len__(self) -> int:
        return sum(int(c.size) for c in self.id_chunks)

    def append(self, vectors: np.ndarray, ids: np.ndarray) -> None:
        start = len(self)
        self.flat.write(vectors)
        self.id_chunks.append(ids.copy())
        for j, i in enumerate(ids.tolist()):
            self.reverse[i] = start + j

    def keep(self, keep: np.ndarray) -> None:
        """Compaction of the field: new row j is the j-th kept row."""
        ids = self.id_map()[keep]
        new_len = self.flat.compact(keep)
        assert new_len == ids.size
        self.id_chunks = [ids]
        self.reverse = {i: j for j, i in enumerate(ids.tolist())}
        self.rowmap_stamp = None

    def build_hnsw(self, metric: Optional[int] = None, opts: Optional[dict] = None) -> None:
        """The graph over the field's rows, with the metric and options given or those of the last build; they are kept only when the
        build succeeded."""
        from .core import HNSW_SEED

        metric = self.metric if metric is None else int(metric)
        o = self.hnsw_opts if opts is None else opts
        self.flat.build_hnsw(metric, o["m"], o["ef_construction"], o["ef_search"], o["max_level"], HNSW_SEED)
        self.metric, self.hnsw_opts = metric, o
        self.hnsw, self.hnsw_rows = True, len(self.flat)

    def extend_hnsw(self) -> None:
        """Vectors were added after the build: the graph takes them in (FlatIndex.extend_hnsw, equal to a build over every row); a
        handle that cannot extend its graph builds it again."""
        try:
            self.flat.extend_hnsw()
        except NotImplementedError:
            self.build_hnsw()
        self.hnsw_rows = len(self.flat)

    def drop_hnsw(self) -> None:
        self.flat.drop_hnsw()
        self.hnsw, self.hnsw_rows = False, 0
