"""On-disk formats either side of the search path: what the reference writes, this
module reads into HBM shards — and writes back in the same bytes.

* segmented vector store — `vector_manifest.json` + raw little-endian row-major segment files, legacy
  single `vectors.bin` (src/storage/vector_store.rs:24-66, :160-215, :370-445);
* `id_map.bin` — one LE u64 user id per row; rows past its end map to themselves
  (src/engine.rs:2588-2617, :3071-3074);
* `<data>.ivf_meta.bin` of IvfFlatMmap — header (dim, n, n_partitions as LE u64), centroids f32,
  partition offsets u64, original ids u32, next to the slab-ordered data file
  (src/storage/ivf_flat_mmap.rs:448-530, :115-130).

Host logic only: parsing, validation and layout.  Searching needs the HIP library (no CPU fallback).
"""
from __future__ import annotations

import json
import os
from dataclasses import dataclass, field
from pathlib import Path, PurePosixPath
from typing import List, Optional, Sequence, Tuple

import numpy as np

VECTOR_MANIFEST_FILE = "vector_manifest.json"      # vector_store.rs:24
VECTOR_MANIFEST_VERSION = 1                        # :25
SEGMENT_DIR = "vector_segments"                    # :26
DEFAULT_ID_MAP_FILE = "id_map.bin"                 # :27
UPDATE_JOURNAL_FILE = "vector_updates.wal"         # :28
DEFAULT_SEGMENT_TARGET_BYTES = 256 * 1024 * 1024   # :32


class StorageError(IOError):
    """LynseError::Storage."""


@dataclass
class SegmentEntry:  # vector_store.rs:36-40
    file: str
    rows: int


@dataclass
class VectorManifest:  # vector_store.rs:42-48
    version: int = VECTOR_MANIFEST_VERSION
    generation: int = 0
    id_map_file: str = DEFAULT_ID_MAP_FILE
    segments: List[SegmentEntry] = field(default_factory=list)

    def to_json(self) -> str:
        return json.dumps({"version": self.version, "generation": self.generation, "id_map_file": self.id_map_file,
                           "segments": [{"file": s.file, "rows": s.rows} for s in self.segments]}, indent=2)


def dtype_width(dtype: str) -> int:
    """VectorDtype::parse + byte_width (src/storage/dtype.rs:12-29)."""
    d = dtype.strip().lower()
    if d in ("f32", "float32", "float"):
        return 4
    if d in ("f16", "float16", "half", "fp16"):
        return 2
    raise ValueError(f"unsupported vector dtype '{dtype}'; expected float32/f32 or float16/f16")


def validate_manifest_path(value: str, label: str) -> None:
    """vector_store.rs:68-81: a non-empty relative path made of normal components only."""
    p = PurePosixPath(value)
    bad = (not value) or p.is_absolute() or value.startswith("\\") or any(c in ("..", ".") for c in value.replace("\\", "/").split("/")) \
        or any(c == "" for c in value.replace("\\", "/").split("/"))
    if bad:
        raise StorageError(f"vector manifest {label} must be a safe relative path: {value!r}")


def load_manifest(collection_path, dim: int, dtype: str = "f32") -> VectorManifest:
    """VectorStore::new (vector_store.rs:160-215): parse or synthesise (legacy `vectors.bin`) the manifest, validate the
    paths, and take every segment's row count from its FILE LENGTH (a partial trailing row is ignored)."""
    root = Path(collection_path)
    row_width = dim * dtype_width(dtype)
    if (root / UPDATE_JOURNAL_FILE).exists():
        # VectorStore::has_pending_updates (vector_store.rs:682-687): in-place row updates that were journalled but not yet
        # applied to the segment files.  Replaying the journal is the storage engine's job (out of scope); serving the
        # segments as they are would silently return stale rows.
        raise StorageError(f"{root / UPDATE_JOURNAL_FILE} exists: the collection has pending row updates that were not applied to "
                           "its segment files; open it with LynseDB once (the journal is replayed on open) before loading it here")
    mpath = root / VECTOR_MANIFEST_FILE
    if mpath.exists():
        try:
            raw = json.loads(mpath.read_bytes())
            m = VectorManifest(int(raw["version"]), int(raw["generation"]), str(raw["id_map_file"]),
                               [SegmentEntry(str(s["file"]), int(s["rows"])) for s in raw["segments"]])
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError(f"vector manifest: {e}") from e  # LynseError::Serialization
        if m.version > VECTOR_MANIFEST_VERSION:
            raise StorageError(f"vector manifest version {m.version} is newer than supported version {VECTOR_MANIFEST_VERSION}")
    else:
        legacy = root / "vectors.bin"
        nbytes = legacy.stat().st_size if legacy.exists() else 0
        rows = 0 if row_width == 0 else nbytes // row_width
        m = VectorManifest(segments=[SegmentEntry("vectors.bin", rows)] if rows else [])
    validate_manifest_path(m.id_map_file, "ID-map path")
    seen = set()
    for s in m.segments:
        validate_manifest_path(s.file, "segment path")
        if s.file in seen:
            raise StorageError(f"vector manifest contains duplicate segment path {s.file!r}")
        seen.add(s.file)
    for s in m.segments:
        sp = root / s.file
        if not sp.exists():
            raise StorageError(f"vector manifest segment {sp} is unavailable: not found")
        s.rows = 0 if row_width == 0 else sp.stat().st_size // row_width
    return m


def load_id_map(path) -> np.ndarray:
    """engine.rs:2588-2603: LE u64 per row, partial trailing bytes ignored, missing file = empty."""
    p = Path(path)
    if not p.exists():
        return np.zeros(0, np.uint64)
    raw = p.read_bytes()
    return np.frombuffer(raw[:len(raw) // 8 * 8], dtype="<u8").astype(np.uint64)


def rows_to_user_ids(rows: np.ndarray, id_map: np.ndarray) -> np.ndarray:
    """row_to_user_id (engine.rs:3071-3074): id_map[row], or the row itself past the end of the map."""
    r = np.asarray(rows, np.uint64)
    out = r.copy()
    inside = r < id_map.size
    out[inside] = id_map[r[inside].astype(np.int64)]
    return out


def read_segments(collection_path, dim: int, dtype: str = "f32"):
    """Yield (first_global_row, rows[n, dim]) per segment in manifest order (global row = concatenation order,
    vector_store.rs:1016-1037): f32 values, or the u16 words of an F16 store."""
    root = Path(collection_path)
    m = load_manifest(root, dim, dtype)
    f16 = dtype_width(dtype) == 2  # F16 segments: the rows come back as their u16 words (FlatIndex.write_f16_bits)
    base = 0
    for s in m.segments:
        if s.rows:
            a = np.fromfile(root / s.file, dtype="<u2" if f16 else "<f4", count=s.rows * dim).reshape(s.rows, dim)
            yield base, a
        base += s.rows


def open_flat_collection(collection_path, dim: int, dtype: str = "f32", device: Optional[int] = None):
    """Load a collection directory written by the reference into one HBM shard.
    -> (FlatIndex, id_map u64[...], manifest).  Search rows are global rows; `rows_to_user_ids` maps them."""
    from .core import FlatIndex

    m = load_manifest(collection_path, dim, dtype)
    f16 = dtype_width(dtype) == 2
    idx = FlatIndex(None, dim, device, dtype="f16" if f16 else "f32")
    total = sum(s.rows for s in m.segments)
    if total:
        idx.reserve(total)
    for _, rows in read_segments(collection_path, dim, dtype):
        if f16:
            idx.write_f16_bits(rows)
        else:
            idx.write(rows)
    id_map = load_id_map(Path(collection_path) / m.id_map_file)
    return idx, id_map, m


def write_flat_collection(collection_path, batches: Sequence[np.ndarray], ids: Optional[np.ndarray] = None,
                          segment_target_bytes: int = DEFAULT_SEGMENT_TARGET_BYTES, dtype: str = "f32") -> VectorManifest:
    """Append `batches` the way VectorStore::write does (append_encoded_bytes, vector_store.rs:379-445): the first
    segment is `vectors.bin`; a batch that does not fit the current segment's target size opens
    `vector_segments/seg-{generation+1:020}-{index:06}.bin`; the manifest file appears with the second segment."""
    root = Path(collection_path)
    root.mkdir(parents=True, exist_ok=True)
    mpath = root / VECTOR_MANIFEST_FILE
    batches = list(batches)
    m = VectorManifest()
    if batches and (mpath.exists() or (root / "vectors.bin").exists()):
        # an existing collection is APPENDED to, like VectorStore::write: start from its manifest (row counts from the file
        # lengths), never truncate its segments
        m = load_manifest(root, int(np.asarray(batches[0]).shape[1]), dtype)
    elif mpath.exists() or (root / "vectors.bin").exists():
        return load_manifest(root, 0, dtype)
    for b in batches:
        # encode_f32_slice_as_le_bytes (src/storage/dtype.rs): F16 rounds to nearest even
        a = np.ascontiguousarray(b, dtype="<f4") if dtype_width(dtype) == 4 else np.ascontiguousarray(np.asarray(b, np.float32).astype("<f2"))
        row_width = a.shape[1] * dtype_width(dtype)
        target = max(segment_target_bytes, row_width)
        data = a.tobytes()
        fits = bool(m.segments) and m.segments[-1].rows * row_width + len(data) <= target
        if not m.segments or not fits:
            name = "vectors.bin" if (not m.segments and not mpath.exists()) else \
                f"{SEGMENT_DIR}/seg-{m.generation + 1:020d}-{len(m.segments):06d}.bin"
            p = root / name
            p.parent.mkdir(parents=True, exist_ok=True)
            p.write_bytes(data)
            m.generation += 1
            m.segments.append(SegmentEntry(name, a.shape[0]))
            if len(m.segments) > 1 or mpath.exists():
                tmp = mpath.with_suffix(".tmp")
                tmp.write_text(m.to_json())
                os.replace(tmp, mpath)
        else:
            with open(root / m.segments[-1].file, "ab") as f:
                f.write(data)
            m.segments[-1].rows += a.shape[0]
    if ids is not None:  # append_id_map_path (engine.rs:3058-3067): ids of the appended rows go to the end of the map
        with open(root / m.id_map_file, "ab") as f:
            f.write(np.ascontiguousarray(ids, dtype="<u8").tobytes())
    return m


# ------------------------------------------------------------------------------ IvfFlatMmap files
@dataclass
class IvfMeta:  # ivf_flat_mmap.rs:22-39
    dim: int
    n_vectors: int
    n_partitions: int
    centroids: np.ndarray          # f32 [n_partitions, dim]
    partition_offsets: np.ndarray  # u64 [n_partitions + 1]
    original_ids: np.ndarray       # u32 [n_vectors]: slab position -> original row


def ivf_meta_path(data_path) -> Path:
    """`data_path.with_extension("ivf_meta.bin")` (ivf_flat_mmap.rs:133)."""
    p = Path(data_path)
    return p.with_suffix(".ivf_meta.bin") if p.suffix else p.with_name(p.name + ".ivf_meta.bin")


def save_ivf_meta(path, meta: IvfMeta) -> None:  # ivf_flat_mmap.rs:448-482
    with open(path, "wb") as f:
        f.write(np.array([meta.dim, meta.n_vectors, meta.n_partitions], "<u8").tobytes())
        f.write(np.ascontiguousarray(meta.centroids, "<f4").tobytes())
        f.write(np.ascontiguousarray(meta.partition_offsets, "<u8").tobytes())
        f.write(np.ascontiguousarray(meta.original_ids, "<u4").tobytes())


def load_ivf_meta(path) -> IvfMeta:  # ivf_flat_mmap.rs:484-530
    raw = Path(path).read_bytes()
    if len(raw) < 24:
        raise IOError("failed to fill whole buffer")  # read_exact on a short file
    dim, n, k = (int(x) for x in np.frombuffer(raw[:24], "<u8"))
    need = 24 + k * dim * 4 + (k + 1) * 8 + n * 4
    if len(raw) < need:
        raise IOError("failed to fill whole buffer")
    o = 24
    cen = np.frombuffer(raw[o:o + k * dim * 4], "<f4").reshape(k, dim).astype(np.float32)
    o += k * dim * 4
    off = np.frombuffer(raw[o:o + (k + 1) * 8], "<u8").astype(np.uint64)
    o += (k + 1) * 8
    ids = np.frombuffer(raw[o:o + n * 4], "<u4").astype(np.uint32)
    return IvfMeta(dim, n, k, cen, off, ids)


def ivf_assignments_from_meta(meta: IvfMeta) -> np.ndarray:
    """assignment of every ORIGINAL row, from the slab layout (inverse of ivf_flat_mmap.rs:105-130)."""
    part_of_pos = np.repeat(np.arange(meta.n_partitions, dtype=np.uint32), np.diff(meta.partition_offsets.astype(np.int64)))
    asg = np.zeros(meta.n_vectors, np.uint32)
    asg[meta.original_ids.astype(np.int64)] = part_of_pos
    return asg


def open_ivf_flat(data_path, metric: str = "ip", device: Optional[int] = None):
    """IvfFlatMmap::open (ivf_flat_mmap.rs:161-223): the slab-ordered data file + its `.ivf_meta.bin`.
    -> IvfFlatIndex with the IvfFlat routing semantics; search results are ORIGINAL row ids."""
    from .core import IvfFlatIndex

    meta = load_ivf_meta(ivf_meta_path(data_path))
    slab = np.fromfile(data_path, dtype="<f4", count=meta.n_vectors * meta.dim)
    if slab.size != meta.n_vectors * meta.dim:
        raise IOError("IVF data file is shorter than its metadata")
    slab = slab.reshape(meta.n_vectors, meta.dim)
    original = np.empty_like(slab)
    original[meta.original_ids.astype(np.int64)] = slab  # back to original row order; load() rebuilds the same slabs
    return IvfFlatIndex.load(original, meta.centroids, ivf_assignments_from_meta(meta), metric, device=device, ivfflat_routing=True)


def save_ivf_flat(data_path, index, data: np.ndarray) -> IvfMeta:
    """Write what IvfFlatMmap::build writes (ivf_flat_mmap.rs:105-150) for a built index over `data` (original order)."""
    cen, asg, off, orig = index.export()
    slab = np.ascontiguousarray(np.asarray(data, np.float32)[orig.astype(np.int64)], dtype="<f4")
    Path(data_path).write_bytes(slab.tobytes())
    meta = IvfMeta(cen.shape[1], slab.shape[0], cen.shape[0], cen, off, orig)
    save_ivf_meta(ivf_meta_path(data_path), meta)
    return meta


# ---- pq_index.bin (PQIndex::save / load, src/storage/pq_mmap.rs:431-541) ------------------------------------------------------
PQ_MAGIC = 0x5051_4D4D   # "PQMM"
PQ_VERSION = 1


@dataclass
class PqIndexFile:
    n_subspaces: int
    n_clusters: int
    subspace_size: int
    dim: int
    codebooks: np.ndarray   # f32 [M][K][ss]
    codes: np.ndarray       # u8 [n][M]

    @property
    def n_vectors(self) -> int:
        return int(self.codes.shape[0])


def save_pq_index(path, pq: PqIndexFile) -> None:
    """32-byte little-endian header (magic, version, M, K, ss as u32, n as u64, dim as u32), the f32 codebooks, the u8 codes."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    cb = np.ascontiguousarray(pq.codebooks, dtype="<f4").reshape(-1)
    codes = np.ascontiguousarray(pq.codes, dtype=np.uint8).reshape(-1)
    header = np.array([PQ_MAGIC, PQ_VERSION, pq.n_subspaces, pq.n_clusters, pq.subspace_size], "<u4").tobytes()
    header += np.array([pq.n_vectors], "<u8").tobytes() + np.array([pq.dim], "<u4").tobytes()
    with open(path, "wb") as f:
        f.write(header)
        f.write(cb.tobytes())
        f.write(codes.tobytes())


def load_pq_index(path) -> PqIndexFile:
    """PQIndex::load with the reference's checks and messages (IOError = its io::Error)."""
    raw = Path(path).read_bytes()
    if len(raw) < 32:
        if len(raw) >= 4 and int(np.frombuffer(raw[:4], "<u4")[0]) != PQ_MAGIC:
            raise IOError("Invalid PQ magic bytes")
        raise IOError("failed to fill whole buffer")
    magic, version, m, k, ss = (int(x) for x in np.frombuffer(raw[:20], "<u4"))
    n = int(np.frombuffer(raw[20:28], "<u8")[0])
    dim = int(np.frombuffer(raw[28:32], "<u4")[0])
    if magic != PQ_MAGIC:
        raise IOError("Invalid PQ magic bytes")
    if version != PQ_VERSION:
        raise IOError(f"Unsupported PQ version: {version}")
    if m == 0 or not (1 <= k <= 256) or ss == 0 or m * ss != dim or n > 0xFFFFFFFF:
        raise IOError("Invalid PQ index dimensions")
    cb_len, code_len = m * k * ss, n * m
    if len(raw) < 32 + 4 * cb_len + code_len:
        raise IOError("failed to fill whole buffer")
    cb = np.frombuffer(raw, "<f4", cb_len, 32).astype(np.float32).reshape(m, k, ss)
    codes = np.frombuffer(raw, np.uint8, code_len, 32 + 4 * cb_len).reshape(n, m).copy()
    if codes.size and int(codes.max()) >= k:
        raise IOError("PQ index contains an out-of-range code")
    return PqIndexFile(m, k, ss, dim, cb, codes)


# ---- rabitq_index.bin (RaBitQIndex::save / load, src/storage/rabitq_mmap.rs:236-330) ------------------------------------------
RABITQ_MAGIC = 0x5242_5451   # "RBTQ"
RABITQ_VERSION = 2


def next_power_of_two(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


@dataclass
class RabitqIndexFile:
    dim: int
    padded_dim: int
    sign_words: np.ndarray   # u64 [n_sign_words]
    codes: np.ndarray        # u8 [n][ceil(padded_dim / 8)]
    norms: np.ndarray        # f32 [n]

    @property
    def n_vectors(self) -> int:
        return int(self.codes.shape[0])

    @property
    def code_bytes(self) -> int:
        return (self.padded_dim + 7) // 8


def save_rabitq_index(path, idx: RabitqIndexFile) -> None:
    """Version 2, little endian: u32 magic, version, dim, padded_dim; u64 n; u32 n_sign_words; the u64 sign words; the u8 codes
    [n][code_bytes]; the f32 norms [n]."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    sw = np.ascontiguousarray(idx.sign_words, dtype="<u8").reshape(-1)
    codes = np.ascontiguousarray(idx.codes, dtype=np.uint8).reshape(idx.n_vectors, idx.code_bytes)
    norms = np.ascontiguousarray(idx.norms, dtype="<f4").reshape(-1)
    if norms.shape[0] != idx.n_vectors:
        raise ValueError("norms must hold one value per code row")
    header = np.array([RABITQ_MAGIC, RABITQ_VERSION, idx.dim, idx.padded_dim], "<u4").tobytes()
    header += np.array([idx.n_vectors], "<u8").tobytes() + np.array([sw.shape[0]], "<u4").tobytes()
    with open(path, "wb") as f:
        f.write(header)
        f.write(sw.tobytes())
        f.write(codes.tobytes())
        f.write(norms.tobytes())


def load_rabitq_index(path) -> RabitqIndexFile:
    """RaBitQIndex::load with the reference's checks, in its order, and its messages (IOError = its io::Error).  Versions 1 and 2
    are read alike: version 1 wrote floor(padded_dim / 8) code bytes, which differs only below 8, where it is refused."""
    raw = Path(path).read_bytes()

    def take(off, count, fmt):
        size = count * np.dtype(fmt).itemsize
        if len(raw) < off + size:
            raise IOError("failed to fill whole buffer")
        return np.frombuffer(raw, fmt, count, off), off + size

    v, off = take(0, 1, "<u4")
    if int(v[0]) != RABITQ_MAGIC:
        raise IOError("Invalid RaBitQ magic bytes")
    v, off = take(off, 1, "<u4")
    version = int(v[0])
    if not (1 <= version <= RABITQ_VERSION):
        raise IOError(f"Unsupported RaBitQ version: {version}")
    v, off = take(off, 2, "<u4")
    dim, padded = int(v[0]), int(v[1])
    v, off = take(off, 1, "<u8")
    n = int(v[0])
    if dim == 0 or padded != next_power_of_two(dim):
        raise IOError("Invalid RaBitQ dimensions")
    if version == 1 and padded < 8:
        raise IOError("RaBitQ v1 index is invalid for dimensions below 8")
    cb = (padded + 7) // 8
    v, off = take(off, 1, "<u4")
    sw, off = take(off, int(v[0]), "<u8")
    codes, off = take(off, n * cb, np.uint8)
    norms, off = take(off, n, "<f4")
    return RabitqIndexFile(dim, padded, sw.astype(np.uint64), codes.reshape(n, cb).copy(), norms.astype(np.float32))


# ---- polarvec_index.bin (PolarVecIndex::save / load, src/storage/polarvec_mmap.rs:379-581) -------------------------------------
POLARVEC_MAGIC = 0x504C_5651   # "PLVQ"
POLARVEC_VERSION = 5
POLARVEC_FLAG_RESIDUAL_SQ, POLARVEC_FLAG_INV_V_HAT_NORMS = 1, 2


@dataclass
class PolarvecIndexFile:
    dim: int
    padded_dim: int
    bits: int
    sign_words: np.ndarray    # u64 [ceil(padded_dim / 64)]
    dim_mins: np.ndarray      # f32 [padded_dim]
    dim_scales: np.ndarray    # f32 [padded_dim]
    codes: np.ndarray         # u8 [n][ceil(padded_dim * bits / 8)]
    residual_sq: Optional[np.ndarray] = None       # f32 [n], kept by an index built for L2 (flag 1)
    inv_v_hat_norms: Optional[np.ndarray] = None   # f32 [n], kept by an index built for cosine (flag 2)

    @property
    def n_vectors(self) -> int:
        return int(self.codes.shape[0])

    @property
    def bytes_per_vec(self) -> int:
        return (self.padded_dim * self.bits + 7) // 8

    @property
    def flags(self) -> int:
        return ((POLARVEC_FLAG_RESIDUAL_SQ if self.residual_sq is not None else 0) |
                (POLARVEC_FLAG_INV_V_HAT_NORMS if self.inv_v_hat_norms is not None else 0))


def save_polarvec_index(path, idx: PolarvecIndexFile) -> None:
    """Version 5, little endian: u32 magic, version, dim, padded_dim, bits; u64 n; u32 flags; u32 n_sign_words; the u64 sign words; the
    f32 dim_mins and dim_scales [padded_dim]; the u8 codes [n][bytes_per_vec]; then the f32 [n] arrays the flags name, residual_sq
    first.  (The reference leaves out an EMPTY array; an index holds at least one row here, so present and non-empty are the same.)"""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    n = idx.n_vectors
    sw = np.ascontiguousarray(idx.sign_words, dtype="<u8").reshape(-1)
    mins = np.ascontiguousarray(idx.dim_mins, dtype="<f4").reshape(-1)
    scales = np.ascontiguousarray(idx.dim_scales, dtype="<f4").reshape(-1)
    codes = np.ascontiguousarray(idx.codes, dtype=np.uint8).reshape(n, idx.bytes_per_vec)
    if mins.shape[0] != idx.padded_dim or scales.shape[0] != idx.padded_dim:
        raise ValueError("dim_mins and dim_scales must hold one value per padded dimension")
    tail = []
    for a in (idx.residual_sq, idx.inv_v_hat_norms):
        if a is not None:
            a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
            if a.shape[0] != n:
                raise ValueError("a correction array must hold one value per code row")
            tail.append(a)
    header = np.array([POLARVEC_MAGIC, POLARVEC_VERSION, idx.dim, idx.padded_dim, idx.bits], "<u4").tobytes()
    header += np.array([n], "<u8").tobytes() + np.array([idx.flags, sw.shape[0]], "<u4").tobytes()
    with open(path, "wb") as f:
        f.write(header)
        f.write(sw.tobytes())
        f.write(mins.tobytes())
        f.write(scales.tobytes())
        f.write(codes.tobytes())
        for a in tail:
            f.write(a.tobytes())


def load_polarvec_index(path) -> PolarvecIndexFile:
    """PolarVecIndex::load with the reference's checks, in its order, and its messages (IOError = its io::Error).  Only version 5 is
    read: versions 1-4 (which carry norms, sign sketches and implied arrays) are refused as unsupported."""
    raw = Path(path).read_bytes()

    def take(off, count, fmt):
        size = count * np.dtype(fmt).itemsize
        if len(raw) < off + size:
            raise IOError("failed to fill whole buffer")
        return np.frombuffer(raw, fmt, count, off), off + size

    v, off = take(0, 1, "<u4")
    if int(v[0]) != POLARVEC_MAGIC:
        raise IOError("Invalid PolarVec magic bytes")
    v, off = take(off, 1, "<u4")
    version = int(v[0])
    if version != POLARVEC_VERSION:
        raise IOError(f"Unsupported PolarVec version: {version}")
    v, off = take(off, 3, "<u4")
    dim, padded, bits = (int(x) for x in v)
    v, off = take(off, 1, "<u8")
    n = int(v[0])
    if dim == 0 or padded != next_power_of_two(dim) or not (1 <= bits <= 8) or n > 0xFFFFFFFF:
        raise IOError("Invalid PolarVec index dimensions")
    v, off = take(off, 1, "<u4")
    flags = int(v[0])
    if flags & ~(POLARVEC_FLAG_RESIDUAL_SQ | POLARVEC_FLAG_INV_V_HAT_NORMS):
        raise IOError("PolarVec index contains unknown flags")
    v, off = take(off, 1, "<u4")
    if int(v[0]) != (padded + 63) // 64:
        raise IOError("Invalid PolarVec sign-word count")
    sw, off = take(off, int(v[0]), "<u8")
    mins, off = take(off, padded, "<f4")
    scales, off = take(off, padded, "<f4")
    bpv = (padded * bits + 7) // 8
    codes, off = take(off, n * bpv, np.uint8)
    residual = inv = None
    if flags & POLARVEC_FLAG_RESIDUAL_SQ:
        residual, off = take(off, n, "<f4")
        residual = residual.astype(np.float32)
    if flags & POLARVEC_FLAG_INV_V_HAT_NORMS:
        inv, off = take(off, n, "<f4")
        inv = inv.astype(np.float32)
    return PolarvecIndexFile(dim, padded, bits, sw.astype(np.uint64), mins.astype(np.float32), scales.astype(np.float32),
                             codes.reshape(n, bpv).copy(), residual, inv)


# ---- sparse vectors: sparse_vectors.jsonl (SparseVectorRecord / SparseVectorStore, src/engine.rs:550-718) ----

def _f32_json(x) -> str:
    """the shortest decimal that reads back as the f32 `x`, laid out as serde_json's writer does (ryu): positional with at least one
    fraction digit for 1e-5 <= |x| < 1e16, else d.ddde[-]X"""
    x = np.float32(x)
    if x == 0:
        return "-0.0" if np.signbit(x) else "0.0"
    mant, exp = np.format_float_scientific(x, unique=True, trim="-").split("e")
    sign = "-" if mant.startswith("-") else ""
    digits = mant.lstrip("-").replace(".", "")
    e10 = int(exp)
    if -5 <= e10 < 16:
        if e10 < 0:
            body = "0." + "0" * (-e10 - 1) + digits
        elif len(digits) <= e10 + 1:
            body = digits + "0" * (e10 + 1 - len(digits)) + ".0"
        else:
            body = digits[:e10 + 1] + "." + digits[e10 + 1:]
        return sign + body
    return sign + digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e" + str(e10)


def save_sparse_vectors(path, vectors: dict) -> None:
    """SparseVectorStore::write_records (:697-717): one {"id":u64,"indices":[u32],"values":[f32]} record per line in ascending id
    order, written to a temporary file and renamed into place.  `vectors`: id -> (indices, values), normalised."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    lines = []
    for i in sorted(vectors):
        idx, val = vectors[i]
        lines.append('{"id":%d,"indices":[%s],"values":[%s]}\n' % (int(i), ",".join(str(int(x)) for x in idx), ",".join(_f32_json(v) for v in val)))
    tmp = path.with_name(path.name + ".tmp")
    with open(tmp, "w", encoding="utf-8") as f:
        f.write("".join(lines))
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def load_sparse_vectors(path) -> dict:
    """SparseVectorStore::load (:573-617): blank lines skipped, an indices / values length mismatch refused with the reference's
    message, every record normalised (normalize_sparse_entries), a record that normalises to empty removes its id, a later line for
    an id wins -> id -> (indices u32, values f32).  A missing file is an empty store."""
    from .core import sparse_normalize_arrays

    path = Path(path)
    out: dict = {}
    if not path.exists():
        return out
    for line_no, line in enumerate(path.read_text(encoding="utf-8").splitlines()):
        line = line.strip()
        if not line:
            continue
        try:
            rec = json.loads(line)
            rid, indices, values = rec["id"], rec["indices"], rec["values"]
            if not isinstance(rid, int) or isinstance(rid, bool) or rid < 0 or rid > 0xFFFFFFFFFFFFFFFF or any((not isinstance(x, int)) or isinstance(x, bool) or x < 0 or x > 0xFFFFFFFF for x in indices):
                raise ValueError("id and indices must be unsigned integers")
            vals = np.array([float(v) for v in values], dtype=np.float64)
        except (ValueError, KeyError, TypeError) as e:
            raise StorageError(f"failed to parse sparse vector record at line {line_no + 1}: {e}") from None
        if len(indices) != len(values):
            raise StorageError(f"sparse vector record for id {rid} has {len(indices)} indices but {len(values)} values")
        with np.errstate(over="ignore"):
            v32 = vals.astype(np.float32)
        try:
            _, idx, val = sparse_normalize_arrays(np.array([0, len(indices)], np.uint64), np.array(indices, np.uint32), v32)
        except ValueError as e:
            raise StorageError(str(e)) from None
        if idx.size == 0:
            out.pop(rid, None)
        else:
            out[rid] = (idx, val)
    return out
