"""lynsedb_amd — MI355X-native FLAT / IVF-Flat search behind the `lynse._core` surface.

Importing this package loads liblynse_hip.so (hand-written HIP kernels for gfx950).  There is no
CPU fallback: the import fails loudly if the extension has not been built.
"""
from . import _lib  # noqa: F401  (raises ImportError when the HIP extension is missing)
from .core import (BitSet, Collection, DatabaseManager, FlatIndex, IvfFlatIndex, SearchResult, SparseIndex, SpannIndex, TextIndex,  # noqa: F401
                   default_device, visible_devices, merge_topk, metric_from_index_mode, metric_from_str, normalize_sparse_vector,
                   py_compute_distance, py_top_k_search, tokenize_text)
from .vector_fields import (RowMap, normalize_field_index_mode, resolve_named_vector_metric, validate_vector_field_name,  # noqa: F401
                            vector_dtype_name)

__all__ = ["BitSet", "Collection", "DatabaseManager", "FlatIndex", "IvfFlatIndex", "SearchResult", "SparseIndex", "SpannIndex", "TextIndex", "default_device", "visible_devices",
           "merge_topk", "metric_from_index_mode", "metric_from_str", "normalize_sparse_vector", "py_compute_distance", "py_top_k_search", "tokenize_text",
           "RowMap", "normalize_field_index_mode", "resolve_named_vector_metric", "validate_vector_field_name", "vector_dtype_name"]
__version__ = "0.1.0"
