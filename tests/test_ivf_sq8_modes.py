"""Host-only checks of the IVF-*-SQ8 surface: the index modes parse to their metric and quantizer, PQ stays refused, and the
C header declares the SQ8 entry points the Python layer binds."""
import pytest

from lynsedb_amd import _lib
from lynsedb_amd.core import ivf_quantizer_of, metric_from_index_mode


@pytest.mark.parametrize("mode,metric", [("IVF-IP-SQ8", _lib.METRIC_IP), ("IVF-L2-SQ8", _lib.METRIC_L2),
                                         ("IVF-COS-SQ8", _lib.METRIC_COSINE), ("IVF-COSINE-SQ8", _lib.METRIC_COSINE),
                                         ("ivf-cosine-sq8", _lib.METRIC_COSINE)])
def test_sq8_modes_parse_to_metric_and_quantizer(mode, metric):
    assert metric_from_index_mode(mode) == metric
    assert ivf_quantizer_of(mode) == "sq8"


@pytest.mark.parametrize("mode", ["IVF-IP", "IVF-L2", "IVF-COSINE", "IVF-HAMMING-BINARY", "IVF-JACCARD-BINARY"])
def test_other_ivf_modes_name_no_scalar_quantizer(mode):
    assert ivf_quantizer_of(mode) is None


@pytest.mark.parametrize("mode", ["IVF-IP-PQ", "IVF-L2-PQ", "IVF-HAMMING-SQ8"])
def test_pq_and_binary_sq8_are_refused(mode):
    with pytest.raises(NotImplementedError):
        ivf_quantizer_of(mode)


def test_sq8_entry_points_are_declared_and_bound():
    for sym in ("lynse_hip_ivf_build_sq8", "lynse_hip_ivf_load_sq8", "lynse_hip_ivf_sq8_params"):
        assert sym in _lib.SIGNATURES
        assert hasattr(_lib.lib, sym)
