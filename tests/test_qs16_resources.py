"""The 16x16x64 instantiations of k_scan_qs (scan_qs.h, M16) in the build's resource report: no scratch, no spills, two waves per SIMD.
The form is only worth having while it costs no more registers than the 32x32x32 one; the report is read the way
tests/test_cabi_and_host.py reads it for the other hot kernels."""
import re
from pathlib import Path

import pytest


def test_m16_instantiations_fit_the_register_file():
    import lynsedb_amd  # noqa: F401  (build() has produced the library and the resource report)

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    if not rep.exists():
        pytest.skip("resource report not produced by this build")
    text = rep.read_text()
    # k_scan_qs<NSLAB, RB, SL, NS, XPF, NBUF, DBG, PING, STS, MET, SMP, MSK, F4, M16>: the last template argument is M16
    pat = re.compile(r"Function Name: (_ZN5lynse9k_scan_qsILi(\d+)E(?:L[ib]\d+E){12}Li1EEEv\S*)(.*?)LDS Size", flags=re.S)
    seen = {}
    for name, nslab, body in pat.findall(text):
        f = {k: int(v) for k, v in re.findall(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", body)}
        assert f["ScratchSize [bytes/lane]"] == 0 and f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (name, f)
        assert f["Occupancy [waves/SIMD]"] == 2, (name, f)
        assert f["VGPRs"] + f["AGPRs"] <= 256, (name, f)
        seen[int(nslab)] = f
    # the tilings launch_scan_qs picks the form for: 256 / 384 / 512 / 640 / 768 columns
    assert sorted(seen) == [2, 3, 4, 5, 6], sorted(seen)
