"""The carried step tail of the 16x16x64 scan (scan_qs.h, CARRY) holds seven more fragments — 28 registers — across the barrier.  It is
only worth having while that fits: the M16 = 1 instantiations of 2..6 slabs under the ping-pong order keep 0 bytes of scratch, no spills
and two waves per SIMD in the build's resource report (read the way tests/test_qs16_resources.py reads it)."""
import re
from pathlib import Path


def test_carry_instantiations_hold_the_tail_in_registers():
    import lynsedb_amd  # noqa: F401  (build() has produced the library and the resource report)

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    assert rep.exists(), f"{rep}: the build writes the resource report next to the sources; without it this check says nothing"
    text = rep.read_text()
    # k_scan_qs<NSLAB, RB, SL, NS, XPF, NBUF, DBG, PING, STS, MET, SMP, MSK, F4, M16>: PING = 1 (eighth) and M16 = 1 (last) select the carry
    pat = re.compile(r"Function Name: (_ZN5lynse9k_scan_qsILi(\d+)E(?:L[ib]\d+E){6}Li1E(?:L[ib]\d+E){5}Li1EEEv\S*)(.*?)LDS Size", flags=re.S)
    seen = {}
    for name, nslab, body in pat.findall(text):
        f = {k: int(v) for k, v in re.findall(r"(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill): (\d+)", body)}
        assert f["ScratchSize [bytes/lane]"] == 0, (name, f)
        assert f["SGPRs Spill"] == 0 and f["VGPRs Spill"] == 0, (name, f)
        assert f["Occupancy [waves/SIMD]"] == 2, (name, f)
        assert f["VGPRs"] + f["AGPRs"] <= 256, (name, f)
        seen[int(nslab)] = f
    assert sorted(seen) == [2, 3, 4, 5, 6], sorted(seen)
