"""FLAT-*-POLARVEC<b> on the CPU: mode parsing and refusals, the polarvec_index.bin codec (src/storage/polarvec_mmap.rs:379-581), the
restatement's bit packing across byte boundaries, and the scan kernels' resource report."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import polarvec_common as PC
from lynsedb_amd.core import POLARVEC_OVERSAMPLE, flat_polarvec_mode, flat_pq_mode, flat_rabitq_mode
from lynsedb_amd.storage import (POLARVEC_MAGIC, POLARVEC_VERSION, PolarvecIndexFile, load_polarvec_index, next_power_of_two,
                                 save_polarvec_index)

f32 = np.float32


def test_modes_and_refusals():
    assert POLARVEC_OVERSAMPLE == 20
    for bits in range(1, 9):
        for metric in ("IP", "L2", "COS", "COSINE"):
            mode = f"FLAT-{metric}-POLARVEC{bits}"
            assert flat_polarvec_mode(mode) == bits
            assert not flat_pq_mode(mode) and not flat_rabitq_mode(mode)
    for mode in ("FLAT-IP-POLARVEC0", "FLAT-L2-POLARVEC9", "FLAT-COS-POLARVEC12"):   # parse_bits: outside 1..8 = the default
        assert flat_polarvec_mode(mode) == 4
    assert flat_polarvec_mode("flat-l2-polarvec5") == 5
    assert flat_polarvec_mode("FLAT-COSINE-POLARVEC3") == 3
    for mode in ("FLAT-IP-POLARVEC", "FLAT-L2-POLARVEC", "flat-cos-polarvec"):   # the reference reads 4 bits; refused here
        with pytest.raises(NotImplementedError):
            flat_polarvec_mode(mode)
    for mode in ("FLAT-HAMMING-POLARVEC4", "FLAT-JACCARD-POLARVEC8"):
        with pytest.raises(NotImplementedError):
            flat_polarvec_mode(mode)
    for mode in ("FLAT-IP", "FLAT-IP-RABITQ", "IVF-IP-POLARVEC4", "FLAT-IP-PQ8", "FLAT-L2-SQ8"):
        assert flat_polarvec_mode(mode) is None


# ---- polarvec_index.bin ----
def _index(n=5, dim=20, bits=4, flags=3, seed=1):
    rng = np.random.default_rng(seed)
    P = next_power_of_two(dim)
    return PolarvecIndexFile(dim, P, bits, rng.integers(0, 1 << 63, (P + 63) // 64, dtype=np.uint64),
                             rng.standard_normal(P).astype(f32), rng.random(P).astype(f32),
                             rng.integers(0, 256, (n, (P * bits + 7) // 8), dtype=np.uint8),
                             rng.random(n).astype(f32) if flags & 1 else None, rng.random(n).astype(f32) if flags & 2 else None)


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_codec_against_hand_assembled_bytes(tmp_path, flags):
    """dim 3 -> padded 4, bits 4: two code bytes per row, one sign word; two rows; no array, residual_sq, inv_v_hat_norms."""
    tail = {0: b"", 1: b"\x00\x00\x00\x3f" + b"\x00\x00\x40\x40", 2: b"\x00\x00\x80\x3e" + b"\x00\x00\x00\x41"}[flags]
    raw = (b"\x51\x56\x4c\x50" + b"\x05\x00\x00\x00" + b"\x03\x00\x00\x00" + b"\x04\x00\x00\x00" + b"\x04\x00\x00\x00" +
           b"\x02" + b"\x00" * 7 + bytes([flags]) + b"\x00\x00\x00" + b"\x01\x00\x00\x00" + b"\xef\xcd\xab\x89\x67\x45\x23\x01" +
           b"\x00\x00\x80\xbf" + b"\x00\x00\x00\x00" + b"\x00\x00\x00\x80" + b"\x00\x00\x00\x40" +      # dim_mins -1, 0, -0, 2
           b"\x00\x00\x80\x3f" * 3 + b"\x00\x00\x00\x3f" +                                               # dim_scales 1, 1, 1, 0.5
           b"\x21\x43" + b"\xa5\x0f" + tail)
    idx = PolarvecIndexFile(3, 4, 4, np.array([0x0123456789ABCDEF], np.uint64), np.array([-1.0, 0.0, -0.0, 2.0], f32),
                            np.array([1.0, 1.0, 1.0, 0.5], f32), np.array([[0x21, 0x43], [0xA5, 0x0F]], np.uint8),
                            np.array([0.5, 3.0], f32) if flags == 1 else None, np.array([0.25, 8.0], f32) if flags == 2 else None)
    path = tmp_path / "polarvec_index.bin"
    save_polarvec_index(path, idx)
    assert path.read_bytes() == raw
    back = load_polarvec_index(path)
    assert (back.dim, back.padded_dim, back.bits, back.bytes_per_vec, back.n_vectors, back.flags) == (3, 4, 4, 2, 2, flags)
    assert back.sign_words.tolist() == [0x0123456789ABCDEF]
    assert back.dim_mins.view(np.uint32).tolist() == [0xBF800000, 0, 0x80000000, 0x40000000]
    assert back.dim_scales.tolist() == [1.0, 1.0, 1.0, 0.5]
    assert back.codes.tolist() == [[0x21, 0x43], [0xA5, 0x0F]]
    assert (back.residual_sq is None) == (flags != 1) and (back.inv_v_hat_norms is None) == (flags != 2)
    if flags == 1:
        assert back.residual_sq.tolist() == [0.5, 3.0]
    if flags == 2:
        assert back.inv_v_hat_norms.tolist() == [0.25, 8.0]


def test_codec_round_trip_with_a_nan(tmp_path):
    idx = _index(n=37, dim=300, bits=3, flags=3)
    idx.residual_sq[3] = np.nan
    idx.dim_mins[7] = np.nan
    idx.dim_mins[8] = np.inf
    path = tmp_path / "sub" / "polarvec_index.bin"
    save_polarvec_index(path, idx)
    raw = path.read_bytes()
    assert len(raw) == 36 + 8 * 8 + 2 * 512 * 4 + 37 * 192 + 2 * 37 * 4
    assert np.frombuffer(raw[:20], "<u4").tolist() == [POLARVEC_MAGIC, POLARVEC_VERSION, 300, 512, 3]
    back = load_polarvec_index(path)
    assert np.array_equal(back.sign_words, idx.sign_words) and np.array_equal(back.codes, idx.codes)
    for a, b in ((back.dim_mins, idx.dim_mins), (back.dim_scales, idx.dim_scales), (back.residual_sq, idx.residual_sq),
                 (back.inv_v_hat_norms, idx.inv_v_hat_norms)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _patched(tmp_path, raw, off, value, fmt="<u4"):
    b = bytearray(raw)
    v = np.array([value], fmt).tobytes()
    b[off:off + len(v)] = v
    p = tmp_path / "bad.bin"
    p.write_bytes(bytes(b))
    return p


def test_codec_rejections_and_a_short_file(tmp_path):
    path = tmp_path / "polarvec_index.bin"
    save_polarvec_index(path, _index())
    raw = path.read_bytes()
    # offsets: magic 0, version 4, dim 8, padded_dim 12, bits 16, n 20 (u64), flags 28, n_sign_words 32
    cases = [(0, 0x1234, "Invalid PolarVec magic bytes"), (4, 0, "Unsupported PolarVec version: 0"), (4, 6, "Unsupported PolarVec version: 6"),
             (4, 4, "Unsupported PolarVec version: 4"),   # versions 1-4 are not read by this build
             (8, 0, "Invalid PolarVec index dimensions"), (12, 16, "Invalid PolarVec index dimensions"),
             (8, 33, "Invalid PolarVec index dimensions"), (16, 0, "Invalid PolarVec index dimensions"),
             (16, 9, "Invalid PolarVec index dimensions"), (28, 4, "PolarVec index contains unknown flags"),
             (28, 0x80000001, "PolarVec index contains unknown flags"), (32, 2, "Invalid PolarVec sign-word count"),
             (32, 0, "Invalid PolarVec sign-word count")]
    for off, val, msg in cases:
        with pytest.raises(IOError, match=msg):
            load_polarvec_index(_patched(tmp_path, raw, off, val))
    with pytest.raises(IOError, match="Invalid PolarVec index dimensions"):
        load_polarvec_index(_patched(tmp_path, raw, 20, 1 << 32, "<u8"))
    short = tmp_path / "short.bin"
    for cut in (len(raw) - 1, len(raw) - 21, 100, 34, 30, 10, 3):
        short.write_bytes(raw[:cut])
        with pytest.raises(IOError, match="failed to fill whole buffer"):
            load_polarvec_index(short)


# ---- the restatement's packing ----
@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return PC.compile_ref(tmp_path_factory.mktemp("polarvec_ref"))


@pytest.mark.parametrize("bits", [3, 5])
def test_restatement_packs_across_byte_boundaries(ref, bits):
    """Codes of a known pattern, packed one dimension at a time in a scrambled order (a later write must not disturb a neighbour), against
    the bit string assembled in Python: dimension d at bits [d * bits, (d + 1) * bits), LSB first."""
    P = 16
    codes = [(7 * d + 3) % (1 << bits) for d in range(P)]
    row = np.full((P * bits + 7) // 8, 0xFF, np.uint8)   # stale bits everywhere: packing overwrites exactly its own
    for d in sorted(range(P), key=lambda d: (d * 5) % P):
        ref.plr_pack(row.ctypes.data_as(C.c_void_p), d, codes[d], bits)
    stream = sum(c << (d * bits) for d, c in enumerate(codes))
    assert row.tolist() == list(stream.to_bytes(row.size, "little"))
    assert [ref.plr_unpack(row.ctypes.data_as(C.c_void_p), d, bits) for d in range(P)] == codes
    spans = [d for d in range(P) if (d * bits) // 8 != (d * bits + bits - 1) // 8]
    assert spans, "no code crosses a byte at this width"
    # hand-checked: bits 3, codes 3, 2, 1 -> 0b001_010_011 = 0x53 and bit 8 = 0
    if bits == 3:
        assert codes[:3] == [3, 2, 1] and row[0] == 0x53 and row[1] & 1 == 0


def test_restatement_rounds_half_away_and_clamps(ref):
    assert [ref.plr_code(v, 0.0, 1.0, 16) for v in (0.5, 1.5, 2.5, -0.5, -3.0, 14.5, 99.0)] == [1, 2, 3, 0, 0, 15, 15]
    assert ref.plr_code(float("nan"), 0.0, 1.0, 16) == 0
    assert ref.plr_code(float("inf"), 0.0, 1.0, 16) == 15


def test_scan_kernels_have_no_scratch_spills():
    import lynsedb_amd

    rep = Path(lynsedb_amd.__file__).parent / "csrc" / "resource_usage.txt"
    if not rep.exists():
        pytest.skip("resource report not produced by this build")
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", rep.read_text(), flags=re.S)
    scans = [(name, int(scratch)) for name, scratch in blocks if "k_plv_scan" in name]
    assert len(scans) == 8, scans   # four classes x QB 4 / 1
    assert all(scratch == 0 for _, scratch in scans), scans
