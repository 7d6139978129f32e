"""FLAT-*-RABITQ on the CPU: mode parsing and refusals, the sign words of SmallRng::seed_from_u64(42) and the rabitq_index.bin
codec (src/storage/rabitq_mmap.rs:236-330, :337-340)."""
import ctypes as C

import numpy as np
import pytest

from lynsedb_amd import _lib
from lynsedb_amd.core import RABITQ_OVERSAMPLE, flat_pq_mode, flat_rabitq_mode
from lynsedb_amd.storage import (RABITQ_MAGIC, RABITQ_VERSION, RabitqIndexFile, load_rabitq_index, next_power_of_two,
                                 save_rabitq_index)

M64 = (1 << 64) - 1


def test_modes_and_refusals():
    assert RABITQ_OVERSAMPLE == 200
    for mode in ("FLAT-IP-RABITQ", "FLAT-L2-RABITQ", "FLAT-COS-RABITQ", "FLAT-COSINE-RABITQ", "flat-l2-rabitq"):
        assert flat_rabitq_mode(mode)
        assert not flat_pq_mode(mode)
    for mode in ("FLAT-IP", "FLAT-IP-SQ8", "FLAT-IP-PQ8", "IVF-IP-RABITQ", "SPANN-L2"):
        assert not flat_rabitq_mode(mode)
    for mode in ("FLAT-HAMMING-RABITQ", "FLAT-JACCARD-RABITQ"):
        with pytest.raises(NotImplementedError):
            flat_rabitq_mode(mode)
    for mode in ("FLAT-IP-POLARVEC", "FLAT-L2-POLARVEC"):
        with pytest.raises(NotImplementedError):
            flat_rabitq_mode(mode)


# ---- the sign words: three independent statements of the same stream ----
def splitmix_stream(seed, count):
    out, st = [], seed
    for _ in range(count):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        out.append(z ^ (z >> 31))
    return out


def xoshiro_stream(state, count):
    s, out = list(state), []
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
    for _ in range(count):
        out.append((rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64)
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t
        s[3] = rotl(s[3], 45)
    return out


def lib_sign_words(seed, count):
    out = (C.c_uint64 * max(count, 1))()
    assert _lib.lib.lynse_hip_rabitq_sign_words(seed, count, out) == 0
    return list(out)[:count]


def test_restatement_reproduces_the_published_vectors():
    """xoshiro256++ from state (1, 2, 3, 4) and SplitMix64 from 1234567, as published with the generators' reference code."""
    assert xoshiro_stream((1, 2, 3, 4), 4) == [41943041, 58720359, 3588806011781223, 3591011842654386]
    assert splitmix_stream(1234567, 3) == [6457827717110365317, 3203168211198807973, 9817491932198370423]


@pytest.mark.parametrize("seed,count", [(42, 1), (42, 16), (42, 512), (0, 5), (7, 33)])
def test_sign_words_against_python_and_the_pq_streams(seed, count):
    got = lib_sign_words(seed, count)
    assert got == xoshiro_stream(splitmix_stream(seed, 4), count)
    state = (C.c_uint64 * 4)()
    assert _lib.lib.lynse_hip_pq_splitmix_stream(seed, 4, state) == 0
    out = (C.c_uint64 * count)()
    assert _lib.lib.lynse_hip_pq_xoshiro_stream(state, count, out) == 0
    assert got == list(out)


def test_sign_words_edge_arguments():
    assert lib_sign_words(42, 0) == []
    assert _lib.lib.lynse_hip_rabitq_sign_words(42, 3, None) != 0
    assert lib_sign_words(42, 16)[:3] == lib_sign_words(42, 3)   # a prefix: word w does not depend on the count


# ---- rabitq_index.bin ----
def _index(n=5, dim=20, seed=1):
    rng = np.random.default_rng(seed)
    padded = next_power_of_two(dim)
    return RabitqIndexFile(dim, padded, rng.integers(0, 1 << 63, (padded + 63) // 64, dtype=np.uint64),
                           rng.integers(0, 256, (n, (padded + 7) // 8), dtype=np.uint8), rng.standard_normal(n).astype(np.float32))


def test_next_power_of_two():
    assert [next_power_of_two(d) for d in (1, 2, 3, 5, 8, 100, 128, 300, 768, 1536)] == [1, 2, 4, 8, 8, 128, 128, 512, 1024, 2048]


def test_codec_against_hand_assembled_bytes(tmp_path):
    """dim 3 -> padded 4, one code byte, one sign word; two rows."""
    raw = (b"\x51\x54\x42\x52" + b"\x02\x00\x00\x00" + b"\x03\x00\x00\x00" + b"\x04\x00\x00\x00" + b"\x02" + b"\x00" * 7 +
           b"\x01\x00\x00\x00" + b"\xef\xcd\xab\x89\x67\x45\x23\x01" + b"\x05\x0a" + b"\x00\x00\x80\x3f" + b"\x00\x00\x00\xc0")
    idx = RabitqIndexFile(3, 4, np.array([0x0123456789ABCDEF], np.uint64), np.array([[5], [10]], np.uint8),
                          np.array([1.0, -2.0], np.float32))
    path = tmp_path / "rabitq_index.bin"
    save_rabitq_index(path, idx)
    assert path.read_bytes() == raw
    back = load_rabitq_index(path)
    assert (back.dim, back.padded_dim, back.code_bytes, back.n_vectors) == (3, 4, 1, 2)
    assert back.sign_words.tolist() == [0x0123456789ABCDEF]
    assert back.codes.tolist() == [[5], [10]]
    assert back.norms.view(np.uint32).tolist() == [0x3F800000, 0xC0000000]


def test_codec_round_trip(tmp_path):
    idx = _index(n=37, dim=300)
    idx.norms[3] = np.nan
    path = tmp_path / "sub" / "rabitq_index.bin"
    save_rabitq_index(path, idx)
    raw = path.read_bytes()
    assert len(raw) == 28 + 8 * 8 + 37 * 64 + 37 * 4
    assert np.frombuffer(raw[:16], "<u4").tolist() == [RABITQ_MAGIC, RABITQ_VERSION, 300, 512]
    back = load_rabitq_index(path)
    assert np.array_equal(back.sign_words, idx.sign_words)
    assert np.array_equal(back.codes, idx.codes)
    assert np.array_equal(back.norms.view(np.uint32), idx.norms.view(np.uint32))


def _patched(tmp_path, raw, off, value, fmt="<u4"):
    b = bytearray(raw)
    v = np.array([value], fmt).tobytes()
    b[off:off + len(v)] = v
    p = tmp_path / "bad.bin"
    p.write_bytes(bytes(b))
    return p


def test_codec_rejections_and_version_1(tmp_path):
    idx = _index()
    path = tmp_path / "rabitq_index.bin"
    save_rabitq_index(path, idx)
    raw = path.read_bytes()
    cases = [(0, 0x1234, "Invalid RaBitQ magic bytes"), (4, 0, "Unsupported RaBitQ version: 0"), (4, 3, "Unsupported RaBitQ version: 3"),
             (8, 0, "Invalid RaBitQ dimensions"), (12, 16, "Invalid RaBitQ dimensions"), (12, 64, "Invalid RaBitQ dimensions"),
             (8, 33, "Invalid RaBitQ dimensions")]
    for off, val, msg in cases:
        with pytest.raises(IOError, match=msg):
            load_rabitq_index(_patched(tmp_path, raw, off, val))
    short = tmp_path / "short.bin"
    for cut in (len(raw) - 1, 30, 10, 3):
        short.write_bytes(raw[:cut])
        with pytest.raises(IOError, match="failed to fill whole buffer"):
            load_rabitq_index(short)
    # version 1 reads like version 2 from padded_dim 8 on ...
    v1 = load_rabitq_index(_patched(tmp_path, raw, 4, 1))
    assert np.array_equal(v1.codes, idx.codes) and np.array_equal(v1.norms.view(np.uint32), idx.norms.view(np.uint32))
    small = _index(n=3, dim=8)
    save_rabitq_index(path, small)
    assert load_rabitq_index(_patched(tmp_path, path.read_bytes(), 4, 1)).codes.shape == (3, 1)
    # ... and is refused below it, where it wrote zero-byte codes; version 2 reads those sizes
    for dim in (1, 3, 4):
        tiny = _index(n=3, dim=dim)
        save_rabitq_index(path, tiny)
        assert load_rabitq_index(path).codes.shape == (3, 1)
        with pytest.raises(IOError, match="RaBitQ v1 index is invalid for dimensions below 8"):
            load_rabitq_index(_patched(tmp_path, path.read_bytes(), 4, 1))
