"""TEST INFRASTRUCTURE for FLAT-*-POLARVEC<b> (tests/test_polarvec_modes.py, tests/test_gpu_flat_polarvec.py): the restatement of
PolarVecIndex (src/storage/polarvec_mmap.rs) — the SmallRng sign words in Python, fit / encode / packing / query tables / table score
in tests/polarvec_ref/polarvec_ref.c — and the comparisons.  Exact distances come from the oracle's exported single-pair kernel, both
canonical (score, row) cuts are taken in numpy.  No tolerances anywhere: codes, f32 bits (a NaN as a NaN), ids."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np

IP, L2, COS = 0, 1, 2
NAME = {IP: "ip", L2: "l2", COS: "cosine"}
f32 = np.float32
HERE = Path(__file__).resolve().parent
_vp = C.c_void_p
M64 = (1 << 64) - 1
OVERSAMPLE = 20


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def compile_ref(tmp_dir):
    """polarvec_ref.c as a shared library in tmp_dir, its entry points typed"""
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if shutil.which(c)), None)
    assert cc, "no C compiler for tests/polarvec_ref/polarvec_ref.c"
    so = Path(tmp_dir) / "libpolarvec_ref.so"
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-o", str(so),
                    str(HERE / "polarvec_ref" / "polarvec_ref.c"), "-lm"], check=True)
    lib = C.CDLL(str(so))
    z = C.c_size_t
    lib.plr_raw_code.argtypes, lib.plr_raw_code.restype = [C.c_float] * 3, C.c_float
    lib.plr_code.argtypes, lib.plr_code.restype = [C.c_float, C.c_float, C.c_float, C.c_uint], C.c_uint
    lib.plr_pack.argtypes, lib.plr_pack.restype = [_vp, z, C.c_uint, z], None
    lib.plr_unpack.argtypes, lib.plr_unpack.restype = [_vp, z, z], C.c_uint
    lib.plr_fit.argtypes = [_vp, z, z, z, _vp, z, _vp, _vp]
    lib.plr_encode.argtypes = [_vp, z, z, z, _vp, z, _vp, _vp, _vp, _vp, _vp]
    lib.plr_query.argtypes = [_vp, z, z, C.c_int, _vp, z, _vp, _vp, _vp]
    lib.plr_scores.argtypes = [_vp, z, z, z, _vp, _vp, _vp, _vp]
    lib.plr_dists.argtypes = [_vp, _vp, z, _vp, z, C.c_int, _vp, _vp]
    for fn in (lib.plr_fit, lib.plr_encode, lib.plr_query, lib.plr_scores, lib.plr_dists):
        fn.restype = None
    return lib


def sign_words(count, seed=42):
    """the first `count` next_u64() of SmallRng::seed_from_u64(seed): xoshiro256++ whose state is four SplitMix64 outputs"""
    s, st = [], seed
    for _ in range(4):
        st = (st + 0x9E3779B97F4A7C15) & M64
        z = st
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        s.append(z ^ (z >> 31))
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & M64
    out = []
    for _ in range(count):
        out.append((rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64)
        t = (s[1] << 17) & M64
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t
        s[3] = rotl(s[3], 45)
    return np.array(out, np.uint64)


def pow2(dim):
    return 1 << max(dim - 1, 0).bit_length()


def bytes_per_vec(dim, bits):
    return (pow2(dim) * bits + 7) // 8


class Enc:
    """what a PolarVecIndex holds: bits, signs, dim_mins, dim_scales, codes and the correction array of the metric it was built for"""

    def __init__(self, bits, signs, mins, scales, codes, residual, inv):
        self.bits, self.signs, self.mins, self.scales, self.codes, self.residual, self.inv = bits, signs, mins, scales, codes, residual, inv


def ref_encode(lib, data, bits, metric, signs=None, fit=None):
    """build_for_metric; `fit` = (dim_mins, dim_scales) skips the fit"""
    data = np.ascontiguousarray(data, f32)
    n, dim = data.shape
    P = pow2(dim)
    signs = sign_words((P + 63) // 64) if signs is None else signs
    if fit is None:
        mins, scales = np.zeros(P, f32), np.zeros(P, f32)
        lib.plr_fit(_p(data), n, dim, bits, _p(signs), signs.size, _p(mins), _p(scales))
    else:
        mins, scales = fit
    codes = np.zeros((n, bytes_per_vec(dim, bits)), np.uint8)
    residual = np.zeros(n, f32) if metric == L2 else None
    inv = np.zeros(n, f32) if metric == COS else None
    lib.plr_encode(_p(data), n, dim, bits, _p(signs), signs.size, _p(mins), _p(scales), _p(codes), _p(residual), _p(inv))
    return Enc(bits, signs, mins, scales, codes, residual, inv)


def cut(scores, asc, N, rows):
    """positions of the N best by the canonical (score, row) key: NaN ranks last (as +-inf), -0 == +0.  A partition first keeps
    every key up to the N-th smallest (ties at the cut included), so the lexsort that decides them sees all of them."""
    s = np.where(np.isnan(scores), np.inf if asc else -np.inf, scores).astype(f32) + f32(0.0)
    key = s if asc else -s
    cand = np.arange(key.size)
    if 0 < N < key.size:
        cand = np.nonzero(key <= np.partition(key, N - 1)[N - 1])[0]
    order = cand[np.lexsort((rows[cand], key[cand]))]
    return order[:N], s


def ref_scores(lib, enc, dim, query, metric):
    """the table score of every indexed row for one query"""
    n = enc.codes.shape[0]
    lut = np.zeros(pow2(dim) << enc.bits, f32)
    q = np.ascontiguousarray(query, f32)
    lib.plr_query(_p(q), dim, enc.bits, metric, _p(enc.signs), enc.signs.size, _p(enc.mins), _p(enc.scales), _p(lut))
    sc = np.zeros(n, f32)
    lib.plr_scores(_p(enc.codes), n, dim, enc.bits, _p(lut), _p(enc.residual if metric == L2 else None),
                   _p(enc.inv if metric == COS else None), _p(sc))
    return sc


def ref_search_ks(lib, dist, for_every_query, data, enc, queries, ks, metric, oversample=OVERSAMPLE, pools=None):
    """{k: per query (rows, exact distances)} for every k of `ks`, the table scores of a query computed once; `pools`, a dict, receives
    {k: each query's pool}"""
    n_plv, dim = enc.codes.shape[0], data.shape[1]
    asc = metric != IP
    data = np.ascontiguousarray(data, f32)

    def one(qi):
        q = np.ascontiguousarray(queries[qi], f32)
        sc = ref_scores(lib, enc, dim, q, metric)
        out = {}
        for k in ks:
            kk = min(k, n_plv)
            pool, _ = cut(sc, asc, min(kk * oversample, n_plv), np.arange(n_plv))
            pool = np.ascontiguousarray(pool, np.uint64)
            d = np.zeros(pool.size, f32)
            lib.plr_dists(_p(q), _p(data), dim, _p(pool), pool.size, metric, dist, _p(d))
            sel, s = cut(d, asc, kk, pool)
            out[k] = (pool[sel].astype(np.uint64), s[sel], pool)
        return out

    res = for_every_query(one, queries.shape[0])
    if pools is not None:
        pools.update({k: [r[k][2] for r in res] for k in ks})
    return {k: [(r[k][0], r[k][1]) for r in res] for k in ks}


def ref_search(lib, dist, for_every_query, data, enc, queries, k, metric, oversample=OVERSAMPLE):
    return ref_search_ks(lib, dist, for_every_query, data, enc, queries, [k], metric, oversample)[k]


def check_search(got, exp):
    rows, dists, counts = got
    assert counts.shape[0] == len(exp)
    for qi, (e_r, e_d) in enumerate(exp):
        c = int(counts[qi])
        assert c == e_r.size, (qi, c, e_r.size)
        assert np.array_equal(rows[qi, :c], e_r), (qi, rows[qi, :c][:10], e_r[:10])
        assert np.array_equal(dists[qi, :c].view(np.uint32), e_d.view(np.uint32)), (qi, dists[qi, :c][:10], e_d[:10])


def bits_of(a):
    """f32 bits with every NaN mapped to one pattern (neither IEEE 754 nor Rust pins a NaN's sign and payload)"""
    return np.where(np.isnan(a), f32(np.nan), a).astype(f32).view(np.uint32)


def check_index(p, enc, dim):
    """a FlatIndex.polarvec_params() dict against the restatement"""
    P = pow2(dim)
    flags = (1 if enc.residual is not None else 0) | (2 if enc.inv is not None else 0)
    assert (p["dim"], p["padded_dim"], p["bits"], p["bytes_per_vec"], p["flags"], p["n"]) == \
        (dim, P, enc.bits, bytes_per_vec(dim, enc.bits), flags, enc.codes.shape[0])
    assert np.array_equal(p["sign_words"], enc.signs)
    assert np.array_equal(bits_of(p["dim_mins"]), bits_of(enc.mins)), (p["dim_mins"][:8], enc.mins[:8])
    assert np.array_equal(bits_of(p["dim_scales"]), bits_of(enc.scales)), (p["dim_scales"][:8], enc.scales[:8])
    bad = np.nonzero((p["codes"] != enc.codes).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], p["codes"][bad[:1]], enc.codes[bad[:1]])
    for name, e in (("residual_sq", enc.residual), ("inv_v_hat_norms", enc.inv)):
        if e is None:
            assert p[name] is None
        else:
            assert np.array_equal(bits_of(p[name]), bits_of(e)), (name, p[name][:8], e[:8])
