"""The SQ7 quantiser and its certified bound (k_sq8_quantize with sq7 = 1, k_i8c_prep_queries with sq7 = 1) restated in
numpy: codes c_d = rint((v_d - min_d) * scale7_d) in [0, 127], scale7_d = 127 / (max_d - min_d) (0 for a constant dimension), stored without
an offset; per query w = q / scale7, s_q = max |w| / 127, u = rint(w / s_q), eta = w / s_q - u.  The identity

    q . v = sum q_d min_d + s_q sum u_d c_d + s_q sum eta_d c_d + sum w_d eps_d

with the mid code's share of the query-residual term moved into the constant, B_q = sum q_d min_d + 64 s_q sum eta_d (eta is known
exactly per query), gives |B_q + s_q u.c - q.v| <= E with E = min(Hoelder, Cauchy-Schwarz) of s_q sum eta_d (c_d - 64) and sum w_d eps_d
(+ the f32 evaluation terms) x 1.02, from the row statistics the quantiser collects (max sum |c - 64|, max sum (c - 64)^2, max sum eps^2
including the f32 evaluation error of the residual).  Checked in f64 for every (row, query) pair of random and adversarial rows.  No GPU."""
import numpy as np
import pytest

f32 = np.float32


def sq7_fit(data):
    mn, mx = data.min(axis=0), data.max(axis=0)
    rng_ = (mx - mn).astype(f32)
    scale = np.where(rng_ > f32(1e-30), f32(127.0) / np.where(rng_ > 0, rng_, f32(1)), f32(0)).astype(f32)
    return mn.astype(f32), scale


def sq7_quantise(data, mn, scale):
    t = ((data - mn).astype(f32) * scale).astype(f32)                     # the two f32 roundings of the kernel
    code = np.clip(np.sign(t) * np.floor(np.abs(t) + f32(0.5)), 0, 127).astype(np.int64)   # roundf: half away from zero
    e = (t - code.astype(f32)).astype(np.float64)
    D = data.shape[1]
    cc = code - 64
    a1 = int(np.abs(cc).sum(axis=1).max())
    a2sq = int((cc * cc).sum(axis=1).max())
    e2 = ((e * e).sum(axis=1) + 1.22e-4 * np.abs(e).sum(axis=1) + D * 3.8e-9) * 1.00002
    return code, a1, a2sq, float(e2.max())


def sq7_prep(q, mn, scale, a1, a2sq, eps2, vmax):
    q = q.astype(np.float64)
    sc = scale.astype(np.float64)
    w = np.where(sc > 0, q / np.where(sc > 0, sc, 1.0), 0.0)
    wmax = np.abs(w).max()
    sq = f32(1.0)
    if 0.0 < wmax < 1e30:
        sq = f32(wmax / 127.0)
        if float(sq) * 127.0 < wmax:
            sq = np.nextafter(sq, f32(np.inf))
    t = w / float(sq)
    u = np.clip(np.rint(t), -127, 127)
    eta = t - u
    bq = float((q * mn.astype(np.float64)).sum()) + 64.0 * float(sq) * float(eta.sum())   # no 128 * sum w term: the codes carry no offset
    tq = min(0.5001 * float(sq) * a1, 1.0002 * float(sq) * np.sqrt((eta * eta).sum()) * np.sqrt(a2sq))
    tr = min(0.5001 * np.abs(w).sum(), 1.0002 * np.sqrt((w * w).sum()) * np.sqrt(eps2))
    s2 = float((q * q).sum())
    gam = 10.0 * len(q) * 5.9604645e-8
    E = (tr + tq + 2.5e-7 * (abs(bq) + s2 + 127.0 * float(sq) * (a1 + 64.0 * len(q))) + gam * np.sqrt(s2) * vmax) * 1.02
    return u.astype(np.int64), float(sq), bq, E


def cases():
    rng = np.random.default_rng(77)
    n, D = 2000, 64
    uniform = rng.random((n, D), dtype=f32)
    gauss = rng.standard_normal((n, D)).astype(f32)
    # adversarial: rows a hair below the rounding boundary of every code, all on one side (eps = +0.4999), with constant dimensions,
    # a dimension of tiny range, rows at both ends of every range, and an outlier that collapses one scale
    step = f32(1.0 / 64.0)
    adv = ((rng.integers(0, 127, (n, D)) + 0.4999) * step).astype(f32)
    adv[0], adv[1] = 0.0, 127.0 * step
    adv[:, 5] = f32(3.25)
    adv[:, 9] = (5.0 + 1e-6 * rng.random(n)).astype(f32)
    adv[7, 11] = f32(1.0e4)
    q_pos = np.abs(rng.standard_normal((40, D))).astype(f32)
    q_mixed = rng.standard_normal((40, D)).astype(f32)
    q_aligned = np.tile((rng.integers(20, 127, D) * 2.0 ** -10).astype(f32), (4, 1))      # exactly representable images: eta = 0, all of E is the row term
    queries = np.vstack([q_pos, q_mixed, q_aligned])
    return {"uniform": (uniform, queries), "gauss": (gauss, queries), "adversarial": (adv, queries)}


@pytest.mark.parametrize("name", ["uniform", "gauss", "adversarial"])
def test_the_sq7_bound_holds_for_every_pair(name):
    data, queries = cases()[name]
    mn, scale = sq7_fit(data)
    code, a1, a2sq, eps2 = sq7_quantise(data, mn, scale)
    assert code.min() >= 0 and code.max() <= 127
    const = scale == 0
    assert np.all(code[:, const] == 0)                                     # constant dimensions: scale 0, exact through B_q
    vmax = float(np.sqrt((data.astype(np.float64) ** 2).sum(axis=1)).max())
    exact = queries.astype(np.float64) @ data.astype(np.float64).T
    worst = 0.0
    for qi, q in enumerate(queries):
        u, sq, bq, E = sq7_prep(q, mn, scale, a1, a2sq, eps2, vmax)
        dot = code @ u
        assert np.abs(dot).max() < 2 ** 29                                 # the 31-step bisection of the integer threshold stays valid
        coarse = bq + sq * dot.astype(np.float64)
        err = np.abs(coarse - exact[qi])
        worst = max(worst, float((err / E).max()))
        assert np.all(err <= E), (name, qi, float(err.max()), E)
    print(f"SQ7 bound, {name}: max |coarse - exact| / E = {worst:.4f}")


def test_non_negative_operands_give_non_negative_products():
    """What the mode is for: with non-negative queries every code, every image byte and so every MAC of the scan is non-negative."""
    data, queries = cases()["uniform"]
    mn, scale = sq7_fit(data)
    code, a1, a2sq, eps2 = sq7_quantise(data, mn, scale)
    u, _, _, _ = sq7_prep(queries[0], mn, scale, a1, a2sq, eps2, 1.0)
    assert queries[0].min() >= 0 and u.min() >= 0 and code.min() >= 0
