"""The generators of tests/predict_common.py against a numpy model of the SQ8 quantiser and of the predicted threshold (unquantised
queries): they must produce what tests/test_gpu_predict_verify.py needs — a planted row of the exact top-k whose coarse score lies under
the threshold while k or more keys arrive, a threshold that admits more keys than the candidate buffer holds, more than keep_max equal
survivors under a valid threshold.  If the quantiser, z or a constant changes, this reports the lost coverage instead of the GPU test
going quietly soft.  No GPU; the model describes the inputs, it is no expectation of a search."""
import math
import re
from pathlib import Path

import numpy as np

import predict_common as P

f32 = np.float32
CSRC = Path(__file__).resolve().parent.parent / "lynsedb_amd" / "csrc"


def test_constants_follow_the_sources():
    kern, host = (CSRC / "kernels.h").read_text(), (CSRC / "lynse_hip.hip").read_text()
    m = re.search(r"constexpr uint32_t PRED_MISS = (\d+)u, PRED_NONE = (\d+)u;", kern)
    assert (int(m.group(1)), int(m.group(2))) == (P.PRED_MISS, P.PRED_NONE)
    assert "a.s.overflow[q] |= PRED_MISS" in kern and "a.s.overflow[q] |= PRED_NONE" in kern
    keep = re.findall(r"sa\.keep_max = w\.cap / (\d+);", host)
    assert keep and all(P.CAP // int(d) == P.KEEP_MAX for d in keep), keep
    assert int(re.search(r'env_int\("LYNSE_HIP_PREDICT_C", (\d+)\)', host).group(1)) == P.PREDICT_C_DEFAULT
    assert "sorted_path = keep > a.keep_max;" in kern      # the exit the duplicates case is about


def fitted(data):
    mins, scales = P.sq8_fit_model(data)
    codes = P.sq8_codes(data, mins, scales)
    return mins, scales, codes, P.code_stats(codes)


def test_quantiser_model_on_a_small_case():
    data = np.array([[0.0, -1.0, 5.0], [1.0, 1.0, 5.0], [0.5, 0.0, 5.0], [0.001, 0.999, 5.0]], f32)
    mins, scales = P.sq8_fit_model(data)
    assert mins.tolist() == [0.0, -1.0, 5.0] and scales.tolist() == [255.0, 127.5, 0.0]
    codes = P.sq8_codes(data, mins, scales)
    assert codes[:, 0].tolist() == [-128.0, 127.0, 0.0, -128.0]      # 127.5 rounds away from zero: code 128; 0.255 -> 0
    assert codes[:, 1].tolist() == [-128.0, 127.0, 0.0, 127.0] and codes[:, 2].tolist() == [-128.0] * 4
    z = P.z_numpy(70_000, 10)
    assert abs(70_000 * 0.5 * math.erfc(z / math.sqrt(2.0)) - 10) < 1e-6 and P.z_numpy(100, 50) == 0.0


def test_band_planting_gives_k_keys_and_a_top_k_row_under_the_threshold(capsys):
    """The margins asserted are what the device run needs, not what the model happened to give: the query image's rounding moves a coarse
    score by about s_q ||c|| / sqrt(12) = 0.15 here (s_q = max |w| / 127 ~ 1.1e-3, ||c|| ~ 16 * 29), so a victim 0.5 under the threshold
    and helpers 0.5 above it stay there at three sigma, and a threshold shift under 0.1 leaves the 0.8 / 1.0 of the construction standing."""
    data, queries, src = P.band_inputs()
    n, k = len(data), P.BAND_K
    mins, scales, codes, (mu, var) = fitted(data)
    thr = P.model_threshold(queries, mins, scales, mu, var, n, 1, k)
    cnt = (P.model_coarse(queries, mins, scales, codes) >= thr[:, None]).sum(axis=1)
    picks = P.pick_band_queries(cnt)
    assert len(picks) == P.BAND_PICKS, cnt
    planted, victims, helpers = P.plant_band(np.random.default_rng(2742), data, queries, thr, picks, k, avoid=src)
    mins2, scales2, codes2, (mu2, var2) = fitted(planted)
    assert np.array_equal(mins2.view(np.uint32), mins.view(np.uint32)) and np.array_equal(scales2.view(np.uint32), scales.view(np.uint32))
    thr2 = P.model_threshold(queries, mins2, scales2, mu2, var2, n, 1, k)
    shift = float(np.abs(thr2 - thr).max())
    assert shift < 0.1, shift
    coarse = P.model_coarse(queries[picks], mins2, scales2, codes2)
    exact = queries[picks].astype(np.float64) @ planted.astype(np.float64).T
    good, lines = 0, []
    for i, qi in enumerate(picks):
        at = int((coarse[i] >= thr2[qi]).sum())
        above = exact[i, victims[i]] - thr2[qi]
        below = thr2[qi] - coarse[i, victims[i]]
        rank = int((exact[i] > exact[i, victims[i]]).sum())
        helpers_in = bool((coarse[i, helpers[i]] >= thr2[qi] + 0.5).all())
        ok = k <= at <= k + 2 and 1.0 <= above <= 3.0 and 0.5 <= below <= 1.6 and rank < k and helpers_in
        good += ok
        lines.append(f"query {qi}: {cnt[qi]} -> {at} rows at or above thr, victim exact +{above:.2f}, coarse -{below:.2f}, exact rank {rank}{'' if ok else '  (does not count)'}")
    with capsys.disabled():
        print(f"\nband: threshold shift {shift:.3f}; " + "; ".join(lines))
    assert good >= 6, lines


def test_too_low_a_threshold_overflows_the_candidate_buffer():
    data, queries = P.overflow_inputs()
    n, k = len(data), 10
    assert n >= 8 * P.OVER_C * k and n >= 65536                       # predict_wanted
    mins, scales, codes, (mu, var) = fitted(data)
    thr = P.model_threshold(queries, mins, scales, mu, var, n, P.OVER_C, k)
    cnt = (P.model_coarse(queries, mins, scales, codes) >= thr[:, None]).sum(axis=1)
    print(f"overflow: {int(cnt.min())}..{int(cnt.max())} rows at or above the threshold (cap {P.CAP})")
    assert cnt.min() >= 18_000 > P.CAP, (int(cnt.min()), int(cnt.max()))


def test_duplicates_pass_keep_max_under_a_valid_threshold():
    data, ids, queries = P.duplicate_inputs()
    n, k = len(data), 10
    assert len(ids) == P.DUP_COPIES and P.KEEP_MAX < P.DUP_COPIES < P.CAP
    assert (data[ids] == data[ids[0]]).all() and len(queries) == P.DUP_NEAR + P.DUP_FAR
    mins, scales, codes, (mu, var) = fitted(data)
    thr = P.model_threshold(queries, mins, scales, mu, var, n, P.PREDICT_C_DEFAULT, k)
    cnt = (P.model_coarse(queries, mins, scales, codes) >= thr[:, None]).sum(axis=1)
    near, far = cnt[:P.DUP_NEAR], cnt[P.DUP_NEAR:]
    kth = np.sort(queries[:P.DUP_NEAR].astype(np.float64) @ data.astype(np.float64).T, axis=1)[:, -k]
    print(f"duplicates: near {int(near.min())}..{int(near.max())}, far {int(far.min())}..{int(far.max())}, k-th exact score above thr by >= {float((kth - thr[:P.DUP_NEAR]).min()):.0f}")
    assert near.min() >= P.DUP_COPIES and near.max() <= 12_000, (int(near.min()), int(near.max()))
    assert far.min() >= 3 * k and far.max() <= P.CAP // 3, (int(far.min()), int(far.max()))
