"""GPU tests of the Sim(3) RANSAC (csrc/picp_sim3.hip; picp_sim3_batch, picp_sim3_fit_batch) against
tests/sim3_ref.py: the samples, every hypothesis' bits (the host build of the same closed form,
bin/sim3_check_plain), every inlier count (the float32 test restated in numpy, compared exactly),
and the winner, the refits and the result by the stated rules.  Tolerances are sim3_ref.tol
(1e-6 + 4 floor on the probe discrepancy); nothing here is tuned on the device's output.
"""
import os
import subprocess

import numpy as np
import pytest

import sim3_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

PLAIN = os.path.join(PKG, "bin", "sim3_check_plain")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _problem(n, seed, outlier_frac=0.5, noise=0.01):
    src, dst, _, _ = R.e2e_case(n, seed, outlier_frac, noise) if n else (np.zeros((0, 3), np.float32),) * 2 + (None, None)
    return src, dst


def _same_outputs(a, b):
    for x, y in zip(a, b):
        assert set(x) == set(y)
        for k in x:
            if isinstance(x[k], np.ndarray) and x[k].dtype == np.float32:
                np.testing.assert_array_equal(_bits(x[k]), _bits(y[k]), err_msg=k)
            elif isinstance(x[k], float):
                assert np.float32(x[k]).view(np.uint32) == np.float32(y[k]).view(np.uint32), k
            else:
                np.testing.assert_array_equal(x[k], y[k], err_msg=k)


# ---------------------------------------------------------------------------------------------
# 1. samples; the same bits on every call
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 64, 257])
@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFE1234])
def test_samples_equal_the_reference(native, H, seed):
    sizes = [4, 5, 63, 64, 65, 1025, 2049, 64]  # the last repeats problem 3's data at another position
    ps = [_problem(n, 7) for n in sizes]
    call = lambda: native.sim3_ransac_batch([p[0] for p in ps], [p[1] for p in ps], hypotheses=H, seed=seed,
                                            want_mask=True, debug=True)
    out = call()
    for i, n in enumerate(sizes):
        S = out[i]["samples"]
        np.testing.assert_array_equal(S, R.samples(seed, i, H, n))
        assert S.min() >= 0 and S.max() < n and all(len(set(t)) == 3 for t in S.tolist())
    if H > 1:
        assert not (out[3]["samples"] == out[7]["samples"]).all()  # the batch position is an input
    _same_outputs(out, call())


# ---------------------------------------------------------------------------------------------
# 2. hypothesis bits
# ---------------------------------------------------------------------------------------------
def _degenerate_problems():
    rng = np.random.default_rng(5)
    out = []
    # the fourth point copies the first, and so on: many triples hold one pair twice
    src, dst = _problem(8, 11, outlier_frac=0.0)
    src[4:], dst[4:] = src[:4], dst[:4]
    out.append((src, dst))
    src, dst = _problem(64, 12)
    src[3], dst[3] = src[0], dst[0]
    out.append((src, dst))
    # a collinear run: six of twelve points on one exact line (small integers: exact in float32)
    src, dst = _problem(12, 13, outlier_frac=0.0)
    k = np.arange(6, dtype=np.float32)[:, None]
    src[:6] = np.array([1, 2, 3], np.float32) + k * np.array([1, 2, 1], np.float32)
    dst[:6] = 2 * src[:6] + 1
    out.append((src, dst))
    # a NaN and an Inf coordinate
    src, dst = _problem(16, 14, outlier_frac=0.0)
    src[2, 1], dst[5, 0] = np.nan, np.inf
    out.append((src, dst))
    return out


@pytest.mark.parametrize("with_scale", [True, False])
def test_hypotheses_have_the_bits_of_the_host_build(native, with_scale, tmp_path):
    ps = _degenerate_problems()
    H = 256
    out = native.sim3_ransac_batch([p[0] for p in ps], [p[1] for p in ps], hypotheses=H, seed=3, with_scale=with_scale,
                                   debug=True)
    n_rejected = 0
    for i, ((src, dst), d) in enumerate(zip(ps, out)):
        np.testing.assert_array_equal(d["samples"], R.samples(3, i, H, len(src)))
        cases = [(src[idx], dst[idx], with_scale) for idx in d["samples"]]
        host, _ = R.run_check(PLAIN, cases, tmp_path, "hyp%d" % i)
        for h in range(H):
            ref = R.closed(cases[h][0], cases[h][1], with_scale)
            assert bool(d["hyp_valid"][h]) == (ref is not None) == (host[h] is not None), (i, h)
            if host[h] is None:
                assert (d["hyp_S"][h] == 0).all() and d["hyp_count"][h] == 0
                n_rejected += 1
            else:
                np.testing.assert_array_equal(_bits(d["hyp_S"][h]), _bits(host[h]), err_msg=str((i, h)))
        assert d["hyp_valid"].sum() > H // 8, i
    assert n_rejected > 50


# ---------------------------------------------------------------------------------------------
# 3. counts, winner, refits, result
# ---------------------------------------------------------------------------------------------
def _check_result(d, src, dst, thr, min_inliers, refits, with_scale=True):
    """Everything from the debug arrays by the stated rules.  Returns the winner."""
    H = len(d["hyp_valid"])
    for h in range(H):
        if d["hyp_valid"][h]:
            assert d["hyp_count"][h] == R.count(d["hyp_S"][h], src, dst, thr), h
        else:
            assert d["hyp_count"][h] == 0 and (d["hyp_S"][h] == 0).all()
    w = R.select(d["hyp_count"], d["hyp_valid"])
    chain, cur = [], (d["hyp_S"][w] if w is not None else None)
    for r in range(refits):
        ref = None
        if cur is not None:
            m = R.inlier_mask(cur, src, dst, thr)
            ref = R.closed(src[m], dst[m], with_scale)
        if ref is None:
            assert d["refit_count"][r] == -1 and (d["refit_S"][r] == 0).all(), r
            cur = None
        else:
            cur = d["refit_S"][r]
            assert R.discrepancy(ref, cur, src[m], dst[m]) <= R.tol(ref, src[m], dst[m]), r
            assert d["refit_count"][r] == R.count(cur, src, dst, thr), r
        chain.append((cur, int(d["refit_count"][r])))
    want = R.finish(d["hyp_S"][w] if w is not None else None, int(d["hyp_count"][w]) if w is not None else 0, chain,
                    src, dst, thr, min_inliers)
    assert d["found"] == want["found"] and d["inliers"] == want["inliers"]
    np.testing.assert_array_equal(_bits(d["S"]), _bits(want["S"]))
    np.testing.assert_array_equal(d["mask"], want["mask"])
    assert abs(d["scale"] - want["scale"]) <= 1e-5 * want["scale"]
    assert abs(d["rms"] - want["rms"]) <= 1e-5 * want["rms"] + 1e-12
    if want["found"]:
        assert int(d["mask"].sum()) == d["inliers"]
        if not with_scale:
            assert d["scale"] == 1.0
    else:
        assert d["scale"] == 1.0 and d["rms"] == 0.0
    return w


def _ragged():
    sizes = (4, 1025, 64, 0, 2049, 3)
    ps = [_problem(n, 20 + i) for i, n in enumerate(sizes)]
    # NaN and Inf points: never inliers, and a triple that holds one gives no transform
    for src, dst in ps:
        if len(src) >= 64:
            src[5, 0], src[17, 2], dst[33, 1], dst[40, 0] = np.nan, np.inf, np.nan, -np.inf
    return sizes, ps


@pytest.mark.parametrize("thr", [1e-4, 1.0])
def test_counts_winner_refits_and_result_on_a_ragged_batch(native, thr):
    sizes, ps = _ragged()
    H = 64
    out = native.sim3_ransac_batch([p[0] for p in ps], [p[1] for p in ps], threshold=thr, hypotheses=H, seed=9,
                                   refits=2, want_mask=True, debug=True)
    for i, ((src, dst), d) in enumerate(zip(ps, out)):
        w = _check_result(d, src, dst, thr, 4, 2)
        if sizes[i] < 4:
            assert not d["found"] and d["inliers"] == 0 and w is None and not d["hyp_valid"].any()
            assert (d["S"] == np.eye(4, dtype=np.float32)).all()
        if sizes[i] >= 64:
            bad = ~(np.isfinite(src).all(1) & np.isfinite(dst).all(1))
            assert bad.sum() == 4 and not d["mask"][bad].any()
            if thr == 1.0:
                assert d["found"] and d["inliers"] >= sizes[i] // 2 - 4


def test_counts_over_several_hypothesis_tiles_and_slices(native):
    """The score stage's walk beyond one tile of hypotheses: two whole tiles and a tile of 2 (130
    hypotheses with the kernel's tile of 64).  A: one problem of one pair more than a score block
    holds (1025): two score blocks, three slices of grid y, one tile each.  B: 400 problems of 5:
    400 score blocks, two slices; slice 0 walks tiles 0 and 2, slice 1 takes tile 1.  The tile
    sizes are the library's own."""
    HT, TILE = native.lib().picp_sim3_hyp_tile(), native.lib().picp_sim3_score_tile()
    H, thr = 2 * HT + 2, 0.01
    src, dst = _problem(TILE + 1, 80)
    d = native.sim3_ransac_batch([src], [dst], threshold=thr, hypotheses=H, seed=4, refits=2, want_mask=True,
                                 debug=True)[0]
    _check_result(d, src, dst, thr, 4, 2)
    assert d["hyp_valid"][:HT].any() and d["hyp_valid"][HT:2 * HT].any() and d["hyp_valid"][2 * HT:].any()
    ps = [_problem(5, 300 + i, outlier_frac=0.2) for i in range(400)]
    out = native.sim3_ransac_batch([p[0] for p in ps], [p[1] for p in ps], threshold=thr, hypotheses=H, seed=4,
                                   refits=2, want_mask=True, debug=True)
    for i, d in enumerate(out):
        assert d["hyp_count"].shape == (H,) and (d["hyp_count"] >= 0).all() and (d["hyp_count"] <= 5).all()
        assert (d["hyp_count"][d["hyp_valid"] == 0] == 0).all(), i
    for i in (0, 199, 399):
        np.testing.assert_array_equal(out[i]["samples"], R.samples(4, i, H, 5))
        _check_result(out[i], ps[i][0], ps[i][1], thr, 4, 2)
        assert out[i]["hyp_valid"][HT:2 * HT].any() and out[i]["hyp_valid"][2 * HT:].any()


def test_min_inliers_and_no_refits(native):
    src, dst = _problem(64, 30)
    for kw in (dict(min_inliers=60), dict(refits=0), dict(refits=8), dict(min_inliers=0, hypotheses=1)):
        prm = dict(threshold=0.01, hypotheses=32, seed=1, refits=2, min_inliers=4)
        prm.update(kw)
        d = native.sim3_ransac_batch([src], [dst], want_mask=True, debug=True, **prm)[0]
        _check_result(d, src, dst, prm["threshold"], prm["min_inliers"], prm["refits"])
        if kw.get("min_inliers") == 60:
            assert not d["found"] and 4 <= d["inliers"] < 60  # the best count seen


# ---------------------------------------------------------------------------------------------
# 4. robustness
# ---------------------------------------------------------------------------------------------
def test_robust_to_half_outliers(native):
    """50 % outliers uniform in the cloud's box, 1 cm noise, threshold 0.01 (10 cm).  The device
    holds every non-outlier (tests/test_sim3_cpu.py confirms the numpy reference does, on every
    seed: none dropped) and its result is within tol of Umeyama on the true inlier set plus the
    noise's effect: twice the distance the numpy reference pipeline itself shows from the
    constructed transform on that case (another random subset decides the estimate, hence the
    margin), 4.3e-4 of the extent at most (n = 64, seed 100)."""
    cases = [R.e2e_case(n, seed) for n, seed in R.E2E_CASES]
    out = native.sim3_ransac_batch([c[0] for c in cases], [c[1] for c in cases], threshold=R.E2E_THRESHOLD,
                                   hypotheses=256, refits=2, seed=5, want_mask=True)
    for (n, seed), (src, dst, S_true, outl), d in zip(R.E2E_CASES, cases, out):
        ref = R.ransac(src, dst, R.E2E_THRESHOLD, 256, 4, True, 2, seed, 0)
        assert ref["found"] and ref["mask"][~outl].all()
        noise = R.discrepancy(ref["S"], S_true, src[~outl], dst[~outl])
        U = R.closed(src[~outl], dst[~outl])
        got = R.discrepancy(d["S"], U, src[~outl], dst[~outl])
        print("n=%d seed=%d: device %.2e from Umeyama on the true inliers, reference's noise effect %.2e"
              % (n, seed, got, noise))
        assert d["found"] and d["mask"][~outl].all() and d["inliers"] >= n // 2
        assert got <= R.tol(U, src[~outl], dst[~outl]) + 2.0 * noise


# ---------------------------------------------------------------------------------------------
# 5. the refit stage alone, the rigid form, the facade
# ---------------------------------------------------------------------------------------------
def test_fit_batch_with_a_mask_has_the_refit_stage_bits(native):
    sizes = (64, 1025, 5)
    ps = [_problem(n, 40 + i) for i, n in enumerate(sizes)]
    ps[1][0][7, 1] = np.nan
    for ws in (True, False):
        out = native.sim3_ransac_batch([p[0] for p in ps], [p[1] for p in ps], threshold=0.01, hypotheses=64, seed=2,
                                       refits=1, with_scale=ws, debug=True)
        masks = []
        for (src, dst), d in zip(ps, out):
            w = R.select(d["hyp_count"], d["hyp_valid"])
            masks.append(R.inlier_mask(d["hyp_S"][w], src, dst, 0.01))
        fit = native.sim3_fit_batch([p[0] for p in ps], [p[1] for p in ps], masks, with_scale=ws)
        for d, f, m in zip(out, fit, masks):
            assert f["found"] == (d["refit_count"][0] >= 0)
            want = d["refit_S"][0] if f["found"] else np.eye(4, dtype=np.float32)
            np.testing.assert_array_equal(_bits(f["S"]), _bits(want))
        if ws:  # the data carry a scale: the rigid form finds few inliers, and may find no refit
            assert fit[0]["found"] and fit[1]["found"]


def test_fit_batch_without_a_mask_is_umeyama_of_the_finite_pairs(native):
    ps = [_problem(n, 50 + i, outlier_frac=0.0) for i, n in enumerate((500, 3, 2, 0, 1025))]
    ps[0][0][3, 0], ps[0][1][9, 2], ps[4][1][1000, 1] = np.nan, np.inf, np.nan
    fit = native.sim3_fit_batch([p[0] for p in ps], [p[1] for p in ps])
    for (src, dst), f in zip(ps, fit):
        ok = np.isfinite(src).all(1) & np.isfinite(dst).all(1) if len(src) else np.zeros(0, bool)
        ref = R.closed(src[ok], dst[ok])
        assert f["found"] == (ref is not None)
        if ref is None:
            assert (f["S"] == np.eye(4, dtype=np.float32)).all() and f["scale"] == 1.0 and f["rms"] == 0.0
            continue
        assert R.discrepancy(ref, f["S"], src[ok], dst[ok]) <= R.tol(ref, src[ok], dst[ok])
        assert abs(f["scale"] / R.scale_of(ref) - 1) < 1e-5
        rms = np.sqrt((np.linalg.norm(R.apply(ref, src[ok]) - dst[ok], axis=1) ** 2).mean())
        assert abs(f["rms"] - rms) <= 1e-3 * rms + 1e-6  # 1 cm of noise seen through float32 residuals
    assert fit[0]["found"] and fit[1]["found"] and not fit[2]["found"] and not fit[3]["found"] and fit[4]["found"]


def test_rigid_form_returns_scale_one_and_a_rotation(native):
    rng = np.random.default_rng(70)
    src = rng.uniform(-5, 5, (64, 3)).astype(np.float32)
    dst = (src.astype(np.float64) @ R.random_rotation(rng).T + rng.uniform(-5, 5, 3) + rng.normal(0, 0.01, (64, 3)))
    dst[::4] = rng.uniform(-5, 5, (16, 3))  # a quarter wrong
    dst = dst.astype(np.float32)
    d = native.sim3_ransac_batch([src], [dst], threshold=0.01, with_scale=False, debug=True)[0]
    assert d["found"] and d["inliers"] >= 48
    for h in np.flatnonzero(d["hyp_valid"]):
        M = d["hyp_S"][h][:3, :3].astype(np.float64)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-6
    # the least-squares fit of data that do carry a scale (1.3): still c = 1 exactly
    src2, dst2, _ = next(iter(R.family("rigid", 1)))
    for d in (d, native.sim3_fit_batch([src2], [dst2], with_scale=False)[0]):
        assert d["found"] and d["scale"] == 1.0
        M = d["S"][:3, :3].astype(np.float64)
        assert np.abs(M @ M.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(M) > 0


def test_facade_reproduces_the_python_call(native, tmp_path):
    src, dst = _problem(500, 60)
    prm = dict(threshold=0.01, hypotheses=128, min_inliers=10, with_scale=True, refits=2, seed=77)
    d = native.sim3_ransac_batch([src], [dst], **prm)[0]
    path = os.path.join(str(tmp_path), "problem.txt")
    with open(path, "w") as f:
        f.write("%s %d %d %d %d %d\n%d\n" % (float(np.float32(prm["threshold"])).hex(), prm["hypotheses"],
                                              prm["min_inliers"], 1, prm["refits"], prm["seed"], len(src)))
        for p, q in zip(src, dst):
            f.write(" ".join(float(v).hex() for v in list(p) + list(q)) + "\n")
    out = subprocess.run([os.path.join(PKG, "bin", "sim3_main"), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    tok = out.stdout.split()
    assert tok[0] == "align" and int(tok[1]) == int(d["found"]) == 1 and int(tok[2]) == d["inliers"]
    assert int(tok[3], 16) == int(np.float32(d["scale"]).view(np.uint32))
    np.testing.assert_array_equal(np.array([int(t, 16) for t in tok[4:20]], np.uint32), _bits(d["S"].T.reshape(16)))
