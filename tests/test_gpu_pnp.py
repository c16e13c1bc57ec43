"""GPU tests of the P3P RANSAC (csrc/picp_pnp.hip; picp_pnp_batch, picp_relocalize) against
tests/pnp_ref.py (samples, selection rule) and the CPU oracle (every inlier count: the oracle's own
linearize at the device's float32 pose, so counts are compared exactly).
"""
import os
import subprocess

import numpy as np
import pytest

import pnp_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

ROWS, COLS = 480, 640
K_SKEW = np.array([[183.0, 0.75, 318.5], [0.0, 176.5, 243.25], [0.0, 0.0, 1.0]], np.float32)
FAR = (1.0, 2.0)  # rad and m per axis: the prior relocalize must not need


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _problem(n, seed, K=None, **kw):
    """synth.make_problem; with another K the pixels are mapped so the frame is consistent with it."""
    from picp_amd import synth
    p = synth.make_problem(n, seed=seed, **kw)
    if K is not None:
        M = np.asarray(K, np.float64) @ np.linalg.inv(synth.K_REF)
        h = (M @ np.column_stack([p["uv"].astype(np.float64), np.ones(n)]).T).T
        p["uv"] = np.ascontiguousarray((h[:, :2] / h[:, 2:3]).astype(np.float32))
        p["K"] = np.asarray(K, np.float32)
    return p


def _hard_frame(n, seed):
    """A frame where a third of the points are behind the camera or project far out of the image
    at the true pose (and at most hypotheses)."""
    from picp_amd import synth
    p = _problem(n, seed, outlier_frac=0.5, pixel_noise=0.5)
    rng = np.random.default_rng(seed)
    T = p["T_gt"].astype(np.float64)
    idx = rng.choice(n, n // 3, replace=False)
    cam = np.column_stack([rng.uniform(-3, 3, len(idx)), rng.uniform(-3, 3, len(idx)), rng.uniform(-4, -0.5, len(idx))])
    cam[::2, 2] = rng.uniform(0.05, 0.3, len(cam[::2]))  # in front, but far outside the image
    cam[::2, 0] = rng.choice([-1, 1], len(cam[::2])) * rng.uniform(2, 5, len(cam[::2]))
    p["xyz"][idx] = ((cam - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    return p


def _check_counts(O, d, p, K, thr):
    """hyp_count of every valid (hypothesis, root) equals the oracle's n_in at hyp_T; 0 elsewhere."""
    H = len(d["n_roots"])
    seen = 0
    for h in range(H):
        nr = int(d["n_roots"][h])
        assert 0 <= nr <= 4
        assert (d["hyp_count"][h][nr:] == 0).all() and (d["hyp_T"][h][nr:] == 0).all()
        for r in range(nr):
            assert d["hyp_count"][h][r] == R.count(O, d["hyp_T"][h][r], K, ROWS, COLS, p["xyz"], p["uv"], thr), (h, r)
            seen += 1
    return seen


def _check_winner(native, d, p, K, thr, min_inliers=4):
    """T_out, inliers, found and mask follow from the debug arrays by the stated rule."""
    w = R.select(d["hyp_count"], d["n_roots"])
    n = len(p["xyz"])
    if w is None or n < 4 or w[2] < min_inliers:
        assert not d["found"] and (d["T"] == np.eye(4, dtype=np.float32)).all()
        assert d["inliers"] == (w[2] if w else 0) and not d["mask"].any()
        return None
    assert d["found"] and d["inliers"] == w[2]
    np.testing.assert_array_equal(_bits(d["T"]), _bits(d["hyp_T"][w[0]][w[1]]))
    b = native.Batch([n], rows=ROWS, cols=COLS, K=K)
    b.set_data(p["xyz"], p["uv"])
    state = b.classify(thr, poses=d["T"][None], want_chi2=False)["state"]
    b.close()
    np.testing.assert_array_equal(d["mask"], state == native.CORR_INLIER)
    assert int(d["mask"].sum()) == d["inliers"]
    return w


# ---------------------------------------------------------------------------------------------
# 1. samples
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 64, 257])
@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFE1234])
def test_samples_equal_the_reference(native, H, seed):
    sizes = [4, 5, 63, 64, 65, 2049, 64]  # the last repeats problem 3's data at another position
    ps = [_problem(n, 7) for n in sizes]
    out = native.pnp_ransac_batch([p["xyz"] for p in ps], [p["uv"] for p in ps], hypotheses=H, seed=seed, debug=True)
    for i, n in enumerate(sizes):
        S = out[i]["samples"]
        np.testing.assert_array_equal(S, R.samples(seed, i, H, n))
        assert S.min() >= 0 and S.max() < n and all(len(set(t)) == 3 for t in S.tolist())
    if H > 1:
        assert not (out[3]["samples"] == out[6]["samples"]).all()  # the batch position is an input
    again = native.pnp_ransac_batch([p["xyz"] for p in ps], [p["uv"] for p in ps], hypotheses=H, seed=seed, debug=True)
    for a, b in zip(out, again):
        for k in ("samples", "n_roots", "hyp_count"):
            np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(_bits(a["hyp_T"]), _bits(b["hyp_T"]))
        np.testing.assert_array_equal(_bits(a["T"]), _bits(b["T"]))


# ---------------------------------------------------------------------------------------------
# 2. the P3P solver
# ---------------------------------------------------------------------------------------------
def test_solver_on_noiseless_triples(native):
    from picp_amd import synth
    p = _problem(64, 64)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], hypotheses=256, debug=True)[0]
    hit, worst_px = 0, 0.0
    for h in range(256):
        nr = int(d["n_roots"][h])
        idx = d["samples"][h]
        errs = []
        for r in range(nr):
            T = d["hyp_T"][h][r]
            assert np.isfinite(T).all() and (T[3] == [0, 0, 0, 1]).all()
            worst_px = max(worst_px, R.reproj_err(T, p["K"], p["xyz"][idx], p["uv"][idx]).max())
            errs.append(synth.se3_log_norm(T, p["T_gt"]))
        hit += bool(errs) and min(errs) < 1e-4
    print("hypotheses with a root within 1e-4 of T_gt: %d of 256; worst own-point reprojection %.2e px" % (hit, worst_px))
    assert worst_px < 1e-2
    assert hit >= 0.99 * 256


def test_solver_on_degenerate_samples(native):
    base = _problem(8, 3)
    line = (np.array([1.0, 2.0, 3.0]) + np.outer(np.arange(8.0), [0.5, -0.25, 0.75])).astype(np.float32)  # exact
    twin = base["xyz"][:4].copy()
    twin[1] = twin[0]
    nan = base["xyz"].copy()
    nan[2, 1] = np.nan
    nanuv = base["uv"].copy()
    nanuv[5, 0] = np.nan
    same = np.repeat(base["xyz"][:1], 6, 0)
    cases = [(line, base["uv"]), (twin, base["uv"][:4]), (nan, base["uv"]), (base["xyz"], nanuv), (same, base["uv"][:6])]
    out = native.pnp_ransac_batch([c[0] for c in cases], [c[1] for c in cases], hypotheses=64, debug=True, want_mask=True)
    for i, d in enumerate(out):
        for h in range(64):
            nr = int(d["n_roots"][h])
            assert np.isfinite(d["hyp_T"][h][:nr]).all()
            idx = d["samples"][h]
            bad = not (np.isfinite(cases[i][0][idx]).all() and np.isfinite(cases[i][1][idx]).all())
            if i in (0, 4) or bad or (i == 1 and {0, 1} <= set(idx.tolist())):
                assert nr == 0, (i, h)
        assert np.isfinite(d["T"]).all()
    assert not out[0]["found"] and not out[4]["found"] and out[0]["inliers"] == 0


# ---------------------------------------------------------------------------------------------
# 3. scoring is the PICP gate, exactly; 4. selection and mask
# ---------------------------------------------------------------------------------------------
SCORE_CASES = [("n%d_thr%d" % (n, thr), n, None, float(thr)) for n in (5, 64, 65, 500, 2049) for thr in (9, 3000)]
SCORE_CASES += [("skew_thr9", 500, K_SKEW, 9.0), ("skew_thr3000", 65, K_SKEW, 3000.0),
                ("hard_thr9", 500, "hard", 9.0), ("hard_thr3000", 500, "hard", 3000.0)]


@pytest.mark.parametrize("name,n,kind,thr", SCORE_CASES, ids=[c[0] for c in SCORE_CASES])
def test_counts_are_the_oracle_gate_and_the_winner_follows(native, oracle, name, n, kind, thr):
    if isinstance(kind, str):
        p, K = _hard_frame(n, 11), np.asarray(native.K_REF)
    else:
        K = native.K_REF if kind is None else kind
        p = _problem(n, 11 + n, K=kind, outlier_frac=0.5, pixel_noise=0.5)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], K=K, threshold=thr, hypotheses=64, debug=True, want_mask=True)[0]
    seen = _check_counts(oracle, d, p, K, thr)
    # not vacuous: a triple of three non-outliers has a root (about one triple in eight; one that
    # holds a random pixel usually has no solution with positive depths)
    assert seen >= 4
    if isinstance(kind, str):
        T = d["hyp_T"][0][0].astype(np.float64)
        cam = p["xyz"] @ T[:3, :3].T + T[:3, 3]
        assert (cam[:, 2] <= 0).any()  # the gate's z test is exercised
    w = _check_winner(native, d, p, K, thr)
    print("%s: %d poses checked, winner %s" % (name, seen, w))


def test_ties_go_to_the_lowest_hypothesis_then_root(native, oracle):
    p = _problem(32, 9)
    p["xyz"] = np.repeat(p["xyz"], 2, 0)
    p["uv"] = np.repeat(p["uv"], 2, 0)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], hypotheses=64, debug=True, want_mask=True)[0]
    _check_counts(oracle, d, p, native.K_REF, 9.0)
    best = d["hyp_count"].max()
    assert (d["hyp_count"] == best).sum() >= 2 and best == 64
    w = _check_winner(native, d, p, native.K_REF, 9.0)
    first = np.argwhere(d["hyp_count"] == best)[0]
    assert (w[0], w[1]) == tuple(first)
    # below min_inliers: not found, the best count still reported
    e = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], hypotheses=64, min_inliers=65, debug=True, want_mask=True)[0]
    assert _check_winner(native, e, p, native.K_REF, 9.0, min_inliers=65) is None and e["inliers"] == 64


def test_counts_over_several_hypothesis_tiles_and_slices(native, oracle):
    """The score stage's walk beyond one tile of hypotheses: two whole tiles and a tile of 2 (130
    hypotheses with the kernel's tile of 64).  A: one problem of one correspondence more than a
    score block holds (1025): two score blocks, the second with a single item, and three slices of
    grid y, one tile each.  B: 400 problems of 5: 400 score blocks, two slices; slice 0 walks tiles
    0 and 2, slice 1 takes tile 1 (tests/test_ransac_cpu.py holds the plan of both shapes to these
    figures).  The tile sizes are the library's own."""
    HT, TILE = native.lib().picp_pnp_hyp_tile(), native.lib().picp_pnp_score_tile()
    H, K, thr = 2 * HT + 2, native.K_REF, 9.0
    # no outliers, so that nearly every triple has a pose and the tile of 2 is not empty; the
    # pixel noise spreads the counts
    p = _problem(TILE + 1, 31, pixel_noise=0.5)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], threshold=thr, hypotheses=H, debug=True, want_mask=True)[0]
    seen = _check_counts(oracle, d, p, K, thr)
    assert seen >= 8 and (d["n_roots"][HT:2 * HT] > 0).any() and (d["n_roots"][2 * HT:] > 0).any()  # every tile has a pose
    _check_winner(native, d, p, K, thr)
    ps = [_problem(5, 100 + i, pixel_noise=0.5) for i in range(400)]
    out = native.pnp_ransac_batch([q["xyz"] for q in ps], [q["uv"] for q in ps], threshold=thr, hypotheses=H,
                                  debug=True, want_mask=True)
    for i, d in enumerate(out):
        assert d["hyp_count"].shape == (H, 4) and (d["hyp_count"] >= 0).all() and (d["hyp_count"] <= 5).all()
        assert (d["hyp_count"][np.arange(4)[None, :] >= d["n_roots"][:, None]] == 0).all(), i
    for i in (0, 199, 399):
        np.testing.assert_array_equal(out[i]["samples"], R.samples(0, i, H, 5))
        assert _check_counts(oracle, out[i], ps[i], K, thr) >= 3
        assert (out[i]["n_roots"][HT:2 * HT] > 0).any() and (out[i]["n_roots"][2 * HT:] > 0).any()
        _check_winner(native, out[i], ps[i], K, thr)


# ---------------------------------------------------------------------------------------------
# 5. end to end: a ragged batch, polished by the batch solver
# ---------------------------------------------------------------------------------------------
def test_ragged_batch_then_picp_reaches_the_near_prior_solution(native):
    from picp_amd import synth
    ps = [_problem(n, seed, outlier_frac=0.5, pixel_noise=0.5) for n, seed in R.E2E_CASES]
    small = {2: _problem(3, 1), 5: _problem(4, 2)}
    xyz, uv, real = [], [], []
    for i in range(len(ps) + 3):
        if i == 0:
            xyz.append(np.zeros((0, 3), np.float32)), uv.append(np.zeros((0, 2), np.float32))
        elif i in small:
            xyz.append(small[i]["xyz"]), uv.append(small[i]["uv"])
        else:
            real.append(i)
            xyz.append(ps[len(real) - 1]["xyz"]), uv.append(ps[len(real) - 1]["uv"])
    out = native.pnp_ransac_batch(xyz, uv, want_mask=True)
    for i in (0, 2):
        assert not out[i]["found"] and (out[i]["T"] == np.eye(4, dtype=np.float32)).all() and out[i]["inliers"] == 0
    assert out[5]["inliers"] <= 4 and np.isfinite(out[5]["T"]).all()
    b = native.Batch([len(p["xyz"]) for p in ps], rows=ROWS, cols=COLS)
    b.set_data(np.concatenate([p["xyz"] for p in ps]), np.concatenate([p["uv"] for p in ps]))
    b.set_poses(np.stack([out[i]["T"] for i in real]))
    b.solve(threshold=3000.0)
    Ta = b.poses()
    b.set_poses(np.stack([p["T_init"] for p in ps]))
    b.solve(threshold=3000.0)
    Tb = b.poses()
    b.close()
    for k, i in enumerate(real):
        good = int((~ps[k]["outlier"]).sum())
        dist = synth.se3_log_norm(Ta[k], Tb[k])
        print("n %d seed %d: %d inliers of %d non-outliers, se3(picp from ransac, picp from T_init) = %.2e"
              % (R.E2E_CASES[k] + (out[i]["inliers"], good, dist)))
        assert out[i]["found"] and out[i]["inliers"] >= 0.9 * good
        assert int(out[i]["mask"].sum()) == out[i]["inliers"]
        assert dist < 1e-4


# ---------------------------------------------------------------------------------------------
# 6. the point of the feature: a frame whose prior is useless
# ---------------------------------------------------------------------------------------------
def _far(T_init):
    from picp_amd import synth
    D = np.eye(4)
    D[:3, :3] = synth.euler_xyz(FAR[0], FAR[0], FAR[0])
    D[:3, 3] = FAR[1]
    return (D @ T_init.astype(np.float64)).astype(np.float32)


def test_relocalize_then_solve_from_a_far_prior(native):
    from picp_amd import synth
    checked, plain = 0, 0
    for seed in range(10):
        p = _problem(500, seed, outlier_frac=0.3, pixel_noise=0.5)
        s = native.PICPSolver()
        s.init(p["T_init"], p["world"], p["image"])
        s.setKernelThreshold(3000.0)
        s.solve(p["pairs"])
        T_near = s.pose()
        s.set_pose(_far(p["T_init"]))
        s.solve(p["pairs"])
        plain += synth.se3_log_norm(s.pose(), T_near) < 1e-4
        s.set_pose(_far(p["T_init"]))
        found, inl = s.relocalize(p["pairs"])
        s.solve(p["pairs"])
        d = synth.se3_log_norm(s.pose(), T_near)
        near_ok = synth.se3_log_norm(T_near, p["T_gt"]) < 1e-2
        print("seed %d: near-prior solve ok %s, relocalize found %s (%d inliers), se3 to the near-prior solve %.2e"
              % (seed, near_ok, found, inl, d))
        if near_ok:
            checked += 1
            assert found and d < 1e-4, seed
        s.close()
    print("plain solve() from the far prior reaches the near-prior solution on %d of 10 seeds" % plain)
    assert checked >= 5  # the comparison is not vacuous (9 of 10 on the CPU oracle)


def test_failed_relocalize_leaves_pose_and_stats(native):
    p = _problem(64, 1, outlier_frac=0.3, pixel_noise=0.5)
    s = native.PICPSolver()
    s.init(p["T_init"], p["world"], p["image"])
    s.setKernelThreshold(3000.0)
    s.solve(p["pairs"], max_rounds=3, conv_eps=-1.0)
    pose, stats = _bits(s.pose()).copy(), bytes(s._stats)
    found, inl = s.relocalize(p["pairs"], min_inliers=65)
    assert not found and 0 < inl <= 64
    np.testing.assert_array_equal(_bits(s.pose()), pose)
    assert bytes(s._stats) == stats
    found, inl2 = s.relocalize(p["pairs"])
    assert found and inl2 == inl
    # the handle's RANSAC is the batch call on the gathered correspondences (problem 0)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]])[0]
    np.testing.assert_array_equal(_bits(s.pose()), _bits(d["T"]))
    s.close()


def test_facade_program(native, tmp_path):
    """bin/pnp_main (pr::localize, PICPSolver::relocalize, the oneRound loop) prints the poses of
    the Python path bit for bit."""
    p = _problem(500, 3, outlier_frac=0.3, pixel_noise=0.5)
    far, rounds, seed = _far(p["T_init"]), 12, 77
    path = tmp_path / "problem.txt"
    with open(path, "w") as f:
        f.write("%d %d\n" % (ROWS, COLS))
        f.write(" ".join(repr(float(v)) for v in np.asarray(native.K_REF).reshape(-1)) + "\n")
        f.write("9.0 128 4 %d\n3000.0 %d\n" % (seed, rounds))
        f.write("%d %d %d\n" % (len(p["world"]), len(p["image"]), len(p["pairs"])))
        f.write(" ".join(repr(float(v)) for v in far.reshape(-1)) + "\n")
        for a in (p["world"], p["image"]):
            for row in a:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
        for a, b in p["pairs"]:
            f.write("%d %d\n" % (a, b))
    out = subprocess.run([os.path.join(PKG, "bin", "pnp_main"), str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = {l.split()[0]: l.split()[1:] for l in out.stdout.strip().splitlines()}
    s = native.PICPSolver()
    s.init(far, p["world"], p["image"])
    s.setKernelThreshold(3000.0)
    found, inl = s.relocalize(p["pairs"], hypotheses=128, seed=seed)
    want = _bits(native.pose_to_c(s.pose()))
    for key in ("localize", "relocalize"):
        assert [int(v) for v in lines[key][:2]] == [int(found), inl]
        np.testing.assert_array_equal(np.array([int(v, 16) for v in lines[key][2:]], np.uint32), want)
    good = sum(s.oneRound(p["pairs"]) for _ in range(rounds))
    assert int(lines["final"][0]) == good == rounds
    np.testing.assert_array_equal(np.array([int(v, 16) for v in lines["final"][1:]], np.uint32),
                                  _bits(native.pose_to_c(s.pose())))
    s.close()


# ---------------------------------------------------------------------------------------------
# 7. sizes
# ---------------------------------------------------------------------------------------------
def test_more_problems_than_a_grid_dimension(native, oracle):
    p = _problem(4, 21)
    P = 70001
    out = native.pnp_ransac_batch([p["xyz"]] * P, [p["uv"]] * P, hypotheses=1, debug=True)
    inl = np.array([d["inliers"] for d in out])
    cnt = np.array([d["hyp_count"][0].max() for d in out])
    np.testing.assert_array_equal(inl, cnt)
    assert all(d["found"] == (d["inliers"] >= 4) for d in out)
    for i in (0, 1, 65534, 65535, 65536, 70000):
        np.testing.assert_array_equal(out[i]["samples"], R.samples(0, i, 1, 4))
        _check_counts(oracle, out[i], p, native.K_REF, 9.0)
    assert (inl == 4).sum() > P // 2  # a noiseless frame: most triples find all four points


def test_one_large_problem(native, oracle):
    p = _problem(100000, 5, outlier_frac=0.3, pixel_noise=0.5)
    d = native.pnp_ransac_batch([p["xyz"]], [p["uv"]], hypotheses=16, debug=True, want_mask=True)[0]
    assert d["found"]
    assert d["inliers"] == R.count(oracle, d["T"], native.K_REF, ROWS, COLS, p["xyz"], p["uv"], 9.0)
    w = R.select(d["hyp_count"], d["n_roots"])
    assert d["inliers"] == w[2] and int(d["mask"].sum()) == w[2]
    np.testing.assert_array_equal(_bits(d["T"]), _bits(d["hyp_T"][w[0]][w[1]]))
