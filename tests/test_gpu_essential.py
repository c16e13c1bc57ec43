"""GPU parity of the essential-matrix bootstrap (src/cam.cpp:37-91: findEssentialMat + recoverPose,
SURVEY.md §8f rank 4) against the oracle (oracle/picp_essential.c), which is pinned by reproducing
the reference's published trajectory (tests/test_oracle.py::test_kat_bootstrap_reproduces_reference_run).

Both compute the same RANSAC subsets, five-point solutions and inlier counts in double (the
kernels with FP contraction off), so the chosen model, its inlier count and recoverPose's count
are equal and the poses agree to float rounding of the output.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _oracle_full(oracle, p1, p2, K, dist=50.0, **kw):
    """-> (T, inliers, good, mask): find_essential with **kw, then recover_pose with dist."""
    E, cnt = oracle.find_essential(p1, p2, K, **kw)
    if E is None:
        return np.eye(4), 0, 0, np.zeros(len(p1), bool)
    R, t, mask, good = oracle.recover_pose(E, p1, p2, K, dist=dist)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return np.linalg.inv(T), cnt, good, mask


def _oracle_pose(oracle, p1, p2, K, **kw):
    return _oracle_full(oracle, p1, p2, K, **kw)[:3]


def _data_pairs(oracle, vo, ks):
    p1s, p2s = [], []
    for k in ks:
        fa, fb = vo.frame(k), vo.frame(k + 1)
        m = oracle.match_points(fa["desc"], fb["desc"])  # exec/icp_test.cpp:46
        acc = m["accepted"].astype(bool)
        p1s.append(fa["uv"][acc])
        p2s.append(fb["uv"][m["best_idx"][acc]])
    return p1s, p2s


def test_essential_matches_oracle_on_every_data_frame_pair(native, oracle, vo):
    """All 120 consecutive pairs of data/ in one batch (frames 0-1 is the reference's bootstrap;
    the others include near-pure-rotation pairs where recoverPose keeps few points)."""
    ks = list(range(vo.n_frames - 1))
    p1s, p2s = _data_pairs(oracle, vo, ks)
    K = vo.K.astype(np.float64)
    res = native.essential_recover_pose_batch(p1s, p2s, K=vo.K, want_mask=True)
    for k, r in zip(ks, res):
        T, inl, good, mask = _oracle_full(oracle, p1s[k], p2s[k], K)
        assert r["inliers"] == inl, k
        assert r["good"] == good, k
        assert r["mask"].sum() == good, k
        np.testing.assert_array_equal(r["mask"], mask, err_msg="pair %d" % k)
        np.testing.assert_allclose(r["T"], T, atol=2e-6, err_msg="pair %d" % k)


def test_essential_bootstrap_frame0_is_reference_pose(native, oracle, vo):
    p1s, p2s = _data_pairs(oracle, vo, [0])
    r = native.essential_recover_pose_batch(p1s, p2s, K=vo.K)[0]
    assert r["inliers"] == 115 and r["good"] == 115
    # the reference's bootstrap after frame 1's PICP is output/estimated_trajectory.txt row 1
    row = vo.trajectory_rows([np.eye(4), r["T"]])[1]
    np.testing.assert_allclose(row[1:], vo.ref_trajectory[1, 1:], atol=5e-5)


def _two_view(rng, n, outlier_frac, noise_px):
    K = np.array([[180.0, 0, 320], [0, 180, 240], [0, 0, 1]])
    ang = rng.normal(0, 0.1, 3)
    th = np.linalg.norm(ang)
    kx = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    t = rng.normal(0, 1, 3)
    t[2] = abs(t[2])
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-3, 3, (n, 2)), rng.uniform(3, 10, n)]
    X2 = X @ R.T + t
    p1 = (X @ K.T)[:, :2] / X[:, 2:]
    p2 = (X2 @ K.T)[:, :2] / X2[:, 2:]
    p1 += rng.normal(0, noise_px, p1.shape)
    p2 += rng.normal(0, noise_px, p2.shape)
    bad = rng.random(n) < outlier_frac
    p2[bad] = rng.uniform([0, 0], [640, 480], (bad.sum(), 2))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return p1.astype(np.float32), p2.astype(np.float32), np.linalg.inv(T), K


def test_essential_synthetic_outliers_and_noise(native, oracle):
    rng = np.random.default_rng(7)
    cases = [_two_view(rng, n, of, nz) for n, of, nz in
             [(200, 0.0, 0.0), (200, 0.3, 0.3), (500, 0.5, 0.5), (60, 0.2, 0.2), (1000, 0.3, 0.5), (9, 0.0, 0.1)]]
    res = native.essential_recover_pose_batch([c[0] for c in cases], [c[1] for c in cases], K=cases[0][3])
    for i, (p1, p2, Tgt, K) in enumerate(cases):
        T, inl, good = _oracle_pose(oracle, p1, p2, K)
        assert res[i]["inliers"] == inl and res[i]["good"] == good, i
        np.testing.assert_allclose(res[i]["T"], T, atol=2e-6, err_msg="case %d" % i)
        # and the geometry is recovered (unit baseline)
        assert np.abs(res[i]["T"][:3, :3] - Tgt[:3, :3]).max() < 5e-2, i
        assert np.abs(res[i]["T"][:3, 3] - Tgt[:3, 3]).max() < 0.25, i  # 9 points, 0.1 px: 0.17


def test_essential_edge_cases(native, oracle):
    rng = np.random.default_rng(11)
    p1, p2, _, K = _two_view(rng, 40, 0.0, 0.0)
    res = native.essential_recover_pose_batch([p1[:3], np.zeros((0, 2)), p1[:5], p1], [p2[:3], np.zeros((0, 2)), p2[:5], p2],
                                              K=K)
    for r in res[:2]:  # fewer than five points: no model
        assert r["inliers"] == 0 and r["good"] == 0
        np.testing.assert_array_equal(r["T"], np.eye(4))
    T5, inl5, good5 = _oracle_pose(oracle, p1[:5], p2[:5], K)
    assert res[2]["inliers"] == inl5 == 5
    np.testing.assert_allclose(res[2]["T"], T5, atol=2e-6)
    assert res[3]["inliers"] == 40
    with pytest.raises(native.PicpError):
        native.essential_recover_pose_batch([p1], [p2], K=K, max_iters=0)
    with pytest.raises(native.PicpError):
        native.essential_recover_pose_batch([p1], [p2], K=K, prob=1.0)


def _planar(rng, n, outlier_frac, noise_px):
    """_two_view with every point on the plane z = 6 of the first camera."""
    K = np.array([[180.0, 0, 320], [0, 180, 240], [0, 0, 1]])
    ang = np.array([0.04, -0.08, 0.03])
    th = np.linalg.norm(ang)
    kx = np.array([[0, -ang[2], ang[1]], [ang[2], 0, -ang[0]], [-ang[1], ang[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx
    t = np.array([0.8, -0.2, 0.3])
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-3, 3, (n, 2)), np.full(n, 6.0)]
    X2 = X @ R.T + t
    p1 = (X @ K.T)[:, :2] / X[:, 2:] + rng.normal(0, noise_px, (n, 2))
    p2 = (X2 @ K.T)[:, :2] / X2[:, 2:] + rng.normal(0, noise_px, (n, 2))
    bad = rng.random(n) < outlier_frac
    p2[bad] = rng.uniform([0, 0], [640, 480], (bad.sum(), 2))
    return p1.astype(np.float32), p2.astype(np.float32)


DEFAULTS = {"max_iters": 1000, "threshold": 1.0, "prob": 0.999, "dist": 50.0}
# one parameter at a time (the hypothesis kernel's grid is ceil(max_iters / 64): 1, 63, 64, 65 sit on
# both sides of one block; the adaptive bound depends on prob, the cheirality test on dist), then
# all four away from their defaults
SWEEP = ([{"max_iters": m} for m in (1, 63, 64, 65, 1000)] + [{"threshold": t} for t in (0.25, 1.0, 3.0)] +
         [{"prob": p} for p in (0.5, 0.9999)] + [{"dist": d} for d in (6.0, 50.0)] +
         [{"max_iters": 65, "threshold": 0.25, "prob": 0.5, "dist": 6.0}])


@pytest.fixture(scope="module")
def sweep_problems(oracle, vo):
    """The cases of test_essential_synthetic_outliers_and_noise, a planar scene, three data pairs and
    a case with 70 % outliers."""
    rng = np.random.default_rng(7)
    cases = [_two_view(rng, n, of, nz) for n, of, nz in
             [(200, 0.0, 0.0), (200, 0.3, 0.3), (500, 0.5, 0.5), (60, 0.2, 0.2), (1000, 0.3, 0.5), (9, 0.0, 0.1)]]
    K = cases[0][3]
    np.testing.assert_array_equal(np.asarray(vo.K, np.float64), K)  # one K per batch
    p1s, p2s = [c[0] for c in cases], [c[1] for c in cases]
    a, b = _planar(np.random.default_rng(8), 150, 0.2, 0.3)
    d1, d2 = _data_pairs(oracle, vo, [0, 37, 90])
    # 70 % outliers: the adaptive bound never drops below max_iters, so every hypothesis counts
    hard = _two_view(np.random.default_rng(9), 150, 0.7, 0.5)
    return p1s + [a] + d1 + [hard[0]], p2s + [b] + d2 + [hard[1]], K


@pytest.mark.parametrize("over", SWEEP, ids=lambda o: ",".join("%s=%g" % kv for kv in o.items()))
def test_essential_parameter_sweep_matches_oracle(native, oracle, sweep_problems, over):
    """max_iters, threshold, prob and dist away from their defaults: one batch per parameter set,
    inliers, good and the recoverPose mask (element by element) equal to the oracle's with the same
    keywords, T to the float rounding of the output."""
    p1s, p2s, K = sweep_problems
    kw = dict(DEFAULTS, **over)
    res = native.essential_recover_pose_batch(p1s, p2s, K=K, want_mask=True, **kw)
    for i, r in enumerate(res):
        T, inl, good, mask = _oracle_full(oracle, p1s[i], p2s[i], K, **kw)
        assert r["inliers"] == inl, (i, r["inliers"], inl)
        assert r["good"] == good, (i, r["good"], good)
        np.testing.assert_array_equal(r["mask"], mask, err_msg="problem %d" % i)
        np.testing.assert_allclose(r["T"], T, atol=2e-6, err_msg="problem %d" % i)


def test_essential_sweep_parameters_change_the_answer(oracle, sweep_problems):
    """The sweep discriminates: on the oracle each parameter moves the counts of some case, so a
    kernel that ignored one of them would fail the sweep."""
    p1s, p2s, K = sweep_problems

    def counts(i, **over):
        return _oracle_full(oracle, p1s[i], p2s[i], K, **dict(DEFAULTS, **over))[1:3]

    base = counts(1)  # 200 points, 30 % outliers
    assert counts(1, max_iters=1)[0] < base[0]
    assert counts(1, threshold=0.25)[0] < base[0] < counts(1, threshold=3.0)[0]
    assert counts(1, dist=6.0)[1] < base[1]
    assert counts(1, prob=0.5)[0] < base[0]  # a lower bound on the iterations keeps a worse model
    assert counts(-1, max_iters=64)[0] < counts(-1)[0]  # 70 % outliers: hypotheses 65 .. 1000 matter


def test_essential_more_problems_than_a_grid_has_rows(native, oracle):
    """70,001 problems: the hypothesis and score kernels take the problem from blockIdx.y, whose
    limit is 65,535, so the launch wrapper runs such a batch in slices.  16 distinct problems of
    4 to 12 points (one without a model, one with exactly five points) tiled over the batch: the
    first, the last, every 4,099th and the 16 around index 65,535 equal the oracle's answer for
    their source; every other problem has the bits of its source's first occurrence."""
    rng = np.random.default_rng(21)
    sizes = [8, 9, 10, 11, 12, 4, 5, 8, 9, 10, 11, 12, 8, 10, 12, 9]
    src = [_two_view(rng, 12, 0.3 if k % 2 else 0.0, 0.2)[:2] for k in range(16)]
    src = [(a[:n], b[:n]) for (a, b), n in zip(src, sizes)]
    K = np.array([[180.0, 0, 320], [0, 180, 240], [0, 0, 1]])
    n_prob = 70001
    p1s = [src[i % 16][0] for i in range(n_prob)]
    p2s = [src[i % 16][1] for i in range(n_prob)]
    res = native.essential_recover_pose_batch(p1s, p2s, K=K, max_iters=4, want_mask=True)
    assert len(res) == n_prob
    ref = [_oracle_full(oracle, a, b, K, max_iters=4) for a, b in src]
    assert ref[5][1] == 0 and ref[6][1] == 5 and sum(r[1] > 0 for r in ref) == 15
    assert len({(r[1], r[2]) for r in ref}) >= 8  # the sources differ, so a shifted slice would show
    checked = sorted(set([0, n_prob - 1] + list(range(0, n_prob, 4099)) + list(range(65535 - 8, 65535 + 8))))
    for i in checked:
        T, inl, good, mask = ref[i % 16]
        assert (res[i]["inliers"], res[i]["good"]) == (inl, good), i
        np.testing.assert_array_equal(res[i]["mask"], mask, err_msg="problem %d" % i)
        np.testing.assert_allclose(res[i]["T"], T, atol=2e-6, err_msg="problem %d" % i)
    T = np.stack([r["T"] for r in res]).view(np.uint32)
    cnt = np.array([(r["inliers"], r["good"]) for r in res])
    mask = np.concatenate([r["mask"] for r in res])
    reps = -(-n_prob // 16)
    np.testing.assert_array_equal(T, np.tile(T[:16], (reps, 1, 1))[:n_prob])
    np.testing.assert_array_equal(cnt, np.tile(cnt[:16], (reps, 1))[:n_prob])
    np.testing.assert_array_equal(mask, np.tile(mask[:sum(sizes)], reps)[:len(mask)])
