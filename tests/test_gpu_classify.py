"""GPU tests of the classify pass (picp_classify / picp_batch_classify, csrc/picp_classify.hip):
which correspondences a pose rests on.

The reference is the oracle evaluated point by point: oracle.error_and_jacobian gives ok and e,
chi2 = float32(e0*e0) + float32(e1*e1), oracle.project_point the projection.  state, chi2 and
proj_uv must equal it bit for bit (the library's gate is bit-exact to the reference); the inlier
indices and the counts follow from the states.  Above 4099 correspondences the per-point oracle
is replaced by a numpy float32 restatement in the oracle's operation order, itself checked
against the per-point oracle at 4099, plus the oracle's linearize counts.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG

pytestmark = pytest.mark.gpu

THR = 3000.0
ROWS, COLS = 480, 640
TILE = 1024  # CLS_TILE of picp_classify.hip: one of the sizes below
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 65537]
K_SKEW = np.array([[180, 3.5, 320], [0, 181, 240], [0, 0, 1.0000001]], np.float32)


def _synth():
    from picp_amd import synth
    return synth


@functools.lru_cache(maxsize=None)
def _problem(m, outlier_frac=0.3, pixel_noise=0.5, seed=42):
    synth = _synth()
    if m == 0:
        p = dict(synth.make_problem(4, seed=seed, outlier_frac=outlier_frac, pixel_noise=pixel_noise))
        p["pairs"] = np.zeros((0, 2), np.int32)
        p["xyz"] = np.zeros((0, 3), np.float32)
        p["uv"] = np.zeros((0, 2), np.float32)
        return p
    return synth.make_problem(m, seed=seed, outlier_frac=outlier_frac, pixel_noise=pixel_noise)


def _oracle_classify(O, T, K, xyz, uv, thr):
    """state, chi2, proj_uv of every correspondence from the oracle, point by point."""
    m = len(xyz)
    state = np.zeros(m, np.uint8)
    chi2 = np.full(m, -1.0, np.float32)
    puv = np.full((m, 2), -1.0, np.float32)
    for k in range(m):
        ok, e, _ = O.error_and_jacobian(T, K, ROWS, COLS, xyz[k], uv[k])
        if not ok:
            continue
        ok2, img = O.project_point(T, K, ROWS, COLS, xyz[k])
        assert ok2
        c = np.float32(e[0] * e[0]) + np.float32(e[1] * e[1])
        chi2[k] = c
        puv[k] = img
        state[k] = 2 if c > np.float32(thr) else 1
    return state, chi2, puv


def _np_classify(T, K, xyz, uv, thr):
    """The same in numpy float32, every operation rounded on its own, in the oracle's order."""
    f = np.float32
    T = np.asarray(T, f)
    K = np.asarray(K, f)
    x, y, z = (np.ascontiguousarray(xyz[:, i], f) for i in range(3))
    with np.errstate(all="ignore"):
        pc = [((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3] for i in range(3)]
        ph = [(K[i, 0] * pc[0] + K[i, 1] * pc[1]) + K[i, 2] * pc[2] for i in range(3)]
        iz = (f(1.0) / ph[2]).astype(f)
        ix, iy = ph[0] * iz, ph[1] * iz
        valid = ~(pc[2] <= 0) & ~((ix < 0) | (ix > f(COLS - 1)) | (iy < 0) | (iy > f(ROWS - 1)))
        e0, e1 = ix - uv[:, 0].astype(f), iy - uv[:, 1].astype(f)
        chi = e0 * e0 + e1 * e1
    assert chi.dtype == np.float32
    state = np.where(valid, np.where(chi > f(thr), 2, 1), 0).astype(np.uint8)
    return state, np.where(valid, chi, f(-1)).astype(f), np.where(valid[:, None], np.stack([ix, iy], 1), f(-1)).astype(f)


@functools.lru_cache(maxsize=None)
def _reference(m, outlier_frac, pixel_noise, pose, thr, general_k=False):
    import oracle as O
    p = _problem(m, outlier_frac, pixel_noise)
    K = K_SKEW if general_k else p["K"]
    T = _pose(p, pose)
    if m <= 4099:
        return _oracle_classify(O, T, K, p["xyz"], p["uv"], thr)
    return _np_classify(T, K, p["xyz"], p["uv"], thr)


def _pose(p, which):
    if which == "init":
        return p["T_init"]
    if which == "gt":
        return p["T_gt"]
    assert which == "behind"  # T_gt turned by pi about the camera y axis: every point has z < 0
    R = np.diag([-1.0, 1.0, -1.0, 1.0])
    return (R @ p["T_gt"].astype(np.float64)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def _assert_equal_bits(got, ref):
    state, chi2, puv = ref
    np.testing.assert_array_equal(got["state"], state)
    np.testing.assert_array_equal(_bits(got["chi2"]), _bits(chi2))
    np.testing.assert_array_equal(_bits(got["uv"]), _bits(puv))
    np.testing.assert_array_equal(got["inlier_idx"], np.nonzero(state == 1)[0])
    np.testing.assert_array_equal(got["counts"], np.bincount(state, minlength=3))


def _classify(native, p, T, thr, K=None):
    s = native.PICPSolver(rows=ROWS, cols=COLS, K=p["K"] if K is None else K)
    s.init(T, p["world"], p["image"])
    s.setKernelThreshold(thr)
    return s, s.classify(p["pairs"])


def test_numpy_restatement_is_the_oracle(oracle):
    """The reference used above 4099 correspondences equals the per-point oracle, and both equal
    the oracle's linearize counts."""
    p = _problem(4099)
    a = _oracle_classify(oracle, p["T_init"], p["K"], p["xyz"], p["uv"], THR)
    b = _np_classify(p["T_init"], p["K"], p["xyz"], p["uv"], THR)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    lin = oracle.linearize(p["T_init"], p["K"], ROWS, COLS, p["world"], p["image"], p["pairs"], THR)
    assert (a[0] == 1).sum() == lin["n_in"] and (a[0] != 0).sum() == lin["n_projected"]


@pytest.mark.parametrize("m", SIZES)
def test_sizes_match_oracle_bit_for_bit(native, oracle, m):
    assert TILE in SIZES and TILE - 1 in SIZES and TILE + 1 in SIZES
    p = _problem(m)
    _, got = _classify(native, p, p["T_init"], THR)
    ref = _reference(m, 0.3, 0.5, "init", THR)
    _assert_equal_bits(got, ref)
    if m > 4099:
        lin = oracle.linearize(p["T_init"], p["K"], ROWS, COLS, p["world"], p["image"], p["pairs"], THR)
        assert got["counts"][1] == lin["n_in"] and got["counts"][1] + got["counts"][2] == lin["n_projected"]


@pytest.mark.parametrize("thr,outlier_frac,expect", [(3000.0, 0.3, (161, 2794, 1144)), (4.0, 0.0, (163, 163, 3773))])
def test_mixed_classes(native, thr, outlier_frac, expect):
    p = _problem(4099, outlier_frac, 0.5)
    _, got = _classify(native, p, p["T_init"], thr)
    ref = _reference(4099, outlier_frac, 0.5, "init", thr)
    assert tuple(np.bincount(ref[0], minlength=3)) == expect  # what the oracle gives
    assert all(c > 0 for c in got["counts"])
    _assert_equal_bits(got, ref)


@pytest.mark.parametrize("case", ["all_skipped", "all_inliers", "all_outliers"])
def test_degenerate_sets(native, case):
    m = 4099
    if case == "all_skipped":
        args, pose, thr, cls = (0.3, 0.5), "behind", THR, 0
    elif case == "all_inliers":
        args, pose, thr, cls = (0.0, 0.0), "gt", THR, 1
    else:
        args, pose, thr, cls = (0.0, 0.5), "gt", 0.0, 2
    p = _problem(m, *args)
    _, got = _classify(native, p, _pose(p, pose), thr)
    ref = _reference(m, args[0], args[1], pose, thr)
    _assert_equal_bits(got, ref)
    expect = [0, 0, 0]
    expect[cls] = m
    assert list(np.bincount(ref[0], minlength=3)) == expect  # what the oracle gives
    assert list(got["counts"]) == expect


def test_general_k(native):
    p = _problem(1000, 0.3, 0.5)
    _, got = _classify(native, p, p["T_init"], THR, K=K_SKEW)
    ref = _reference(1000, 0.3, 0.5, "init", THR, True)
    assert all(c > 0 for c in np.bincount(ref[0], minlength=3))
    _assert_equal_bits(got, ref)


def test_consistent_with_linearize(native):
    p = _problem(4099)
    s, got = _classify(native, p, p["T_init"], THR)
    lin = s.linearize(p["pairs"])
    assert lin["n_in"] == got["counts"][1]
    assert lin["n_projected"] == got["counts"][1] + got["counts"][2]
    chi_in = got["chi2"][got["state"] == 1].astype(np.float64).sum()
    assert abs(chi_in - lin["chi_in"]) <= 1e-5 * abs(lin["chi_in"])
    np.testing.assert_array_equal(s.pose(), p["T_init"])  # neither call moved the pose


def _solve_twice(native, p, with_classify):
    s = native.PICPSolver()
    s.init(p["T_init"], p["world"], p["image"])
    s.setKernelThreshold(THR)
    out = []
    for k in range(2):
        s.set_pose(p["T_init"])
        st = s.solve(p["pairs"], max_rounds=20, conv_eps=-1.0)
        out.append((s.pose().copy(), dict(st)))
        if with_classify and k == 0:
            pose = s.pose().copy()
            c = s.classify(p["pairs"])
            assert c["counts"].sum() == len(p["pairs"])
            np.testing.assert_array_equal(s.pose(), pose)
    return out


def test_classify_does_not_change_a_solve(native):
    p = _problem(4099)
    a = _solve_twice(native, p, True)
    b = _solve_twice(native, p, False)
    for (Ta, sa), (Tb, sb) in zip(a, b):
        np.testing.assert_array_equal(_bits(Ta), _bits(Tb))
        assert sa == sb


def _batch_mode(native, sizes, mode):
    old = os.environ.get("PICP_MODE")
    os.environ["PICP_MODE"] = mode
    try:
        return native.Batch(sizes)
    finally:
        if old is None:
            os.environ.pop("PICP_MODE", None)
        else:
            os.environ["PICP_MODE"] = old


def _batch_data(sizes):
    ps = [_problem(int(n), 0.3, 0.5, seed=100 + i) if n else _problem(0) for i, n in enumerate(sizes)]
    xyz = np.concatenate([p["xyz"] for p in ps]) if sum(sizes) else np.zeros((0, 3), np.float32)
    uv = np.concatenate([p["uv"] for p in ps]) if sum(sizes) else np.zeros((0, 2), np.float32)
    return ps, xyz, uv, np.stack([p["T_init"] for p in ps])


@pytest.mark.parametrize("mode,sizes", [("block", [1000] * 8), ("persistent", [100003])])
def test_classify_does_not_change_a_batch_solve(native, mode, sizes):
    ps, xyz, uv, T0 = _batch_data(sizes)
    res = []
    for with_classify in (True, False):
        b = _batch_mode(native, sizes, mode)
        assert b.info()["mode"] == mode
        b.set_data(xyz, uv)
        b.set_poses(T0)
        out = []
        for k in range(2):
            b.solve(threshold=THR, max_rounds=20, conv_eps=-1.0)
            out.append((b.poses().copy(), b.stats()))
            if with_classify and k == 0:
                c = b.classify(THR)
                assert c["counts"].sum() == sum(sizes)
                np.testing.assert_array_equal(_bits(b.poses()), _bits(out[0][0]))
        assert b.info()["mode"] == mode
        res.append(out)
    for (Ta, sa), (Tb, sb) in zip(*res):
        np.testing.assert_array_equal(_bits(Ta), _bits(Tb))
        assert sa == sb


def _single(native, p, T, thr):
    """picp_classify of one problem alone (xyz/uv in pair order, identity pairs)."""
    s = native.PICPSolver()
    n = len(p["xyz"])
    s.init(T, p["xyz"] if n else np.zeros((1, 3), np.float32), p["uv"] if n else np.zeros((1, 2), np.float32))
    s.setKernelThreshold(thr)
    return s.classify(np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32))


def _assert_batch_equals_singles(native, got, ps, sizes, poses, thr):
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    np.testing.assert_array_equal(got["inlier_off"], np.concatenate([[0], np.cumsum(got["counts"][:, 1])]))
    for i, p in enumerate(ps):
        one = _single(native, p, poses[i], thr)
        sl = slice(offs[i], offs[i + 1])
        np.testing.assert_array_equal(got["state"][sl], one["state"])
        np.testing.assert_array_equal(_bits(got["chi2"][sl]), _bits(one["chi2"]))
        np.testing.assert_array_equal(got["counts"][i], one["counts"])
        np.testing.assert_array_equal(got["inlier_idx"][got["inlier_off"][i]:got["inlier_off"][i + 1]], one["inlier_idx"])


@pytest.mark.parametrize("sizes", [[0, 1, 5, 257, 0, 4099, 3, 1024], [1000] * 8, [10] * 128],
                         ids=["ragged", "8x1000", "128x10"])
def test_batch_equals_single_problem_classify(native, sizes):
    ps, xyz, uv, T0 = _batch_data(sizes)
    b = native.Batch(sizes)
    b.set_data(xyz, uv)
    # explicit poses
    _assert_batch_equals_singles(native, b.classify(THR, poses=T0), ps, sizes, T0, THR)
    # NULL after set_poses: those poses
    b.set_poses(T0)
    got = b.classify(THR)
    exp = b.classify(THR, poses=T0)
    for k in ("state", "inlier_off", "inlier_idx", "counts"):
        np.testing.assert_array_equal(got[k], exp[k])
    np.testing.assert_array_equal(_bits(got["chi2"]), _bits(exp["chi2"]))
    # NULL after a solve: the solved poses
    b.solve(threshold=THR, max_rounds=10, conv_eps=-1.0)
    T1 = b.poses()
    _assert_batch_equals_singles(native, b.classify(THR), ps, sizes, T1, THR)
    # state only (no chi2, no offsets wanted) gives the same states and counts
    lean = b.classify(THR, want_chi2=False)
    full = b.classify(THR)
    np.testing.assert_array_equal(lean["state"], full["state"])
    np.testing.assert_array_equal(lean["counts"], full["counts"])
    assert b.classify_time(THR, 2) > 0.0


def test_batch_with_more_tiles_than_one_scan_round(native):
    """9,000 problems of 2 correspondences are 9,000 tiles: more than the 8,192 the block scan
    covers per round, so the running totals carry from one round to the next.  All problems at one
    pose, so the batch must equal that pose's single classify of the 18,000 correspondences."""
    n, per = 9000, 2
    p = _problem(n * per)
    one = _single(native, p, p["T_init"], THR)
    b = native.Batch([per] * n)
    b.set_data(p["xyz"], p["uv"])
    got = b.classify(THR, poses=np.broadcast_to(p["T_init"], (n, 4, 4)))
    np.testing.assert_array_equal(got["state"], one["state"])
    np.testing.assert_array_equal(_bits(got["chi2"]), _bits(one["chi2"]))
    st = one["state"].reshape(n, per)
    np.testing.assert_array_equal(got["counts"], np.stack([(st == c).sum(1) for c in range(3)], 1))
    np.testing.assert_array_equal(got["inlier_off"], np.concatenate([[0], np.cumsum((st == 1).sum(1))]))
    owner = np.repeat(np.arange(n), (st == 1).sum(1))
    np.testing.assert_array_equal(got["inlier_idx"] + per * owner, one["inlier_idx"])


def test_state_errors(native):
    s = native.PICPSolver()
    with pytest.raises(native.PicpError) as e:
        s.classify(np.zeros((0, 2), np.int32))  # no points set
    assert e.value.code == native.ERR_STATE


def test_facade_program(native, tmp_path):
    """pr::PICPSolver::classify / inliers from plain host C++ on a 257-point problem."""
    p = _problem(257)
    ref = _reference(257, 0.3, 0.5, "init", THR)
    path = tmp_path / "problem.txt"
    with open(path, "w") as f:
        f.write("%d %d %r\n" % (ROWS, COLS, THR))
        f.write(" ".join(repr(float(v)) for v in p["K"].reshape(-1)) + "\n")
        f.write(" ".join(repr(float(v)) for v in p["T_init"].reshape(-1)) + "\n")
        f.write("%d %d %d\n" % (len(p["world"]), len(p["image"]), len(p["pairs"])))
        for arr in (p["world"], p["image"]):
            for row in arr:
                f.write(" ".join(repr(float(v)) for v in row) + "\n")
        for a, b in p["pairs"]:
            f.write("%d %d\n" % (a, b))
    out = subprocess.run([os.path.join(PKG, "bin", "classify_main"), str(path)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    counts = np.bincount(ref[0], minlength=3)
    assert [int(v) for v in lines["counts"].split()] == list(counts)
    inl = np.nonzero(ref[0] == 1)[0]
    checksum = sum((q + 1) * (int(p["pairs"][k, 0]) + 3 * int(p["pairs"][k, 1])) for q, k in enumerate(inl))
    assert [int(v) for v in lines["inliers"].split()] == [len(inl), checksum]
    assert lines["consistent"] == "1" and lines["pose_unchanged"] == "1"
