"""GPU tests of the alternating pose / point adjustment (picp_refine_run_poses, picp_refine_adjust;
csrc/picp_adjust.hip, csrc/picp_adjust_runtime.cpp).

Three things are exact and compared bit for bit: the pose-major view (integers and copied pixels)
with the numpy view of tests/adjust_ref.py; a pose step with a picp_amd.Batch fed the same lists
and poses; a run of sweeps with the same calls made one by one.  The adjustment as a whole is held
to the float64 reference of tests/adjust_ref.py: per case and sweep count, D_X / D_T = the largest
point / pose-entry difference between the reference run in float32 and in float64, measured on the
CPU (tests/test_adjust_cpu.py keeps the constants below honest).  Points that are not borderline in
any point step of the reference so far must lie within 4 D_X (the rule of test_gpu_refine.py),
every pose within the project's 1e-4 on the SE(3) log, and the steps' inlier counts must be equal.
"""
import numpy as np
import pytest

import adjust_ref as AR

pytestmark = pytest.mark.gpu

# metres / pose-entry units after 1 and 3 sweeps (adjust_ref.distances)
D_X = {"data_perturbed": {1: 6.68e-06, 3: 8.34e-06}, "synth": {1: 3.82e-04, 3: 2.82e-04}}
D_T = {"data_perturbed": {1: 5.72e-06, 3: 8.11e-06}, "synth": {1: 2.15e-06, 3: 7.15e-07}}
BORDERLINE_CAP = 0.01
POSE_TOL = 1e-4
STAT_KEYS = ("chi_in", "chi_out", "n_in", "ok", "rounds", "converged", "n_projected")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_stats(a, b, what):
    for k in STAT_KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32),
                                      err_msg="%s %s" % (what, k))


def _refiner(native, C, fixed=True):
    r = native.PointRefiner(rows=C["rows"], cols=C["cols"], K=C["K"])
    r.set_poses(C["poses"])
    r.set_tracks(C["off"], C["obs_pose"], C["obs_uv"])
    r.set_points(C["start"])
    if fixed:
        r.set_fixed_poses(C["fixed"])
    return r


def _two_long_names(native):
    t = native.adjust_rank_tile()
    return ["two_long_%d" % n for n in (t - 1, t, t + 1, 2 * t + 1)]


def _reversed(C):
    """The same tracks with the points in reverse order."""
    off = C["off"]
    order = np.arange(len(off) - 1)[::-1]
    idx = np.concatenate([np.arange(off[i], off[i + 1]) for i in order] + [np.zeros(0, np.int64)]).astype(np.int64)
    roff = np.zeros(len(off), np.int64)
    roff[1:] = np.cumsum(np.diff(off)[order])
    return {**C, "off": roff, "obs_pose": C["obs_pose"][idx], "obs_uv": C["obs_uv"][idx], "start": C["start"][order]}


# ---- 1. the view is exact

def _assert_view(r, C, what):
    off, pt, uv = r.pose_view()
    woff, wpt, wuv = AR.pose_view(len(C["poses"]), C["off"], C["obs_pose"], C["obs_uv"])
    assert off.dtype == np.int64 and pt.dtype == np.int32
    np.testing.assert_array_equal(off, woff, err_msg=what)
    np.testing.assert_array_equal(pt, wpt, err_msg=what)
    np.testing.assert_array_equal(_bits(uv), _bits(wuv), err_msg=what)


def test_view_is_exact(native, oracle):
    names = ["data_perturbed", "synth", "tiny"] + _two_long_names(native)
    assert names[-1] == "two_long_2049"  # the cases below were sized for a tile of 1024
    # the scan of the per-pose counts runs in chunks of 1,024 poses: one chunk short of full, full,
    # one pose into the second chunk, and three chunks with the boundary inside the non-empty run
    names += ["many_poses_%d" % n for n in (1023, 1024, 1025, 2049)]
    for name in names:
        C = AR.case(oracle, name)
        r = _refiner(native, C)
        _assert_view(r, C, name)
        _assert_view(r, C, name + " again")
        R = _reversed(C)
        r.set_tracks(R["off"], R["obs_pose"], R["obs_uv"])
        _assert_view(r, R, name + " reversed")
        r.close()
    C = AR.case(oracle, "tiny")
    off, pt, _ = AR.pose_view(3, C["off"], C["obs_pose"], C["obs_uv"])
    assert list(np.diff(off)) == [3, 2, 0] and list(pt[:3]) == [0, 2, 2]


# ---- 2. the pose step is the batch solve

@pytest.mark.parametrize("name", ["data_perturbed", "synth", "two_long_2049"])
def test_pose_step_is_the_batch_solve(native, oracle, name):
    C = AR.case(oracle, name)
    n = len(C["poses"])
    off, pt, uv = AR.pose_view(n, C["off"], C["obs_pose"], C["obs_uv"])
    mov = AR.movable_poses(C)
    assert len(mov) >= 2
    sel = np.concatenate([np.arange(off[k], off[k + 1]) for k in mov])
    for prm in ({}, {"keep_outliers": 1}):
        b = native.Batch(np.diff(off)[mov], rows=C["rows"], cols=C["cols"], K=C["K"])
        b.set_data(C["start"][pt[sel]], uv[sel])
        b.set_poses(C["poses"][mov])
        b.solve(**prm)
        want_T, want_st = b.poses(), b.stats()
        b.close()
        r = _refiner(native, C)
        T, st = r.run_poses(**prm)
        r.close()
        np.testing.assert_array_equal(_bits(T[mov]), _bits(want_T), err_msg="%s %s" % (name, prm))
        for j, k in enumerate(mov):
            assert {f: st[f][k].item() for f in STAT_KEYS} == {f: want_st[j][f] for f in STAT_KEYS}, (name, prm, k)
        assert (st["rounds"][mov] > 0).all() and (_bits(T[mov]) != _bits(C["poses"][mov])).any()
        rest = np.setdiff1d(np.arange(n), mov)
        np.testing.assert_array_equal(_bits(T[rest]), _bits(C["poses"][rest]))
        for f in STAT_KEYS:
            assert not np.asarray(st[f][rest]).view(np.uint32).any(), f


def test_pose_step_on_the_tiny_case(native, oracle):
    """Pose 2 is in no track and keeps its bits with zero stats; poses 0 and 1 are solved on lists of
    3 (one point twice) and 2 entries."""
    C = AR.case(oracle, "tiny")
    r = _refiner(native, C)
    T, st = r.run_poses(threshold=3000.0)
    r.close()
    np.testing.assert_array_equal(_bits(T[2]), _bits(C["poses"][2]))
    assert st["n_projected"][2] == 0 and st["rounds"][2] == 0 and st["ok"][2] == 0
    assert (st["rounds"][:2] > 0).all() and (_bits(T[:2]) != _bits(C["poses"][:2])).any()


# ---- 3. sweeps are the composition of the steps

def _alternate(r, sweeps):
    per = []
    for _ in range(sweeps):
        _, pt = r.run(**AR.POINTS)
        _, ps = r.run_poses(**AR.POSES)
        per.append((pt, ps))
    return per


@pytest.mark.parametrize("name", ["data_perturbed", "synth"])
def test_sweeps_are_the_composition(native, oracle, name):
    C = AR.case(oracle, name)
    a = _refiner(native, C)
    a.adjust(sweeps=3, points=AR.POINTS, poses=AR.POSES)
    b = _refiner(native, C)
    per = _alternate(b, 3)
    np.testing.assert_array_equal(_bits(a.points()), _bits(b.points()))
    np.testing.assert_array_equal(_bits(a.poses()), _bits(b.poses()))
    _same_stats(a.stats(), b.stats(), "point stats")
    _same_stats(a.pose_stats(), b.pose_stats(), "pose stats")
    rec = a.sweeps()
    assert len(rec) == 3
    for s, (pt, ps) in zip(rec, per):
        for kind, st in (("points", pt), ("poses", ps)):
            want = float(np.sum(st["chi_in"].astype(np.float64)))
            assert abs(s["chi_in_" + kind] - want) <= 1e-12 * abs(want), (kind, s, want)
            assert s["n_in_" + kind] == int(st["n_in"].astype(np.int64).sum())
            assert s["ok_" + kind] == int(st["ok"].astype(np.int64).sum())
    assert rec[0]["chi_in_points"] > rec[2]["chi_in_points"] > 0 and rec[0]["ok_poses"] == len(AR.movable_poses(C))
    c = _refiner(native, C)
    c.adjust(sweeps=3, points=AR.POINTS, poses=AR.POSES)
    np.testing.assert_array_equal(_bits(a.points()), _bits(c.points()))
    np.testing.assert_array_equal(_bits(a.poses()), _bits(c.poses()))
    assert c.sweeps() == rec
    for r in (a, b, c):
        r.close()


# ---- 4. against the float64 reference

@pytest.mark.parametrize("name", ["data_perturbed", "synth"])
def test_adjustment_matches_the_reference(native, oracle, name):
    from picp_amd import synth
    C = AR.case(oracle, name)
    ref = AR.reference(oracle, name, 3)
    want_sums = AR.record_sums(ref)
    border = np.zeros(len(C["start"]), bool)
    for sweeps in (1, 3):
        r = _refiner(native, C)
        r.adjust(sweeps=sweeps, points=AR.POINTS, poses=AR.POSES)
        X, T, rec = r.points(), r.poses(), r.sweeps()
        r.close()
        for s in ref[:sweeps]:
            border = border | s["border"]
        assert border.sum() <= BORDERLINE_CAP * len(border)
        want = ref[sweeps - 1]
        dx = np.abs(X.astype(np.float64) - want["X"].astype(np.float64)).max(1)[~border].max()
        dt = max(synth.se3_log_norm(a, b) for a, b in zip(T, want["poses"]))
        print("%s sweeps=%d: max|X - ref|=%.3g (D_X %.3g, bound %.3g)  max pose log=%.3g (D_T %.3g)" %
              (name, sweeps, dx, D_X[name][sweeps], 4 * D_X[name][sweeps], dt, D_T[name][sweeps]))
        assert np.isfinite(X).all() and np.isfinite(T).all()
        assert dx <= 4 * D_X[name][sweeps], (dx, 4 * D_X[name][sweeps])
        assert dt < POSE_TOL, dt
        for s, w in zip(rec, want_sums):
            assert (s["n_in_points"], s["n_in_poses"]) == (w["n_in_points"], w["n_in_poses"]), (s, w)


# ---- 5. edges

def test_zero_sweeps_and_all_fixed(native, oracle):
    C = AR.case(oracle, "synth")
    r = _refiner(native, C)
    r.adjust(sweeps=0, points=AR.POINTS, poses=AR.POSES)
    np.testing.assert_array_equal(_bits(r.points()), _bits(C["start"]))
    np.testing.assert_array_equal(_bits(r.poses()), _bits(C["poses"]))
    assert r.sweeps() == []
    with pytest.raises(native.PicpError) as e:
        r.stats()  # nothing ran
    assert e.value.code == native.ERR_STATE
    r.set_fixed_poses(np.ones(len(C["poses"]), bool))
    r.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    np.testing.assert_array_equal(_bits(r.poses()), _bits(C["poses"]))
    assert not any(np.asarray(v).view(np.uint32).any() for v in r.pose_stats().values())
    plain = _refiner(native, C)
    xyz, st = plain.run(**AR.POINTS)
    np.testing.assert_array_equal(_bits(r.points()), _bits(xyz))
    _same_stats(r.stats(), st, "all fixed")
    rec = r.sweeps()
    assert len(rec) == 1 and rec[0]["n_in_poses"] == 0 and rec[0]["n_in_points"] == int(st["n_in"].sum())
    r.close()
    plain.close()


def test_no_points(native, oracle):
    C = AR.case(oracle, "synth")
    r = native.PointRefiner(rows=C["rows"], cols=C["cols"], K=C["K"])
    r.set_poses(C["poses"])
    r.set_tracks(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
    r.set_points(np.zeros((0, 3), np.float32))
    off, pt, uv = r.pose_view()
    assert not off.any() and len(pt) == 0
    r.adjust(sweeps=2)
    np.testing.assert_array_equal(_bits(r.poses()), _bits(C["poses"]))
    rec = r.sweeps()
    assert len(rec) == 2 and all(v == 0 for s in rec for v in s.values())
    r.close()


def test_nan_pixel_stops_its_pose_only(native, oracle):
    C = AR.case(oracle, "data_perturbed")
    n = len(C["poses"])
    off, pt, _ = AR.pose_view(n, C["off"], C["obs_pose"], C["obs_uv"])
    j = 200  # one observation of point 200 by a movable pose
    src = next(int(q) for q in range(C["off"][j], C["off"][j + 1]) if C["obs_pose"][q] != 0)
    k = int(C["obs_pose"][src])
    bad = {**C, "obs_uv": C["obs_uv"].copy()}
    bad["obs_uv"][src, 0] = np.nan
    touch = np.array([(pt[off[q]:off[q + 1]] == j).any() for q in range(n)])
    assert touch[k] and 5 < (~touch).sum() < n
    clean = _refiner(native, C)
    clean.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    r = _refiner(native, bad)
    r.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    T, st = r.poses(), r.pose_stats()
    np.testing.assert_array_equal(_bits(T[k]), _bits(C["poses"][k]))
    assert st["ok"][k] == 0
    np.testing.assert_array_equal(_bits(T[~touch]), _bits(clean.poses()[~touch]))
    others = np.arange(n) != k
    assert np.isfinite(T).all() and (st["ok"][others & (np.arange(n) != 0)] == 1).all()
    X = r.points()
    np.testing.assert_array_equal(_bits(X[j]), _bits(C["start"][j]))  # the point step left it alone
    keep = np.arange(len(X)) != j
    np.testing.assert_array_equal(_bits(X[keep]), _bits(clean.points()[keep]))
    clean.close()
    r.close()


def test_errors_launch_nothing(native, oracle):
    C = AR.case(oracle, "synth")

    def raises(code, fn, *a, **kw):
        with pytest.raises(native.PicpError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    r = native.PointRefiner(rows=C["rows"], cols=C["cols"], K=C["K"])
    raises(native.ERR_ARG, r.set_fixed_poses, C["fixed"])  # before the poses
    raises(native.ERR_STATE, r.run_poses)
    raises(native.ERR_STATE, r.adjust)
    raises(native.ERR_STATE, r.pose_view)
    raises(native.ERR_STATE, r.poses)
    r.set_poses(C["poses"])
    raises(native.ERR_STATE, r.run_poses)  # no tracks
    r.set_tracks(C["off"], C["obs_pose"], C["obs_uv"])
    raises(native.ERR_STATE, r.adjust)     # no points
    raises(native.ERR_STATE, r.run_poses)
    r.set_points(C["start"])
    raises(native.ERR_STATE, r.pose_stats)  # no pose step yet
    r.set_fixed_poses(C["fixed"])
    raises(native.ERR_ARG, r.adjust, sweeps=-1)
    raises(native.ERR_ARG, r.adjust, points={"threshold": float("nan")})
    raises(native.ERR_ARG, r.adjust, poses={"threshold": float("nan")})
    raises(native.ERR_ARG, r.adjust, poses={"max_rounds": -1})
    raises(native.ERR_ARG, r.run_poses, damping=float("nan"))
    raises(native.ERR_ARG, r.adjust_time, 0)
    np.testing.assert_array_equal(_bits(r.points()), _bits(C["start"]))  # nothing ran
    np.testing.assert_array_equal(_bits(r.poses()), _bits(C["poses"]))
    assert r.sweeps() == []
    r.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    want = _refiner(native, C)
    want.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    np.testing.assert_array_equal(_bits(r.points()), _bits(want.points()))
    np.testing.assert_array_equal(_bits(r.poses()), _bits(want.poses()))
    # set_poses resets the mask and the records: pose 0 moves now
    r.set_poses(C["poses"])
    assert r.sweeps() == []
    r.set_points(C["start"])
    r.adjust(sweeps=1, points=AR.POINTS, poses=AR.POSES)
    assert (_bits(r.poses()[0]) != _bits(C["poses"][0])).any()
    r.close()
    want.close()


def test_adjust_time_leaves_one_adjustment(native, oracle):
    C = AR.case(oracle, "data_perturbed")
    a = _refiner(native, C)
    a.adjust(sweeps=2, points=AR.POINTS, poses=AR.POSES)
    b = _refiner(native, C)
    t = b.adjust_time(2, sweeps=2, points=AR.POINTS, poses=AR.POSES)
    print("adjust_time (build, gather, pose, point) us:", t)
    assert all(v > 0 for v in t)
    np.testing.assert_array_equal(_bits(a.points()), _bits(b.points()))
    np.testing.assert_array_equal(_bits(a.poses()), _bits(b.poses()))
    _same_stats(a.stats(), b.stats(), "point stats")
    _same_stats(a.pose_stats(), b.pose_stats(), "pose stats")
    assert a.sweeps() == b.sweeps()
    _assert_view(b, C, "after adjust_time")
    a.close()
    b.close()


# ---- 6. the solve path is untouched

def test_adjust_does_not_change_a_solve(native, oracle):
    from picp_amd import synth
    p = synth.make_problem(4099, seed=42, outlier_frac=0.3, pixel_noise=0.5)

    def solve():
        b = native.Batch([len(p["pairs"])])
        b.set_data(p["world"][p["pairs"][:, 1]], p["image"][p["pairs"][:, 0]])
        b.set_poses(p["T_init"][None])
        b.solve(threshold=3000.0, max_rounds=20, conv_eps=-1.0)
        out = b.poses().copy(), b.stats()
        b.close()
        return out

    Ta, sa = solve()
    r = _refiner(native, AR.case(oracle, "synth"))
    r.adjust(sweeps=2, points=AR.POINTS, poses=AR.POSES)
    Tb, sb = solve()
    r.close()
    np.testing.assert_array_equal(_bits(Ta), _bits(Tb))
    assert sa == sb
