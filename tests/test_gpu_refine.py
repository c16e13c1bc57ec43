"""GPU tests of the point refiner (picp_refine_*, csrc/picp_refine.hip): structure-only
Gauss-Newton of map points against all of their observations, poses fixed.

The reference is the float64 numpy restatement of tests/refine_oracle.py.  Position tolerance: per
case, D = max |X_f32 - X_f64| between the same restatement run in float32 (sequential sums, every
operation rounded) and in float64, measured on the CPU with the case's actual inputs
(tests/test_refine_cpu.py keeps the constants below honest); the GPU must stay within 4 D: its
tree-ordered FP32 sums with contraction differ from the sequential ones by rounding of the same
order, while a wrong Jacobian or gate moves points by 1e-2 m or more.

A point is borderline when, in some oracle round, one of its observations lies within 1e-3
(relative) of the chi2 gate, within 1e-3 px of an image bound or within 1e-6 of zero depth: a gate
decision may then legitimately flip in FP32, so the point is exempt from the position and count
comparison (it must still come back finite).  At most 1 % of a case's points may be exempt.
"""
import os
import subprocess

import numpy as np
import pytest

import refine_oracle as RO
from conftest import PKG

pytestmark = pytest.mark.gpu

# D per case in metres (measured on the CPU by refine_oracle.measured_d; "conv": the float32 run
# with convergence enabled against the float64 FIXED-round result).  The single-pose case is large
# because the depth of a point seen from one pose is held by the damping alone (H has the
# eigenvalue 1 along the ray against ~1e6 across it).
D = {
    "data_clean": 5.58e-06,
    "data_outliers": 9.26e-06,
    "synth_0_121": 0.0,
    "synth_1_121": 7.01e-08,
    "synth_3_121": 5.17e-07,
    "synth_4_121": 1.48e-06,
    "synth_5_121": 1.3e-06,
    "synth_15_121": 9.72e-06,
    "synth_16_121": 6.66e-06,
    "synth_17_121": 2.92e-06,
    "synth_63_121": 1.05e-05,
    "synth_64_121": 2.54e-05,
    "synth_65_121": 1.8e-05,
    "synth_257_121": 2.4e-05,
    "synth_4099_121": 0.000932,
    "synth_65_1": 0.0608,
    "synth_65_2": 1.42e-05,
    "synth_257_2": 0.000601,
    "conv": 0.00225,
    "damp0": 5.46e-05,
    "keep": 0.00174,
    "rounds1": 0.000171,
    "rounds5": 3.15e-05,
}
BORDERLINE_CAP = 0.01


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _refiner(native, case):
    r = native.PointRefiner(rows=case["rows"], cols=case["cols"], K=case["K"])
    r.set_poses(case["poses"])
    r.set_tracks(case["off"], case["obs_pose"], case["obs_uv"])
    r.set_points(case["start"])
    return r


def _run(native, name):
    case, params, X64, st, border = RO.reference(name)
    r = _refiner(native, case)
    xyz, gst = r.run(**params)
    r.close()
    return case, params, X64, st, border, xyz, gst


def _check(native, name, counts=True):
    case, params, X64, st, border, xyz, gst = _run(native, name)
    n = len(X64)
    assert xyz.shape == (n, 3) and np.isfinite(xyz).all()
    assert border.sum() <= BORDERLINE_CAP * n, (border.sum(), n)
    keep = ~border
    diff = np.abs(xyz.astype(np.float64) - X64).max(1) if n else np.zeros(0)
    worst = float(diff[keep].max()) if keep.any() else 0.0
    print("%s: n=%d borderline=%d max|gpu-oracle|=%.3g D=%.3g bound=%.3g" % (name, n, border.sum(), worst, D[name],
                                                                             4 * D[name]))
    assert worst <= 4 * D[name], (name, worst, 4 * D[name])
    if counts:
        for k in ("n_in", "n_projected", "rounds", "ok"):
            np.testing.assert_array_equal(gst[k][keep], st[k][keep], err_msg="%s %s" % (name, k))
    # a track of 0 or 1 observations: ok = 0 and the point unchanged
    short = np.diff(case["off"]) <= 1
    assert (gst["ok"][short] == 0).all() and (gst["rounds"][short] == 0).all()
    np.testing.assert_array_equal(_bits(xyz[short]), _bits(case["start"][short]))
    return case, X64, st, border, xyz, gst


def test_data_clean_matches_oracle_and_ground_truth(native):
    case, X64, st, border, xyz, gst = _check(native, "data_clean")
    assert len(X64) == 396
    err = np.linalg.norm(xyz - case["truth"], axis=1)
    print("data_clean: max |gpu - world.dat| = %.3g m" % err.max())
    assert err.max() <= 1e-3
    assert (gst["ok"] == 1).all() and (gst["rounds"] == 10).all()


def test_data_with_outliers_matches_oracle(native):
    case, X64, st, border, xyz, gst = _check(native, "data_outliers")
    assert (st["n_in"] < st["n_projected"]).sum() > 100  # the gate has work to do


@pytest.mark.parametrize("shape", RO.SHAPES, ids=["%dx%d" % s for s in RO.SHAPES])
def test_shapes(native, shape):
    case, X64, st, border, xyz, gst = _check(native, "synth_%d_%d" % shape)
    n = shape[0]
    if n >= 64 and shape[1] == 121:
        lens = np.diff(case["off"])
        for w in range(0, n - 7, 8):  # every group of 8 points (two to a wave) mixes all the lengths
            assert sorted(lens[w:w + 8]) == sorted(RO.TRACK_LENGTHS)
        assert (st["n_projected"] == 0).sum() > 0  # points behind their cameras
        assert ((st["n_projected"] > 0) & (st["n_projected"] < lens)).sum() > 0  # partly out of view


@pytest.mark.parametrize("name", ["keep", "damp0", "rounds1"])
def test_parameters(native, name):
    case, X64, st, border, xyz, gst = _check(native, name)
    if name == "rounds1":
        assert gst["rounds"].max() == 1
    if name == "keep":
        ref = RO.reference("synth_257_121")
        assert np.abs(ref[2] - X64).max() > 1e-3  # keeping the outliers changes the answer


def test_convergence_stops_early_within_tolerance(native):
    """Convergence enabled: within the tolerance of the fixed-round result, never more rounds."""
    case, X64, st, border, xyz, gst = _check(native, "conv", counts=False)
    assert (gst["rounds"] <= 10).all()
    assert (gst["converged"] == 1).sum() > 0 and (gst["rounds"][gst["converged"] == 1] < 10).any()
    assert ((gst["converged"] == 1) <= (gst["ok"] == 1)).all()


def test_two_runs_of_five_equal_one_of_ten(native):
    case, params = RO.named_case("synth_257_121")
    a = _refiner(native, case)
    a.run(**{**params, "max_rounds": 5})
    xa, sa = a.run(**{**params, "max_rounds": 5})
    b = _refiner(native, case)
    xb, sb = b.run(**params)
    np.testing.assert_array_equal(_bits(xa), _bits(xb))
    # a point that stopped in the first five rounds (too few inliers) stops again at once
    moved = sb["rounds"] == 10
    assert moved.sum() > 100
    np.testing.assert_array_equal(sa["rounds"][moved], 5)
    for k in ("n_in", "n_projected", "chi_in", "chi_out"):
        np.testing.assert_array_equal(sa[k][moved], sb[k][moved])


def test_determinism_and_time_restore(native):
    case, params = RO.named_case("synth_4099_121")
    a = _refiner(native, case)
    xa, sa = a.run(**params)
    b = _refiner(native, case)
    xb, sb = b.run(**params)
    np.testing.assert_array_equal(_bits(xa), _bits(xb))
    for k in sa:
        np.testing.assert_array_equal(sa[k], sb[k])
    c = _refiner(native, case)
    us = c.time(3, **params)
    assert us > 0.0
    np.testing.assert_array_equal(_bits(c.points()), _bits(xa))  # restored before every repetition
    for k, v in c.stats().items():
        np.testing.assert_array_equal(v, sa[k])


def test_gate_is_the_classify_gate(native):
    """picp_classify at (final point, pose) with the solver handle, summed per point, equals the
    n_in / n_projected a further one-round run reports (that run linearises at the final point)."""
    case, params = RO.named_case("synth_257_121")
    r = _refiner(native, case)
    X, _ = r.run(**params)
    _, st = r.run(**{**params, "max_rounds": 1})
    off, obs_pose, uv = case["off"], case["obs_pose"], case["obs_uv"]
    owner = np.repeat(np.arange(len(X)), np.diff(off))
    n_in = np.zeros(len(X), np.int32)
    n_proj = np.zeros(len(X), np.int32)
    s = native.PICPSolver(rows=case["rows"], cols=case["cols"], K=case["K"])
    s.setKernelThreshold(params["threshold"])
    for k in np.unique(obs_pose):
        sel = np.nonzero(obs_pose == k)[0]
        s.init(case["poses"][k], X, uv[sel])
        c = s.classify(np.stack([np.arange(len(sel)), owner[sel]], 1).astype(np.int32))
        np.add.at(n_in, owner[sel], c["state"] == native.CORR_INLIER)
        np.add.at(n_proj, owner[sel], c["state"] != native.CORR_SKIPPED)
    assert n_proj.sum() > 1000 and (n_in < n_proj).any()
    np.testing.assert_array_equal(st["n_in"], n_in)
    np.testing.assert_array_equal(st["n_projected"], n_proj)


def test_errors_launch_nothing(native):
    case, params = RO.named_case("synth_65_121")
    i64 = lambda *v: np.array(v, np.int64)
    r = native.PointRefiner(rows=case["rows"], cols=case["cols"], K=case["K"])
    with pytest.raises(native.PicpError) as e:  # wrong call order
        r.run(**params)
    assert e.value.code == native.ERR_STATE
    with pytest.raises(native.PicpError) as e:
        r.set_points(case["start"])  # before the tracks give n_points
    assert e.value.code == native.ERR_STATE
    r.set_poses(case["poses"])
    with pytest.raises(native.PicpError) as e:
        r.run(**params)
    assert e.value.code == native.ERR_STATE
    uv2 = np.zeros((2, 2), np.float32)
    for bad in (i64(1, 2, 2), i64(0, 2, 1), i64(0, 2 ** 31)):  # not from 0, decreasing, past int32
        with pytest.raises(native.PicpError) as e:
            r.set_tracks(bad, np.zeros(2, np.int32), uv2)
        assert e.value.code == native.ERR_ARG
    for idx in (-1, 121):
        with pytest.raises(native.PicpError) as e:
            r.set_tracks(i64(0, 2), np.array([0, idx], np.int32), uv2)
        assert e.value.code == native.ERR_RANGE
    r.set_tracks(case["off"], case["obs_pose"], case["obs_uv"])
    with pytest.raises(native.PicpError) as e:
        r.run(**params)  # points still missing
    assert e.value.code == native.ERR_STATE
    r.set_points(case["start"])
    r.set_poses(case["poses"][:60])  # poses set after the tracks: checked at run
    with pytest.raises(native.PicpError) as e:
        r.run(**params)
    assert e.value.code == native.ERR_RANGE
    np.testing.assert_array_equal(_bits(r.points()), _bits(case["start"]))  # nothing ran
    with pytest.raises(native.PicpError) as e:
        r.stats()
    assert e.value.code == native.ERR_STATE
    r.set_poses(case["poses"])
    xyz, _ = r.run(**params)
    np.testing.assert_array_equal(_bits(xyz), _bits(_run(native, "synth_65_121")[5]))


def test_one_shot_and_empty(native):
    case, params = RO.named_case("synth_65_121")
    xyz, st = native.refine_points(case["K"], case["rows"], case["cols"], case["poses"], case["off"],
                                   case["obs_pose"], case["obs_uv"], case["start"], **params)
    np.testing.assert_array_equal(_bits(xyz), _bits(_run(native, "synth_65_121")[5]))
    xyz, st = native.refine_points(case["K"], case["rows"], case["cols"], case["poses"], np.zeros(1, np.int64),
                                   np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros((0, 3), np.float32))
    assert xyz.shape == (0, 3) and len(st["ok"]) == 0


def test_facade_program(native, tmp_path):
    """pr::refinePoints from plain host C++ reproduces the Python result bit for bit."""
    case, params, X64, st, border, xyz, gst = _run(native, "synth_65_121")
    path = tmp_path / "problem.txt"
    with open(path, "w") as f:
        f.write("%d %d\n" % (case["rows"], case["cols"]))
        f.write(" ".join(repr(float(v)) for v in case["K"].reshape(-1)) + "\n")
        f.write("%r %r %d %d %d %r\n" % (params["threshold"], params["damping"], params["min_inliers"],
                                         params["keep_outliers"], params["max_rounds"], params["conv_eps"]))
        f.write("%d %d %d\n" % (len(case["poses"]), len(xyz), len(case["obs_pose"])))
        for T in case["poses"]:
            f.write(" ".join(repr(float(v)) for v in T.reshape(-1)) + "\n")
        f.write(" ".join(str(int(v)) for v in case["off"]) + "\n")
        for k, (u, v) in zip(case["obs_pose"], case["obs_uv"]):
            f.write("%d %r %r\n" % (k, float(u), float(v)))
        for p in case["start"]:
            f.write(" ".join(repr(float(v)) for v in p) + "\n")
    out = subprocess.run([os.path.join(PKG, "bin", "refine_main"), str(path)], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.strip().splitlines()]
    assert len(lines) == len(xyz)
    got = np.array([[int(v, 16) for v in l[2:5]] for l in lines], np.uint32)
    np.testing.assert_array_equal(got, _bits(xyz))
    cols = np.array([[int(v) for v in l[5:10]] for l in lines], np.int32)
    for j, k in enumerate(("n_in", "n_projected", "rounds", "ok", "converged")):
        np.testing.assert_array_equal(cols[:, j], gst[k])


def test_refine_does_not_change_a_solve(native):
    from picp_amd import synth
    p = synth.make_problem(4099, seed=42, outlier_frac=0.3, pixel_noise=0.5)

    def solve():
        s = native.PICPSolver()
        s.init(p["T_init"], p["world"], p["image"])
        s.setKernelThreshold(3000.0)
        st = s.solve(p["pairs"], max_rounds=20, conv_eps=-1.0)
        return s.pose().copy(), dict(st)

    Ta, sa = solve()
    _run(native, "synth_257_121")
    Tb, sb = solve()
    np.testing.assert_array_equal(_bits(Ta), _bits(Tb))
    assert sa == sb
