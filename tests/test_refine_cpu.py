"""CPU tests of the point refiner: the numpy oracle (tests/refine_oracle.py) against world.dat
and against the C oracle's error and Jacobian, the tolerances and borderline caps the GPU tests
rely on, the single-thread C++ restatement the bench tool times, the track reader, and the C-ABI's
behaviour without a device.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refine_oracle as RO
from conftest import PKG


def test_known_answer_on_the_dataset(vo):
    """396 landmarks with >= 6 observations, ground-truth poses, start 5 cm off: 10 rounds end
    within 1e-3 m of world.dat (measured 3.75e-4 m; the data are float32 text, cf. the DLT
    known-answer floor of 2.6e-4 m)."""
    case, params, X, st, border = RO.reference("data_clean")
    assert (params["max_rounds"], params["damping"], params["threshold"]) == (10, 1.0, 3000.0)
    assert len(X) == 396
    err = np.linalg.norm(X - case["truth"], axis=1)
    print("max %.3g median %.3g" % (err.max(), np.median(err)))
    assert err.max() <= 1e-3
    assert (st["ok"] == 1).all() and (st["rounds"] == 10).all()
    assert (st["n_in"] == st["n_projected"]).all()  # noise-free data: nothing is gated


def test_error_and_jacobian_match_the_c_oracle(vo, oracle):
    """Per observation: e and J = (columns 0..2 of the solver's 2x6 Jacobian) R_k."""
    case, _ = RO.named_case("data_clean")
    off, obs_pose, uv = case["off"], case["obs_pose"], case["obs_uv"]
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in range(0, 396, 40)])
    owner = np.repeat(np.arange(396), np.diff(off))[sel]
    X = case["start"][owner]
    T = case["poses"][obs_pose[sel]]
    L = RO.linearize_obs(case["K"], vo.rows, vo.cols, T[:, :3, :3], T[:, :3, 3], X, uv[sel])
    assert len(sel) > 200 and L["valid"].sum() > 150
    worst_e = worst_j = 0.0
    for q in range(len(sel)):
        ok, e, J6 = oracle.error_and_jacobian(T[q], case["K"], vo.rows, vo.cols, X[q], uv[sel][q])
        assert ok == bool(L["valid"][q])
        if not ok:
            continue
        J = J6[:, :3].astype(np.float64) @ T[q][:3, :3].astype(np.float64)
        worst_e = max(worst_e, np.abs(e - L["e"][q]).max())
        worst_j = max(worst_j, np.abs(J - L["J"][q]).max() / np.abs(L["J"][q]).max())
    print("max |e - e_oracle| = %.3g px, max relative |J - J_oracle| = %.3g" % (worst_e, worst_j))
    # the C oracle works in float32: pixels of ~640 carry 6e-5, J a few ulps of its largest entry
    assert worst_e <= 5e-4 and worst_j <= 1e-5


@pytest.mark.parametrize("name", RO.NAMES)
def test_tolerances_and_borderline_caps(name):
    """The D constants of the GPU tests are the float32-restatement distances measured here, and
    every case keeps at most 1 % of its points borderline."""
    import test_gpu_refine as G
    case, params, X, st, border = RO.reference(name)
    assert border.sum() <= G.BORDERLINE_CAP * len(X), (border.sum(), len(X))
    d = RO.measured_d(name)
    print("%s: D measured %.4g, constant %.4g" % (name, d, G.D[name]))
    assert d <= G.D[name] <= 1.02 * d + 1e-12


def test_synthetic_cases_cover_the_edges():
    case, params, X, st, border = RO.reference("synth_4099_121")
    lens = np.diff(case["off"])
    assert set(lens) == set(RO.TRACK_LENGTHS)
    assert (st["ok"][lens <= 1] == 0).all() and (X[lens <= 1] == case["start"][lens <= 1]).all()
    assert (st["n_projected"] == 0).sum() > 100           # behind the cameras
    assert ((st["n_projected"] > 0) & (st["n_projected"] < lens)).sum() > 100  # partly out of view
    assert (st["n_in"] < st["n_projected"]).sum() > 100   # gated outliers
    for npz in (1, 2):
        c, _ = RO.named_case("synth_65_%d" % npz)
        assert len(c["poses"]) == npz and set(c["obs_pose"]) == set(range(npz))
    conv = RO.run_case(RO.named_case("conv")[0], np.float64, **RO.named_case("conv")[1])[1]
    assert (conv["converged"] == 1).sum() > 100 and (conv["rounds"][conv["converged"] == 1] < 10).any()


def test_tracks_reader(vo):
    rows, off, obs_pose, obs_uv = vo.tracks()
    assert len(rows) == 491 and len(off) == 492 and off[0] == 0 and off[-1] == len(obs_pose) == len(obs_uv)
    assert len(vo.tracks(min_obs=6)[0]) == 396
    assert np.diff(off).min() >= 2 and obs_pose.dtype == np.int32 and obs_uv.dtype == np.float32
    for i in (0, 100, 490):
        fr = obs_pose[off[i]:off[i + 1]]
        assert (np.diff(fr) >= 0).all()  # sorted by frame
        sel = (vo.meas_real == vo.world_id[rows[i]])
        assert sorted(fr) == sorted(vo.meas_frame[sel])
        k = int(fr[0])
        f = vo.frame(k)
        j = np.nonzero(f["id_real"] == vo.world_id[rows[i]])[0][0]
        np.testing.assert_array_equal(obs_uv[off[i]], f["uv"][j])


def test_cpp_restatement_matches_the_oracle(tmp_path):
    """bin/refine_ref (tools/refine_ref.cpp, the single-thread baseline of tools/refine_bench.py),
    in double like the oracle: the same points to 1e-9 m and the same counts."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(PKG), "tools"))
    import refine_bench
    case, params, X, st, border = RO.reference("synth_257_121")
    path = str(tmp_path / "problem.bin")
    refine_bench.write_problem(path, case, params)
    out = str(tmp_path / "result.bin")
    res = subprocess.run([os.path.join(PKG, "bin", "refine_ref"), path, out, "1"], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    xyz, counts = refine_bench.read_result(out, len(X))
    keep = ~border
    assert np.abs(xyz - X)[keep].max() <= 1e-9
    for j, k in enumerate(("n_in", "n_projected", "rounds", "ok", "converged")):
        np.testing.assert_array_equal(counts[keep, j], st[k][keep])


def test_defaults_and_errors_without_a_device():
    import picp_amd
    L = picp_amd.lib()
    p = picp_amd.default_refine_params()
    assert (p.threshold, p.damping, p.min_inliers, p.keep_outliers, p.max_rounds) == (3000.0, 1.0, 2, 0, 10)
    assert abs(p.conv_eps - 1e-5) < 1e-12
    q = picp_amd.default_params()  # picp_params_default stays as it is
    assert (q.threshold, q.min_inliers, q.max_rounds) == (1000.0, 0, 50)
    K = picp_amd._fptr(picp_amd.k_to_c(picp_amd.K_REF))
    h = ctypes.c_void_p()
    assert L.picp_refine_create(None, 0, 480, 640, K) == picp_amd.ERR_ARG
    assert L.picp_refine_create(ctypes.byref(h), 0, 480, 640, None) == picp_amd.ERR_ARG
    assert L.picp_refine_create(ctypes.byref(h), 0, 0, 640, K) == picp_amd.ERR_ARG
    assert L.picp_refine_set_poses(None, None, 0) == picp_amd.ERR_ARG
    assert L.picp_refine_set_tracks(None, 0, None, None, None) == picp_amd.ERR_ARG
    assert L.picp_refine_set_points(None, None) == picp_amd.ERR_ARG
    assert L.picp_refine_run(None, None) == picp_amd.ERR_ARG
    assert L.picp_refine_get_points(None, None) == picp_amd.ERR_ARG
    assert L.picp_refine_get_stats(None, None) == picp_amd.ERR_ARG
    assert L.picp_refine_time(None, None, 1, None) == picp_amd.ERR_ARG
    assert L.picp_refine_destroy(None) == 0
    assert L.picp_last_error()


def test_create_without_a_device_fails_with_a_status():
    import picp_amd
    n = ctypes.c_int(-1)
    rc = picp_amd.lib().picp_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible; covered by the gpu tests")
    with pytest.raises(picp_amd.PicpError) as e:
        picp_amd.PointRefiner()
    assert e.value.code in (picp_amd.ERR_DEVICE, picp_amd.ERR_ARG)
