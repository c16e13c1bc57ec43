"""CPU tests of the P3P RANSAC (picp_pnp_*, picp_relocalize): argument handling without a device,
the header, the facade driver, and the numpy reference (tests/pnp_ref.py) checking itself against
the oracle.  The GPU tests compare the device against that reference.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_ref as R
from conftest import PKG, ROOT

ROWS, COLS = 480, 640


def _no_gpu():
    import picp_amd
    n = ctypes.c_int(-1)
    rc = picp_amd.lib().picp_device_count(ctypes.byref(n))
    return not (rc == 0 and n.value > 0)


def test_header_declares_the_calls():
    src = open(os.path.join(ROOT, "include", "picp_c.h")).read()
    for name in ("picp_pnp_params_default", "picp_pnp_batch", "picp_pnp_batch_debug", "picp_pnp_batch_time",
                 "picp_relocalize"):
        assert re.search(r"\b%s\s*\(" % name, src), name
    assert "typedef struct picp_pnp_params" in src
    import picp_amd
    for name in ("picp_pnp_batch", "picp_relocalize"):
        assert name in picp_amd.EXPORTED and hasattr(picp_amd.lib(), name)


def test_defaults():
    import picp_amd
    p = picp_amd.PnpParams(0, 0, 0, 7, 5)
    picp_amd.lib().picp_pnp_params_default(ctypes.byref(p))
    assert (p.threshold, p.hypotheses, p.min_inliers, p.reserved, p.seed) == (9.0, 256, 4, 0, 0)
    picp_amd.lib().picp_pnp_params_default(None)  # ignored


def test_bad_arguments_are_rejected_without_a_device():
    import picp_amd
    L = picp_amd.lib()
    K = picp_amd.k_to_c(picp_amd.K_REF)
    Kp = K.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    i64p = ctypes.POINTER(ctypes.c_int64)
    xyz = np.zeros(15, np.float32)
    uv = np.zeros(10, np.float32)
    xp, up = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)) for a in (xyz, uv))
    T = np.zeros(16, np.float32)
    Tp = T.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    inl, fnd = ctypes.c_int32(0), ctypes.c_int32(0)
    offs = np.array([0, 5], np.int64)
    op = offs.ctypes.data_as(i64p)

    def call(n=1, o=op, x=xp, u=up, k=Kp, rows=ROWS, cols=COLS, prm=None, t=Tp, i=ctypes.byref(inl),
             f=ctypes.byref(fnd)):
        return L.picp_pnp_batch(0, n, o, x, u, k, rows, cols, prm, t, i, f, None)

    E = picp_amd.ERR_ARG
    assert call(o=None) == E and call(k=None) == E and call(x=None) == E and call(u=None) == E
    assert call(t=None) == E and call(i=None) == E and call(f=None) == E
    assert call(n=-1) == E and call(rows=0) == E and call(cols=-3) == E
    dec = np.array([0, 5, 3], np.int64)
    assert call(n=2, o=dec.ctypes.data_as(i64p)) == E
    one = np.array([1, 5], np.int64)
    assert call(o=one.ctypes.data_as(i64p)) == E
    for bad in (picp_amd.PnpParams(float("nan"), 256, 4, 0, 0), picp_amd.PnpParams(9.0, 0, 4, 0, 0),
                picp_amd.PnpParams(9.0, 65537, 4, 0, 0), picp_amd.PnpParams(9.0, -1, 4, 0, 0)):
        assert call(prm=ctypes.byref(bad)) == E
    sing = np.zeros(9, np.float32)
    assert call(k=sing.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == E
    assert L.picp_last_error()
    # an empty batch is fine, with or without a device
    assert call(n=0, x=None, u=None, t=None, i=None, f=None) == picp_amd.OK
    assert L.picp_pnp_batch_time(0, 1, op, xp, up, Kp, ROWS, COLS, None, 0, Tp) == E
    assert L.picp_pnp_batch_time(0, 1, op, xp, up, Kp, ROWS, COLS, None, 3, None) == E
    assert L.picp_relocalize(None, None, None) == E
    assert picp_amd.pnp_ransac_batch([], []) == []


def test_no_device_fails_loudly():
    import picp_amd
    if not _no_gpu():
        pytest.skip("a GPU is visible; covered by the gpu tests")
    with pytest.raises(picp_amd.PicpError) as e:
        picp_amd.pnp_ransac_batch([np.zeros((5, 3))], [np.zeros((5, 2))])
    assert e.value.code == picp_amd.ERR_DEVICE
    with pytest.raises(picp_amd.PicpError) as e:
        picp_amd.pnp_ransac_time([np.zeros((5, 3))], [np.zeros((5, 2))], 2)
    assert e.value.code == picp_amd.ERR_DEVICE


def test_facade_driver_is_built():
    exe = os.path.join(PKG, "bin", "pnp_main")
    assert os.path.exists(exe) and os.access(exe, os.X_OK)
    src = open(os.path.join(ROOT, "include", "pr", "pnp.h")).read()
    assert "inline bool localize(" in src
    assert "bool relocalize(const PnpParams& prm" in open(os.path.join(ROOT, "include", "pr", "picp_solver.h")).read()


def test_facade_compiles_without_eigen():
    """include/pr/pnp.h and the driver against the POD stand-ins of pr/defs.h (PR_NO_EIGEN)."""
    res = subprocess.run(["g++", "-DPR_NO_EIGEN", "-std=c++17", "-Wall", "-Wextra", "-Wno-ignored-qualifiers", "-Werror",
                          "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                          os.path.join(ROOT, "tests", "pnp_facade", "pnp_main.cpp")], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr


def test_quartic_root_finder_equals_the_general_one():
    """bin/poly_check (host build of csrc/picp_poly.h with ASan/UBSan): real_roots_t<4>, which the
    P3P uses, returns the bits of real_roots, which the essential unit uses, on random and
    degenerate polynomials of degree <= 4."""
    res = subprocess.run([os.path.join(PKG, "bin", "poly_check")], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 mismatches" in res.stdout, res.stdout


@pytest.mark.parametrize("n", [4, 5, 64])
def test_reference_samples_are_distinct_and_in_range(n):
    for seed in (0, 12345678901234567):
        S = R.samples(seed, 3, 257, n)
        assert S.min() >= 0 and S.max() < n
        assert all(len(set(t)) == 3 for t in S.tolist())
    assert (R.samples(0, 0, 8, 3) == 0).all()  # n < 4: no hypothesis is formed
    # every index is drawn (the skip-past step reaches the last one) and the triples depend on all inputs
    assert set(R.samples(0, 0, 257, n).ravel()) == set(range(n))
    a = R.samples(0, 0, 16, 64)
    assert not (a == R.samples(1, 0, 16, 64)).all() and not (a == R.samples(0, 1, 16, 64)).all()


@pytest.mark.parametrize("n", [8, 64])
def test_reference_p3p_recovers_noiseless_frames(oracle, n):
    from picp_amd import synth
    p = synth.make_problem(n, seed=n)
    res = R.ransac(oracle, p["xyz"], p["uv"], p["K"], ROWS, COLS, 9.0, 256)
    for h in range(256):
        assert 1 <= res["n_roots"][h] <= 4
        assert res["counts"][h][:res["n_roots"][h]].max() == n, h
    assert res["found"] and res["inliers"] == n
    assert synth.se3_log_norm(res["T"], p["T_gt"]) < 1e-4


@pytest.mark.parametrize("n,seed", R.E2E_CASES)
def test_reference_ransac_then_picp_reaches_the_near_prior_solution(oracle, n, seed):
    from picp_amd import synth
    p = synth.make_problem(n, seed=seed, outlier_frac=0.5, pixel_noise=0.5)
    res = R.ransac(oracle, p["xyz"], p["uv"], p["K"], ROWS, COLS, 9.0, 256)
    good = int((~p["outlier"]).sum())
    print("n %d seed %d: %d inliers of %d non-outliers" % (n, seed, res["inliers"], good))
    assert res["found"] and res["inliers"] >= 0.9 * good
    Ta, _ = oracle.solve(res["T"], p["K"], ROWS, COLS, p["world"], p["image"], p["pairs"], 3000.0)
    Tb, _ = oracle.solve(p["T_init"], p["K"], ROWS, COLS, p["world"], p["image"], p["pairs"], 3000.0)
    d = synth.se3_log_norm(Ta, Tb)
    print("se3(picp from ransac, picp from T_init) = %.2e" % d)
    assert d < 1e-4


def test_reference_selection_rule():
    counts = np.array([[3, 9, 0, 0], [9, 9, 0, 0], [9, 0, 0, 0]])
    assert R.select(counts, [2, 2, 1]) == (0, 1, 9)
    assert R.select(counts, [1, 2, 1]) == (1, 0, 9)
    assert R.select(counts, [0, 0, 0]) is None
    assert R.select(np.zeros((2, 4), int), [0, 1]) == (1, 0, 0)
