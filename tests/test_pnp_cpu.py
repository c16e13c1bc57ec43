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


# ---------------------------------------------------------------------------------------------
# the root finders against known roots (bin/poly_check --roots)
# ---------------------------------------------------------------------------------------------
def _finder_roots(tmp_path, polys):
    """real_roots, for degree <= 4 real_roots_t<4> and for quartics the P3P's p3p_quartic_roots on
    ascending coefficient lists -> per polynomial (general, quartic or None, p3p or None)."""
    path = tmp_path / "polys.txt"
    path.write_text("".join(" ".join(float(x).hex() for x in c) + "\n" for c in polys))
    res = subprocess.run([os.path.join(PKG, "bin", "poly_check"), "--roots", str(path)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = []
    for line in res.stdout.strip().splitlines():
        groups = [g.split() for g in line.split("|")]
        groups[0] = groups[0][1:]  # the degree
        found = [np.array([float.fromhex(t) for t in g[1:]]) for g in groups]
        assert all(len(f) == int(g[0]) for f, g in zip(found, groups))
        out.append(tuple(found + [None] * (3 - len(found))))
    assert len(out) == len(polys)
    return out


def _from_roots(r64, e, sign):
    """sign * 2^e * prod (x - r / 64), r integers: integer arithmetic, each coefficient rounded once."""
    from fractions import Fraction
    c = [1]
    for ri in r64:  # ascending coefficients of prod (64 x - r)
        c = [(64 * c[j - 1] if j > 0 else 0) - (int(ri) * c[j] if j < len(c) else 0) for j in range(len(c) + 1)]
    return [sign * float(Fraction(x) * Fraction(2) ** (e - 6 * len(r64))) for x in c]


# Largest ratio measured: 2.29 (degree 4) and 5.65 (degree 10) on these 64 + 64 polynomials, at
# most 7.6 over six other seeds; the median is 0.17 at degree 10 (the bisection ends on the computed polynomial's sign
# change, numpy.roots on the eigenvalues of a balanced companion matrix).
ROOT_ERROR_VS_NUMPY = 16.0


@pytest.mark.parametrize("d", [4, 10])
def test_root_finders_return_the_known_roots(tmp_path, d):
    """Polynomials built from d real roots in [-10, 10], pairwise >= 0.1 apart, every other one with
    its leading coefficient scaled over +-20 binades: every root is returned, none extra, with an
    error of at most 16 times numpy.roots' own on the same polynomial."""
    rng = np.random.default_rng(d)
    cases = []
    for k in range(64):
        while True:
            r = np.sort(rng.integers(-640, 641, d))
            if np.diff(r).min() >= 7:  # 7 / 64 > 0.1
                break
        cases.append((r / 64.0, _from_roots(r, int(rng.integers(-20, 21)) if k % 2 else 0, -1 if k % 4 >= 2 else 1)))
    worst = 0.0
    worst_p3p = 0.0
    for (r, c), (general, quartic, p3p) in zip(cases, _finder_roots(tmp_path, [c for _, c in cases])):
        assert len(general) == d and (np.diff(general) > 0).all()
        err_np = np.abs(np.sort(np.roots(c[::-1]).real) - r).max()
        if d <= 4:
            assert quartic is not None and general.tobytes() == quartic.tobytes()
            # the P3P's own last level (csrc/picp_p3p.h p3p_quartic_roots): the same roots, the same bound
            assert p3p is not None and len(p3p) == d and (np.diff(p3p) > 0).all()
            assert np.abs(p3p - r).max() <= ROOT_ERROR_VS_NUMPY * err_np, (r, p3p)
            worst_p3p = max(worst_p3p, np.abs(p3p - r).max() / err_np if err_np > 0 else 0.0)
        err = np.abs(general - r).max()
        assert err <= ROOT_ERROR_VS_NUMPY * err_np, (r, err, err_np)
        worst = max(worst, err / err_np if err_np > 0 else 0.0)
    print("degree %d: largest error ratio to numpy.roots %.2f (p3p_quartic_roots %.2f)" % (d, worst, worst_p3p))


def test_root_finders_may_miss_a_double_root(tmp_path):
    """The documented blind spot: a root of even multiplicity has no sign change, so the bisection
    may return it twice, once or not at all (csrc/picp_p3p.h looks at the quartic's critical points
    for that reason).  The simple roots are still returned and nothing else is."""
    r = np.array([-128, 64, 64, 192])  # (x + 2) (x - 1)^2 (x - 3)
    (general, quartic, p3p), = _finder_roots(tmp_path, [_from_roots(r, 0, 1)])
    assert general.tobytes() == quartic.tobytes()
    assert all(np.abs(g - np.array([-2.0, 1.0, 3.0])).min() < 1e-6 for g in p3p)
    assert np.abs(p3p + 2).min() < 1e-12 and np.abs(p3p - 3).min() < 1e-12
    assert all(np.abs(g - np.array([-2.0, 1.0, 3.0])).min() < 1e-6 for g in general)
    assert np.abs(general + 2).min() < 1e-12 and np.abs(general - 3).min() < 1e-12
    print("double root at 1: returned %d times" % int((np.abs(general - 1) < 1e-6).sum()))
    assert (np.abs(general - 1) < 1e-6).sum() <= 2
