"""CPU tests of the Sim(3) RANSAC (picp_sim3_*): argument handling without a device, the numpy
reference (tests/sim3_ref.py) checking itself, and the closed form of csrc/picp_umeyama.h built for
the host with ASan/UBSan (bin/sim3_check) against that reference on seeded families, inputs
rounded to float32 as the device reads them.

Tolerance: the discrepancy d of sim3_ref.discrepancy (both transforms map the case's own points in
double; the largest distance over the dst cloud's extent) is held to tol = 1e-6 + 4 floor, floor
being d between the reference transform and its own float32 rounding.  Every family is strict: on
none does double rounding of the inputs alone come near the float32 floor (near_collinear sits
1e-4 of its length off the line, a conditioning of 1e4 against 1e-16).  The largest
(d - 1e-6) / floor measured per family is printed by the test and recorded in DESIGN.md §4.13;
where d < 1e-6 the ratio is negative and printed as 0.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import sim3_ref as R
from conftest import PKG, ROOT

EXE = os.path.join(PKG, "bin", "sim3_check")


def test_header_declares_the_calls():
    src = open(os.path.join(ROOT, "include", "picp_c.h")).read()
    names = ("picp_sim3_params_default", "picp_sim3_batch", "picp_sim3_batch_debug", "picp_sim3_batch_time",
             "picp_sim3_fit_batch")
    import picp_amd
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in picp_amd.EXPORTED and hasattr(picp_amd.lib(), name)
    assert "typedef struct picp_sim3_params" in src
    assert picp_amd.lib().picp_abi_version() == 3


def test_defaults():
    import picp_amd
    p = picp_amd.Sim3Params(0, 0, 0, 0, 0, 7, 5)
    picp_amd.lib().picp_sim3_params_default(ctypes.byref(p))
    assert (p.hypotheses, p.min_inliers, p.with_scale, p.refits, p.reserved, p.seed) == (256, 4, 1, 2, 0, 0)
    assert p.threshold == np.float32(0.01)
    picp_amd.lib().picp_sim3_params_default(None)  # ignored
    assert ctypes.sizeof(picp_amd.Sim3Params) == 32


def test_bad_arguments_are_rejected_without_a_device():
    import picp_amd
    L = picp_amd.lib()
    fp, i64p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
    src, dst = np.zeros(15, np.float32), np.zeros(15, np.float32)
    sp, dp = src.ctypes.data_as(fp), dst.ctypes.data_as(fp)
    S = np.zeros(16, np.float32)
    Sp = S.ctypes.data_as(fp)
    inl, fnd = ctypes.c_int32(0), ctypes.c_int32(0)
    offs = np.array([0, 5], np.int64)
    op = offs.ctypes.data_as(i64p)
    E = picp_amd.ERR_ARG

    def call(n=1, o=op, s=sp, d=dp, prm=None, S_=Sp, i=ctypes.byref(inl), f=ctypes.byref(fnd)):
        return L.picp_sim3_batch(0, n, o, s, d, ctypes.byref(prm) if prm is not None else None, S_, None, i, f, None,
                                 None)

    assert call(n=-1) == E
    assert call(o=None) == E
    assert call(s=None) == E and call(d=None) == E
    assert call(S_=None) == E and call(i=None) == E and call(f=None) == E
    bad = np.array([1, 5], np.int64)
    assert call(o=bad.ctypes.data_as(i64p)) == E
    bad = np.array([0, -1], np.int64)
    assert call(o=bad.ctypes.data_as(i64p)) == E
    for kw in (dict(hypotheses=0), dict(hypotheses=65537), dict(refits=-1), dict(refits=9),
               dict(threshold=float("nan"))):
        assert call(prm=picp_amd.default_sim3_params(**kw)) == E, kw
    assert L.picp_last_error()
    # 2^24 hypotheses per call
    many = np.zeros(258, np.int64)
    assert L.picp_sim3_batch(0, 257, many.ctypes.data_as(i64p), None, None,
                             ctypes.byref(picp_amd.default_sim3_params(hypotheses=65536)), Sp, None,
                             ctypes.byref(inl), ctypes.byref(fnd), None, None) == E
    # no problems: nothing to do, no device needed
    zero = np.zeros(1, np.int64)
    assert L.picp_sim3_batch(0, 0, zero.ctypes.data_as(i64p), None, None, None, None, None, None, None, None,
                             None) == picp_amd.OK
    assert L.picp_sim3_fit_batch(0, 0, zero.ctypes.data_as(i64p), None, None, None, 1, None, None, None,
                                 None) == picp_amd.OK
    assert L.picp_sim3_fit_batch(0, 1, op, sp, dp, None, 1, None, None, None, ctypes.byref(fnd)) == E
    assert L.picp_sim3_fit_batch(0, 1, op, sp, dp, None, 1, Sp, None, None, None) == E
    assert L.picp_sim3_fit_batch(0, 1, None, sp, dp, None, 1, Sp, None, None, ctypes.byref(fnd)) == E
    us = np.zeros(5, np.float32)
    assert L.picp_sim3_batch_time(0, 1, op, sp, dp, None, 0, us.ctypes.data_as(fp)) == E
    assert L.picp_sim3_batch_time(0, 1, op, sp, dp, None, 1, None) == E
    assert L.picp_sim3_batch_time(0, 0, op, sp, dp, None, 1, us.ctypes.data_as(fp)) == E


def test_reference_checks_itself():
    worst = R.self_check()
    print("constructed (c, R, t) recovered within %.1e" % worst)


def test_reference_inlier_test_is_strict_and_rejects_nan():
    S = np.eye(4, dtype=np.float32)
    src = np.array([[0, 0, 0], [0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0], [0, 0, 0]], np.float32)
    dst = np.array([[0.1, 0, 0], [0.05, 0, 0], [0, 0, 0], [0, 0, 0], [0, np.nan, 0]], np.float32)
    thr = np.float32(0.1) * np.float32(0.1)
    assert list(R.inlier_mask(S, src, dst, thr)) == [False, True, False, False, False]
    assert R.select([3, 5, 5, 9], [True, True, True, False]) == 1 and R.select([0, 0], [False, False]) is None


@pytest.mark.parametrize("name", R.FAMILIES)
def test_host_closed_form_against_the_reference(name, tmp_path):
    cases = list(R.family(name))
    assert len(cases) == R.N_CASES
    got, cs = R.run_check(EXE, cases, tmp_path, name)
    worst_ratio = worst_d = 0.0
    for (src, dst, ws), S, c in zip(cases, got, cs):
        ref = R.closed(src, dst, ws)
        assert ref is not None and S is not None
        M = S[:3, :3].astype(np.float64)
        assert abs(np.linalg.det(M / c) - 1) < 1e-5, "det R must be +1"  # float32 entries
        if not ws:
            assert c == 1.0
        else:
            assert abs(c / R.scale_of(ref) - 1) < 1e-5
        d, fl = R.discrepancy(ref, S, src, dst), R.floor(ref, src, dst)
        worst_d = max(worst_d, d)
        if fl > 0:
            worst_ratio = max(worst_ratio, (d - R.TOL_ABS) / fl)
        assert d <= R.TOL_ABS + R.TOL_FACTOR * fl, (name, d, fl)
    print("%s: largest discrepancy %.2e, largest (d - 1e-6) / floor %.2f" % (name, worst_d, worst_ratio))


def test_mirrored_matches_the_reference_reflection_handling(tmp_path):
    """A mirrored dst: Umeyama's sign rule, not the plain U V^T (whose determinant would be -1)."""
    cases = list(R.family("mirrored", 8))
    got, cs = R.run_check(EXE, cases, tmp_path)
    for (src, dst, ws), S, c in zip(cases, got, cs):
        Rm = S[:3, :3].astype(np.float64) / c
        assert np.linalg.det(Rm) > 0.99
        assert np.abs(Rm @ Rm.T - np.eye(3)).max() < 1e-5
        # the residual is large (no rotation fits a mirror image) and equal to the reference's
        r_ref = np.linalg.norm(R.apply(R.closed(src, dst, ws), src) - dst, axis=1).max()
        r_got = np.linalg.norm(R.apply(S, src) - dst, axis=1).max()
        assert r_ref > 0.1 and abs(r_got - r_ref) < 1e-4 * r_ref


def test_no_transform_cases_are_reported_as_such(tmp_path):
    cases = R.no_transform_cases()
    assert {"coincident", "collinear", "nan_src", "inf_dst", "zero_variance_cloud"} <= set(cases)
    for ws in (True, False):
        got, _ = R.run_check(EXE, [(s, d, ws) for s, d in cases.values()], tmp_path)
        for name, S, (s, d) in zip(cases, got, cases.values()):
            assert R.closed(s, d, ws) is None, name
            assert S is None, name


@pytest.mark.parametrize("n,seed", R.E2E_CASES)
def test_reference_pipeline_holds_every_non_outlier(n, seed):
    """The premise of the GPU robustness test (tests/test_gpu_sim3.py): with this sampler, 256
    hypotheses and threshold 0.01 the numpy reference keeps every non-outlier on each of the shared
    cases (50 % outliers uniform in the cloud's box, 1 cm noise).  No seed had to be dropped.  Its
    distance from the constructed transform is the noise's effect the GPU test allows for: the
    largest measured here is 4.3e-4 of the extent (n = 64, seed 100), 1.1e-4 at n = 500."""
    src, dst, S_true, out = R.e2e_case(n, seed)
    assert out.sum() == n // 2
    r = R.ransac(src, dst, R.E2E_THRESHOLD, 256, 4, True, 2, seed, 0)
    assert r["found"] and r["mask"][~out].all()
    noise = R.discrepancy(r["S"], S_true, src[~out], dst[~out])
    print("n=%d seed=%d: %d inliers, %.2e of the extent from the constructed transform" % (n, seed, r["inliers"], noise))
    assert noise < 1e-2  # 1 cm of noise on a cloud of some 20 m: the estimate is not far off
