"""CPU tests of the P3P solver (csrc/picp_p3p.h) against an independent reference
(tests/p3p_ref.py: the conic pencil, Newton on both conics, Kabsch; nothing of Grunert's
elimination).

(a) the reference checks itself on float64-exact inputs: the constructed pose within 1e-6 px in the
    strict families, within 1e-6 px plus its own input sensitivity in the two report-only ones;
(b) bin/p3p_check, the solver's own source built for the host with ASan/UBSan, and
(c) tests/pnp_ref.py:p3p, the numpy restatement of that source,
hold on every strict family, with float32 inputs as the device reads them:
    A (nothing spurious): every pose is within tol_r of some reference root;
    B (nothing lost): every isolated reference root has a pose within tol_r;
on the probe discrepancy, tol_r = 1e-3 px + 4 floor_r (p3p_ref.ACCEPT_PX, TOL_FACTOR).  The factor
is not tuned on any output: a reference root rounded to float32 sits at floor_r by definition
((d - 1e-3) / floor_r < 1), and the largest (d - 1e-3) / floor_r the host build and the restatement
reach on the strict families is 1.00 (equal_depths_1e-4; 0.98 far and skewed_K, 0.85 generic, 0.77
triangle_10cm, 0 where the floor is far below 1e-3 px).  The parent's solver (Grunert's quartic in
v = s3/s1, no polish, no even roots) in the same harness lost 128 of 256 roots on equilateral_0 and
on equilateral_1e-6, 100 (and 45 spurious) on equilateral_1e-4, 9 (5) on equilateral_1e-2 and 61 of
132 (56 spurious) on triangle_10cm.
"""
import os

import numpy as np
import pytest

import p3p_ref as Q
import pnp_ref as R
from conftest import PKG

EXE = os.path.join(PKG, "bin", "p3p_check")


# ---------------------------------------------------------------------------------------------
# (a) the reference
# ---------------------------------------------------------------------------------------------
def _input_sensitivity(K, xyz, uv, T_root, pr, seed):
    """How far the reference's root T_root moves on the probes when every input coordinate moves by
    up to two units in its last place (four random draws, the largest movement).  The constructed
    inputs carry that much rounding themselves: the pixels are rounded once and the world points
    come out of a subtraction and three multiply-adds, so the constructed pose solves them only to
    this figure."""
    rng = np.random.default_rng([seed, 99])
    moved = 0.0
    for _ in range(4):
        x2 = xyz + rng.integers(-2, 3, xyz.shape) * np.spacing(np.abs(xyz))
        u2 = uv + rng.integers(-2, 3, uv.shape) * np.spacing(np.abs(uv))
        moved = max(moved, min([Q.probe_px(T_root, Tr, K, pr) for Tr in Q.solve(K, x2, u2)], default=np.inf))
    return moved


@pytest.mark.parametrize("name", list(Q.FAMILIES))
def test_reference_checks_itself_on_exact_inputs(name):
    """Every root is a rotation and maps the vertices onto their pixels within 1e-8 px.  The
    constructed pose is among the roots within 1e-6 px on the probes in every strict family.  In
    the two report-only families double rounding of the inputs alone moves the solution further
    than that: at 1e-6 px the constructed pose is missed in 39 of 64 near_collinear cases (the worst
    4.1e-4 px away) and in 2 of 64 triangle_1cm cases (1.5e-6 px).  There the bound is 1e-6 px plus
    four times the case's own sensitivity to its inputs' last places (_input_sensitivity; the factor
    covers the worst draw against four sampled ones); the largest (distance - 1e-6) / sensitivity
    measured is 0.99 (near_collinear) and 0.12 (triangle_1cm)."""
    K, strict = Q.FAMILIES[name][0], Q.FAMILIES[name][2]
    n_roots = missed = beyond = close = 0
    worst_hit = worst_vertex = worst_ratio = 0.0
    for i, (xyz, uv, T) in enumerate(Q.family(name, exact=True)):
        assert xyz.dtype == np.float64 and uv.dtype == np.float64
        pr = Q.probes(name, i, T)
        roots = Q.solve(K, xyz, uv)
        n_roots += len(roots)
        for j, Tr in enumerate(roots):
            assert np.isfinite(Tr).all()
            assert abs(np.linalg.det(Tr[:3, :3]) - 1) < 1e-9 and np.abs(Tr[:3, :3] @ Tr[:3, :3].T - np.eye(3)).max() < 1e-9
            worst_vertex = max(worst_vertex, R.reproj_err(Tr, K, xyz, uv).max())
            close += any(Q.probe_px(Tr, To, K, pr) <= Q.ISOLATED_PX for k, To in enumerate(roots) if k != j)
        d = [Q.probe_px(T, Tr, K, pr) for Tr in roots]
        hit = min(d, default=np.inf)
        worst_hit = max(worst_hit, hit)
        if not hit <= 1e-6:
            missed += 1
            if not strict and roots:
                moved = _input_sensitivity(K, xyz, uv, roots[int(np.argmin(d))], pr, i)
                worst_ratio = max(worst_ratio, (hit - 1e-6) / moved if moved > 0 else np.inf)
                beyond += not hit <= 1e-6 + 4.0 * moved
            else:
                beyond += 1
    print("%s: %d roots in %d cases, constructed pose further than 1e-6 px in %d (the worst %.1e px, largest "
          "(distance - 1e-6) / input sensitivity %.2f), vertices within %.1e px, %d roots not isolated"
          % (name, n_roots, Q.N_CASES, missed, worst_hit, worst_ratio, worst_vertex, close))
    assert worst_vertex <= 1e-8
    assert beyond == 0
    if strict:
        assert missed == 0
        assert close <= 0.05 * n_roots


def test_families_are_seeded_and_float32():
    for name in ("generic", "equilateral_1e-6"):
        a, b = list(Q.family(name, 3)), list(Q.family(name, 3))
        for (x0, u0, T0), (x1, u1, T1) in zip(a, b):
            assert x0.dtype == np.float32 and u0.dtype == np.float32 and x0.shape == (3, 3) and u0.shape == (3, 2)
            assert (x0 == x1).all() and (u0 == u1).all() and (T0 == T1).all()
            assert np.abs(T0[:3, 3]).max() <= 5.0
    assert len(Q.STRICT) == 11 and set(Q.REPORT_ONLY) == {"triangle_1cm", "near_collinear"}


def test_probes_tell_roots_apart_where_the_vertices_cannot():
    """Why the metric is the probes: two roots of one case agree on the vertices and not on the probes."""
    c = next(c for c in Q.cases("equilateral_0") if len(c.roots) >= 2)
    Ta, Tb = c.roots[0], c.roots[1]
    assert np.abs(Q.project(Ta, c.K, c.xyz.astype(np.float64)) - Q.project(Tb, c.K, c.xyz.astype(np.float64))).max() < 1e-8
    assert Q.probe_px(Ta, Tb, c.K, c.probes) > Q.ISOLATED_PX


# ---------------------------------------------------------------------------------------------
# (b), (c) the solver's source on the host and its restatement
# ---------------------------------------------------------------------------------------------
def _tally(name, label, poses_of):
    cs = Q.cases(name)
    spurious = lost = n = 0
    worst = 0.0
    for i, c in enumerate(cs):
        poses = poses_of(i, c)
        assert len(poses) <= 4 and all(np.isfinite(T).all() for T in poses)
        n += len(poses)
        s, l, w = c.compare(poses)
        spurious, lost, worst = spurious + s, lost + l, max(worst, w)
    print("%s, %s: %d poses for %d reference roots, %d spurious, %d lost, worst (d - 1e-3) / floor %.2f"
          % (name, label, n, sum(len(c.roots) for c in cs), spurious, lost, worst))
    return spurious, lost


@pytest.fixture(scope="module")
def host_poses(tmp_path_factory):
    """bin/p3p_check once on every case of every family."""
    names = list(Q.FAMILIES)
    tri = [(c.K, c.xyz, c.uv) for name in names for c in Q.cases(name)]
    out = Q.run_p3p_check(EXE, tmp_path_factory.mktemp("p3p") / "cases.txt", tri)
    return {name: out[k * Q.N_CASES:(k + 1) * Q.N_CASES] for k, name in enumerate(names)}


@pytest.mark.parametrize("name", Q.STRICT)
def test_host_build_holds_the_reference_root_set(host_poses, name):
    spurious, lost = _tally(name, "bin/p3p_check", lambda i, c: [Q.pose12(p) for p in host_poses[name][i]])
    assert spurious == 0  # A
    assert lost == 0      # B
    assert any(len(c.roots) >= 3 for c in Q.cases(name))


@pytest.mark.parametrize("name", Q.REPORT_ONLY)
def test_host_build_on_the_report_only_families(host_poses, name):
    """Float32 rounding moves these families' exact solutions by pixels: the numbers are printed,
    only finiteness is asserted (in _tally)."""
    _tally(name, "bin/p3p_check", lambda i, c: [Q.pose12(p) for p in host_poses[name][i]])


def _restated(i, c):
    return [Q.rounded(T) for T in R.p3p(c.xyz.astype(np.float64), R.bearings(c.K, c.uv), c.K, c.uv)]


@pytest.mark.parametrize("name", Q.STRICT)
def test_restatement_holds_the_reference_root_set(name):
    spurious, lost = _tally(name, "pnp_ref.p3p", _restated)
    assert spurious == 0  # A
    assert lost == 0      # B


@pytest.mark.parametrize("name", Q.REPORT_ONLY)
def test_restatement_on_the_report_only_families(name):
    _tally(name, "pnp_ref.p3p", _restated)


def test_host_build_rejects_degenerate_triangles(tmp_path):
    c = Q.cases("generic")[0]
    twin, line, nan = c.xyz.copy(), c.xyz.copy(), c.uv.copy()
    twin[1] = twin[0]
    line[2] = 0.5 * (line[0] + line[1])
    nan[1, 0] = np.nan
    out = Q.run_p3p_check(EXE, tmp_path / "deg.txt", [(c.K, twin, c.uv), (c.K, line, c.uv), (c.K, c.xyz, nan),
                                                      (c.K, c.xyz, c.uv)])
    assert [len(p) for p in out[:3]] == [0, 0, 0] and len(out[3]) == len(c.roots)
