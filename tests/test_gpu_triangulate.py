"""picp_triangulate (triangulate_dlt, the device function behind every map point of the VO
sequence) against an independent float64-SVD reference (tests/tri_reference.py, itself checked
against a 50-digit SVD by tests/test_triangulate_reference.py), on every point of twelve input sets
(about 400 points each; the golden pair has 74): general motion, with 0.5 px noise, a large focal
length, both cameras away from the world origin, a pair rotated 90 degrees, forward motion with
points near the epipole, baselines of 1e-2 and 1e-3, depths up to 1e5, parallax of a few float
ulps of the pixel, points at infinity, the golden pair.  No quantiles: the bounds hold per point.

  (a) |A xh| <= sigma4 + 4 EPS32 sigma1 on every point of every set;
  (b) max|xyz - ref| <= 4 EPS32 max|ref| where kappa = sigma1 / (sigma3 - sigma4) <= 1e3, on the
      seven well-conditioned sets (at least 90 % of their points must qualify);
  (c) points at infinity: a unit vector, +- the back-projection of the pixel, to 4 EPS32;
  (d) a non-finite pixel gives three NaNs and leaves the other rows' bits alone;
  (e) row i of a batch of q points has the bits of the same point triangulated alone, for q on both
      sides of the wave, the 128-thread block and several blocks;
  (f) the oracle meets (a) and (b) on the same inputs (what keeps the bounds honest).

The derivations are in tests/tri_reference.py.  The offset-world case is two sets: kappa grows with
the square of the offset, so at the offset 1e3 no point qualifies for (b) (kappa 1e4 .. 2e5) and
that set gets (a) only; (b) is checked at the offset 5, where the reference's kappa stays under 522.

Worst values observed on an MI355X (bound 4 each).  The oracle's figures are the same to the digits
shown: on the seven sets of (b) the kernel, the oracle and the reference agree bit for bit.

  set                         (|A xh| - sigma4) / (EPS32 sigma1)   direct error / EPS32   max kappa
  general                     0.499                                0                      11.1
  noise                       0.007                                0                      10.6
  large_focal                 0.438                                0                      6.21
  offset_world                0.328                                0                      522
  offset_world_1e3            0.011                                -                      1.9e5
  rotated_pair                0.488                                0                      11.5
  forward                     0.464                                0                      5.9e3 (99.8 % <= 1e3)
  short_baseline_1e-2         0.530                                -                      489
  short_baseline_1e-3_noise   0.012                                -                      1.4e5
  far                         0.420                                -                      10.1
  tiny_parallax               0.506                                -                      9.84
  infinity                    0.324  (direction error 0.25 EPS32)  -                      9.59
  golden                      0.096                                0                      18.6
"""
import numpy as np
import pytest

import tri_reference as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets():
    s = TR.input_sets()
    return {k: (v, TR.reference(v["P1"], v["P2"], v["uv1"], v["uv2"])) for k, v in s.items()}


@pytest.mark.parametrize("name", ["general", "noise", "large_focal", "offset_world", "offset_world_1e3",
                                  "rotated_pair", "forward", "short_baseline_1e-2", "short_baseline_1e-3_noise",
                                  "far", "tiny_parallax", "infinity", "golden"])
def test_triangulate_against_float64_svd(native, oracle, sets, name):
    s, ref = sets[name]
    got = native.triangulate(s["P1"], s["P2"], s["uv1"], s["uv2"])
    orc = oracle.triangulate(s["P1"], s["P2"], s["uv1"], s["uv2"])
    # print every figure before asserting
    for who, xyz in (("gpu", got), ("oracle", orc)):
        res = TR.residual_ratio(ref, xyz)
        ok = ref["kappa"] <= TR.KAPPA_MAX
        d = TR.direct_ulps(ref["xyz"][ok], xyz[ok]) if name in TR.DIRECT_SETS else np.zeros(1)
        print("TRI %-26s %-6s residual %.4f direct %.4f kappa_max %.3g share %.3f" % (
            name, who, np.nanmax(res), np.nanmax(d), ref["kappa"].max(), ok.mean()))
    TR.check_bounds(ref, orc, name, "oracle")  # (f)
    TR.check_bounds(ref, got, name, "gpu")  # (a), (b)
    if name == "infinity":  # (c)
        TR.check_infinity(s, orc, "oracle")
        print("TRI infinity gpu direction error %.4f EPS32" % TR.check_infinity(s, got, "gpu"))
    if name == "tiny_parallax":  # both sides of the FLT_EPSILON rule were exercised
        big = np.abs(got).max(1) > 1e3
        assert big.sum() >= 20 and (~big).sum() >= 20


def test_non_finite_pixels_give_nan_rows_only(native, sets):
    """(d).  Before the rule in tri_null_jacobi a NaN pixel came out as the finite point (1, 0, 0)."""
    s, _ = sets["general"]
    n = 300  # three blocks, the bad rows in different waves
    uv1, uv2 = s["uv1"][:n].copy(), s["uv2"][:n].copy()
    clean = native.triangulate(s["P1"], s["P2"], uv1, uv2)
    bad = [5, 130, 299]
    uv1[5, 0] = np.nan
    uv1[130, 1] = np.inf
    uv2[299, 0] = np.nan
    got = native.triangulate(s["P1"], s["P2"], uv1, uv2)
    assert np.isnan(got[bad]).all(), got[bad]
    keep = np.setdiff1d(np.arange(n), bad)
    np.testing.assert_array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32))
    # -Inf, and an Inf that meets a zero of P (Inf * 0) as well as non-zero entries
    uv1, uv2 = s["uv1"][:4].copy(), s["uv2"][:4].copy()
    uv1[0, 0], uv2[1, 1], uv1[2], uv2[2] = -np.inf, -np.inf, np.inf, np.nan
    got = native.triangulate(s["P1"], s["P2"], uv1, uv2)
    assert np.isnan(got[:3]).all() and np.isfinite(got[3]).all(), got
    # a non-finite P entry: every point of the call
    for k in (0, 7, 11):
        P = s["P2"].copy().reshape(-1)
        P[k] = np.nan if k != 7 else np.inf
        assert np.isnan(native.triangulate(s["P1"], P, s["uv1"][:5], s["uv2"][:5])).all(), k
        assert np.isnan(native.triangulate(P, s["P2"], s["uv1"][:5], s["uv2"][:5])).all(), k


def test_launch_shapes_bit_identical_to_single_point_calls(native, sets):
    """(e): an indexing or tail error that an all-close check forgives."""
    pool = np.concatenate([sets[k][0]["uv1"] for k in ("general", "noise")]), \
        np.concatenate([sets[k][0]["uv2"] for k in ("general", "noise")])
    s = sets["general"][0]
    rng = np.random.default_rng(5)
    # 4097 distinct points: the two sets' 800 and jittered copies of them
    uv1 = np.concatenate([pool[0]] + [(pool[0] + rng.normal(0, 2, pool[0].shape)).astype(np.float32) for _ in range(5)])
    uv2 = np.concatenate([pool[1]] + [(pool[1] + rng.normal(0, 2, pool[1].shape)).astype(np.float32) for _ in range(5)])
    uv1, uv2 = uv1[:4097], uv2[:4097]
    assert len(np.unique(np.c_[uv1, uv2], axis=0)) == 4097
    full = native.triangulate(s["P1"], s["P2"], uv1, uv2)
    assert len(np.unique(full, axis=0)) == 4097
    alone = np.concatenate([native.triangulate(s["P1"], s["P2"], uv1[i:i + 1], uv2[i:i + 1]) for i in range(4097)])
    for q in (1, 63, 64, 65, 127, 128, 129, 1000, 4097):
        got = full if q == 4097 else native.triangulate(s["P1"], s["P2"], uv1[:q], uv2[:q])
        assert got.shape == (q, 3)
        np.testing.assert_array_equal(got.view(np.uint32), alone[:q].view(np.uint32), err_msg="q=%d" % q)
