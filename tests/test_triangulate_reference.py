"""CPU checks of the triangulation reference of tests/tri_reference.py, before any kernel is held
to it: the float64 SVD against an mpmath SVD at 50 digits, and the reference itself and the oracle
(oracle.triangulate, a third method: long-double eigenvectors of A^T A) against bounds (a) and (b).
If the reference alone broke a bound on some input set, the set would be wrong, not the bound.
"""
import numpy as np
import pytest

import tri_reference as TR

U64 = 2.0 ** -53  # float64 unit roundoff


@pytest.fixture(scope="module")
def sets():
    s = TR.input_sets()
    return {k: (v, TR.reference(v["P1"], v["P2"], v["uv1"], v["uv2"])) for k, v in s.items()}


def test_input_sets_are_what_they_claim(sets):
    for name, (s, ref) in sets.items():
        n = len(s["uv1"])
        assert s["P1"].dtype == s["uv1"].dtype == s["uv2"].dtype == np.float32
        assert n >= 40 and np.isfinite(ref["xyz"]).all(), name
        if name != "golden":
            assert n == TR.N_PER_SET
        if name in TR.DIRECT_SETS:
            assert (ref["kappa"] <= TR.KAPPA_MAX).mean() >= TR.MIN_DIRECT_SHARE, (name, ref["kappa"].max())
            assert not ref["at_inf"].any(), name
    # exact data reproduces the points it was projected from
    for name in ("general", "large_focal", "offset_world", "offset_world_1e3", "rotated_pair"):
        s, ref = sets[name]
        assert np.abs(ref["xyz"] - s["X"]).max() <= 1e-3 * np.abs(s["X"]).max(), name
    # forward motion has points near the epipole, and they are the worse conditioned ones
    k = sets["forward"][1]["kappa"]
    assert k[:40].min() > np.median(k[40:])
    # tiny parallax straddles FLT_EPSILON; the points at infinity are all on the |w| <= eps side
    w = np.abs(sets["tiny_parallax"][1]["w"])
    assert (w > TR.EPS32).sum() >= 20 and (w <= TR.EPS32).sum() >= 20
    assert sets["infinity"][1]["at_inf"].all()
    assert np.array_equal(sets["infinity"][0]["uv1"].view(np.uint32), sets["infinity"][0]["uv2"].view(np.uint32))


def test_float64_svd_matches_mpmath_at_50_digits(sets):
    """40 points of each set.  numpy's SVD is backward stable: singular values within p u sigma1
    and the null vector within p u kappa of the exact ones (p: a modest constant, 64 here, u = 2^-53);
    whatever kappa, the residual of its null vector is within p u sigma1 of the exact sigma4."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    for name, (s, ref) in sets.items():
        idx = np.linspace(0, len(s["uv1"]) - 1, 40).astype(int)
        for i in idx:
            A = mp.matrix(ref["A"][i].tolist())  # float64 entries, exact in mpmath
            _, S, V = mp.svd_r(A)
            sig = np.array([float(S[k]) for k in range(4)])
            order = np.argsort(-sig)
            assert np.abs(ref["sig"][i] - sig[order]).max() <= 64 * U64 * sig.max(), (name, i)
            r64 = mp.norm(A * mp.matrix(ref["v"][i].tolist()), 2)
            assert float(r64 - S[int(order[3])]) <= 64 * U64 * sig.max(), (name, i)
            if ref["kappa"][i] <= TR.KAPPA_MAX:
                v = np.array([float(V[int(order[3]), k]) for k in range(4)])
                v = v if v @ ref["v"][i] > 0 else -v
                assert np.abs(v - ref["v"][i]).max() <= 64 * U64 * ref["kappa"][i], (name, i)


def test_reference_and_oracle_inside_bounds(sets, oracle):
    for name, (s, ref) in sets.items():
        orc = oracle.triangulate(s["P1"], s["P2"], s["uv1"], s["uv2"])
        for who, xyz in (("reference", ref["xyz"]), ("oracle", orc)):
            res, direct = TR.check_bounds(ref, xyz, name, who)
            print("%-26s %-9s residual %.3f  direct %s  kappa max %.3g" % (
                name, who, res, "-" if direct is None else "%.3f" % direct, ref["kappa"].max()))
        if name == "infinity":
            TR.check_infinity(s, ref["xyz"], "reference")
            TR.check_infinity(s, orc, "oracle")


def test_oracle_returns_nan_for_non_finite_pixels(sets, oracle):
    s, _ = sets["general"]
    uv1, uv2 = s["uv1"][:8].copy(), s["uv2"][:8].copy()
    uv1[1, 0], uv1[4, 1], uv2[6, 0] = np.nan, np.inf, np.nan
    X = oracle.triangulate(s["P1"], s["P2"], uv1, uv2)
    assert np.isnan(X[[1, 4, 6]]).all() and np.isfinite(np.delete(X, [1, 4, 6], 0)).all()
