"""The preconditions of tests/test_gpu_edge_inputs.py, held on the CPU oracle alone.

Every GPU assertion there has the form "the oracle does not see this replacement, so the GPU must
not either" or "the oracle makes this of the item, so the GPU must too".  This module proves the
oracle's half for every family of tests/edge_inputs.py, every camera and both keep flags, with no
case exempt: what the float32 gate makes of each item (the numpy restatement that
test_gpu_classify.py proves equal to the oracle, and the per-point oracle itself), and which of
the oracle's linearize / solve outputs are bit-identical between the clean and the edge variant.
"""
import numpy as np
import pytest

import edge_inputs as E
from test_gpu_classify import _np_classify, _oracle_classify

KS = {"pinhole": E.K_PIN, "skew": E.K_SKEW}
SIZES = [1, 65, 4099]
ROUNDS = {"depth": 1, "free": 3}  # the rounds the GPU test solves for


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits64(a), _bits64(b))


def _lin(O, T, K, rows, keep):
    return O.linearize_soa(T, K, E.ROWS, E.COLS, *E.soa(rows), E.THR, keep_outliers=keep, mode=O.MODE_F64)


def _solve(O, T, K, rows, keep, R):
    T1, st = O.solve_soa(T, K, E.ROWS, E.COLS, *E.soa(rows), E.THR, keep_outliers=keep, mode=O.MODE_F64,
                         max_rounds=R, conv_eps=-1.0)
    return T1, st


def _poses(p):
    return [p["T0"]] if p["base"] == "depth" else [p["T0"], p["T1"], E.nearby(p["T0"], 99)]


def test_slot_positions():
    """Lane 0 and lane 63 of a wave, a lone item in its wave, a (k, k + 1) pair of one lane for
    every block size, the last item of a ragged problem; in a batch the last item of one frame and
    the first of the next."""
    for n in (4099, 100003, 1000003):
        s = set(E.slots(n).tolist())
        assert {0, 63, 128, 191, n - 1} <= s and n % 64 and n % 512
        assert 261 in s and not any(k in s for k in range(256, 320) if k != 261)  # alone in its wave
        for bs in (256, 512, 1024):
            assert 5 in s and 5 + bs in s
    assert E.slots(1).tolist() == [0] and E.slots(65).tolist() == [0, 5, 63, 64]
    b = E.make_batch("depth", [0, 1, 5, 257, 4099])
    assert b["frames"][0] is None and len(b["clean"]) == sum(b["sizes"])
    for fr in b["frames"][1:]:
        assert fr["slots"][0] == 0 and fr["slots"][-1] == fr["n"] - 1


def test_depth_items_sit_on_their_depth_bits():
    """The signed-permutation pose with a -0 translation makes R p + t exact: every item of the
    depth base has the intended camera-frame depth bit for bit (-0 and the subnormal included)."""
    want = {0x00000000, 0x80000000, int(np.float32(1e-40).view(np.uint32)),
            int((np.float32(2.0) ** -101).view(np.uint32)), int((np.float32(2.0) ** 101).view(np.uint32))}
    seen = set()
    for (base, _), items in E.FAMILIES.items():
        if base == "depth":
            seen |= {int(E._bits(E.depth_f32(E.T_PERM, *it[:3]))[0]) for it in items}
    assert want <= seen
    E.make("depth", 4099)  # asserts the bits of every slot


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("fam", sorted(E.FAMILIES), ids=["%s-%s" % f for f in sorted(E.FAMILIES)])
def test_family_states(oracle, fam, kname):
    """What the gate makes of every item: skipped / outlier / inlier as EXPECTED_STATE says, by the
    numpy restatement and by the oracle point by point; chi2 is inf for the overflowing
    measurements and NaN for the NaN family (NaN passes every comparison: an inlier)."""
    base, name = fam
    rows = np.stack(E.FAMILIES[fam])
    p = E.make(base, 65)
    for T in _poses(p):
        st, chi, uv = _np_classify(T, KS[kname], rows[:, :3], rows[:, 3:], E.THR)
        np.testing.assert_array_equal(st, E.EXPECTED_STATE[fam])
        with np.errstate(all="ignore"):
            so, co, uo = _oracle_classify(oracle, T, KS[kname], rows[:, :3], rows[:, 3:], E.THR)
        np.testing.assert_array_equal(so, st)
        np.testing.assert_array_equal(np.isnan(co), np.isnan(chi))
        np.testing.assert_array_equal(co[~np.isnan(co)], chi[~np.isnan(chi)])
        if fam == ("free", "out"):
            assert np.isposinf(chi).all()
        if fam == ("free", "nan"):
            assert np.isnan(chi).all()
        if fam == ("depth", "out"):
            assert np.isfinite(chi).all()


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("base", ["depth", "free"])
def test_skipped_items_are_invisible_to_the_oracle(oracle, base, n, keep, kname):
    """Replacing a skipped ordinary point by a skipped extreme one changes nothing the oracle
    returns: linearize (H, b, chi_in, chi_out, n_in, n_projected) and a solve (pose, statistics),
    bit for bit, for keep_outliers 0 and 1.  The free base at T0 and two nearby poses and solved
    for 3 rounds, the depth base at T0 and for 1 round."""
    K = KS[kname]
    for shift in range(len(E.FAMILIES[base, "skip"]) if n < 100 else 1):
        p = E.make(base, n, shift=shift)
        for T in _poses(p):
            a, b = _lin(oracle, T, K, p["clean"], keep), _lin(oracle, T, K, p["skip"], keep)
            for k in ("H", "b", "chi_in", "chi_out"):
                assert _same(a[k], b[k]), k
            assert (a["n_in"], a["n_projected"]) == (b["n_in"], b["n_projected"])
            assert np.isfinite(b["H"]).all() and np.isfinite(b["b"]).all()
        Ts = p["T0"] if base == "depth" else p["T1"]
        (Ta, sa), (Tb, sb) = (_solve(oracle, Ts, K, p[v], keep, ROUNDS[base]) for v in ("clean", "skip"))
        np.testing.assert_array_equal(Ta.view(np.uint32), Tb.view(np.uint32))
        assert sa == sb and sb["ok"] == 1


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("base", ["depth", "free"])
def test_valid_outliers_leave_the_inlier_sums_alone(oracle, base, n, kname):
    """The valid-outlier families with keep_outliers = 0: H, b, n_in and chi_in are bit-identical to
    the clean variant, n_projected grows by the number of slots, chi_out is inf for the overflowing
    measurements and finite for the extreme depths; a solve returns the same pose.  (With
    keep_outliers = 1 the oracle's own sums are non-finite or swamped: not a reference.)"""
    K = KS[kname]
    p = E.make(base, n)
    for T in _poses(p):
        a, b = _lin(oracle, T, K, p["clean"], 0), _lin(oracle, T, K, p["out"], 0)
        for k in ("H", "b", "chi_in"):
            assert _same(a[k], b[k]), k
        assert a["n_in"] == b["n_in"] and b["n_projected"] == a["n_projected"] + len(p["slots"])
        assert np.isposinf(b["chi_out"]) if base == "free" else np.isfinite(b["chi_out"])
    Ts = p["T0"] if base == "depth" else p["T1"]
    (Ta, sa), (Tb, sb) = (_solve(oracle, Ts, K, p[v], 0, ROUNDS[base]) for v in ("clean", "out"))
    np.testing.assert_array_equal(Ta.view(np.uint32), Tb.view(np.uint32))
    assert (sa["n_in"], sa["chi_in"], sa["ok"]) == (sb["n_in"], sb["chi_in"], sb["ok"])


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("base", ["depth", "free"])
def test_ordinary_outliers_in_the_slots_leave_the_inlier_sums_alone(oracle, base, n, kname):
    """The second clean variant (an ordinary projectable outlier in every slot), keep_outliers = 0:
    every slot is a projected outlier with a finite chi at every pose, and H, b, n_in, chi_in and
    the solved pose are bit-identical to the clean variant's -- so also to the skip and out
    families'."""
    K = KS[kname]
    p = E.make(base, n)
    for T in _poses(p):
        st, chi, _ = _np_classify(T, K, p["clean_out"][p["slots"], :3], p["clean_out"][p["slots"], 3:], E.THR)
        assert (st == 2).all() and np.isfinite(chi).all()
        a, b = _lin(oracle, T, K, p["clean"], 0), _lin(oracle, T, K, p["clean_out"], 0)
        for k in ("H", "b", "chi_in"):
            assert _same(a[k], b[k]), k
        assert a["n_in"] == b["n_in"] and b["n_projected"] == a["n_projected"] + len(p["slots"])
    Ts = p["T0"] if base == "depth" else p["T1"]
    (Ta, sa), (Tb, sb) = (_solve(oracle, Ts, K, p[v], 0, ROUNDS[base]) for v in ("clean", "clean_out"))
    np.testing.assert_array_equal(Ta.view(np.uint32), Tb.view(np.uint32))
    assert (sa["n_in"], sa["chi_in"], sa["ok"]) == (sb["n_in"], sb["chi_in"], sb["ok"])


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("keep", [0, 1])
def test_tiny_depth_inliers_overflow_the_reference_too(oracle, keep, kname):
    """A projectable point at a depth under 2^-100 is an inlier at the gate (n_in and n_projected
    grow by one per slot) and its J^2 overflows float32 in the reference's own sums: H is not
    finite, so the GPU test checks these items at the gate only."""
    p = E.make("depth", 4099)
    a, b = _lin(oracle, p["T0"], KS[kname], p["clean"], keep), _lin(oracle, p["T0"], KS[kname], p["tiny_in"], keep)
    m = len(p["slots"])
    assert (b["n_in"], b["n_projected"]) == (a["n_in"] + m, a["n_projected"] + m)
    assert not np.isfinite(b["H"]).all()


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_nan_passes_in_the_oracle(oracle, n, keep, kname):
    """NaN passes, as in the reference: every NaN item is an inlier (n_in and n_projected grow by
    one per slot), all 36 entries of H, b and chi_in are NaN, and a 2-round solve returns a NaN
    pose with ok = 1 and, the second round being evaluated at a NaN pose, n_in = n."""
    K = KS[kname]
    p = E.make("free", n)
    m = len(p["slots"])
    for T in _poses(p):
        a, b = _lin(oracle, T, K, p["clean"], keep), _lin(oracle, T, K, p["nan"], keep)
        assert (b["n_in"], b["n_projected"]) == (a["n_in"] + m, a["n_projected"] + m)
        assert np.isnan(b["H"]).all() and np.isnan(b["b"]).all() and np.isnan(b["chi_in"])
    Tn, st = _solve(oracle, p["T1"], K, p["nan"], keep, 2)
    assert np.isnan(Tn[:3, :]).all() and st["ok"] == 1 and st["n_in"] == n


REFINE_ROUNDS = {"tied": 1, "free": 10, "nan": 10}


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", sorted(REFINE_ROUNDS))
def test_refiner_replacements_are_invisible_to_the_restatement(name, dtype):
    """The refiner's restatement (tests/refine_oracle.py), in float64 and with every operation in
    float32: replacing a skipped observation by one at the depth +0, -0, 1e-40 (first round) or
    3e38 (every round) leaves every point and its n_in, chi_in, ok and rounds unchanged, bit for
    bit; so does moving ANOTHER point's start to +-3e38 or NaN.  (In float64 the 3e38-depth
    observation does not overflow and counts as a projected outlier: n_projected and chi_out are
    not part of the statement.)  With the float32 gate, which is the kernel's, a point at +-3e38
    has no projectable observation (ok = 0, unchanged); a NaN point passes every gate as an inlier
    and fails the solve (ok = 0, unchanged)."""
    import refine_oracle as RO
    c = E.refine_case()
    prm = {**RO.BASE, "max_rounds": REFINE_ROUNDS[name]}
    Xc, sc, _ = RO.run_case(c["clean"], dtype, **prm)
    Xe, se, _ = RO.run_case(c[name], dtype, **prm)
    keep = np.ones(len(Xc), bool)
    keep[c["moved"][name]] = False
    assert np.isfinite(Xc).all()
    assert np.array_equal(Xc[keep], Xe[keep])
    for k in ("n_in", "chi_in", "ok", "rounds"):
        np.testing.assert_array_equal(sc[k][keep], se[k][keep], err_msg=k)
    hosts = c["hosts"][:3] if name == "tied" else c["hosts"][3:]
    assert (sc["ok"][hosts] == 1).all() and (sc["n_in"][hosts] >= 10).all()  # the hosts are being refined
    for i in c["moved"][name]:
        if dtype == np.float32:
            assert se["ok"][i] == 0 and se["rounds"][i] == 0
            assert np.array_equal(Xe[i].view(np.uint32), c[name]["start"][i].view(np.uint32))
        if name == "nan":
            assert se["ok"][i] == 0 and se["n_in"][i] == se["n_projected"][i] == np.diff(c[name]["off"])[i]
