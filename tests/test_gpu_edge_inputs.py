"""GPU tests of the solve, classify and refine kernels on extreme and NaN inputs
(tests/edge_inputs.py; the oracle's half of every statement is tests/test_edge_inputs_cpu.py).

The per-correspondence code of picp_item.h has four wave-level branches that depend on the
VALUES of the data.  The cases below take each of them the rare way:

  1. The reciprocal of the depth: accumulate_pinhole2 (RCP_CHECK), accumulate_regs,
     accumulate_regs1 and accumulate_item vote on rcp_safe(depth); one lane whose camera-frame depth
     is 0, subnormal, 2^-101 or 2^101 (the depth base's "skip", "out" and "tiny_in" families), or inf
     or NaN (the free base's "nan" family), sends the whole wave from rcp_rn (RCP_FAST) to the IEEE
     division (RCP_DIV), for every item of the set.
  2. The zeroing of skipped items: accumulate_pinhole votes on "every skipped lane projects from a
     depth >= 1e-12 with a finite chi" and zeroes iz alone or all eight inputs; accumulate_one,
     item_general, accumulate_pinhole2 (PICP_Z2) and the refiner always zero.  A skipped lane with an
     infinite iz (depth +-0, 1e-40), an overflowed ph (x = 3e38, depth 3e38), a depth under 1e-12
     (the "out" family's on-axis 1e-13 ... 2^-101 with keep_outliers = 0) or an infinite chi (the free
     base's "out" family: u = 1e20 ... inf, keep_outliers = 0) takes the all-eight side.
  3. NaN passes as in the reference: the "nan" family through classify, linearize and a solve.
  4. Padding lanes recompute a copy of a real item with in_range = false: every variant puts an
     edge item LAST (slot n - 1, n not a multiple of 64), so up to 63 further lanes evaluate it.

Three kinds of assertion:

  * replacement invariance (bit-exact, no tolerance): where the oracle's outputs are identical
    between the clean and the edge variant, the GPU's are too -- all of linearize and of a solve
    for the "skip" families with keep_outliers 0 and 1; H, b, n_in and chi_in (and the solved pose)
    for the "out" families with keep_outliers = 0.  A wave that holds an edge item takes RCP_DIV
    where the same wave of the clean variant takes RCP_FAST: equal bits prove the two reciprocals
    equal in place, and that a dangerous skipped lane (an infinite iz, ph, e or chi) leaks nothing.
    The clean variant's slots (points behind the camera) do not project, so its waves take the
    all-eight zeroing like the edge waves; with keep_outliers = 0 a second clean variant,
    "clean_out", holds ordinary projectable outliers there, which take the iz-only side: its H, b,
    n_in and chi_in are bit-identical too, which compares the two sides of the zeroing vote on
    purpose;
  * oracle parity: every finite result also within the rules of test_gpu_parity (_lin_close,
    _pose_tol, exact counts);
  * NaN passes: single solver in graph mode only (no NaN runs in persistent or block mode: nobody has
    read the spin-wait code for a NaN, and this suite does not go looking for hangs).
"""
import contextlib
import os

import numpy as np
import pytest

import edge_inputs as E
from test_gpu_classify import _np_classify
from test_gpu_parity import _assert_n_in_explained, _batch_mode, _lin_close, _pose_tol

pytestmark = pytest.mark.gpu

KS = {"pinhole": E.K_PIN, "skew": E.K_SKEW}
THR = E.THR


def _synth():
    from picp_amd import synth
    return synth


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _b32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _ident(n):
    return np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)


def _solver(native, K, rows, T):
    s = native.PICPSolver(rows=E.ROWS, cols=E.COLS, K=K)
    s.init(T, rows[:, :3], rows[:, 3:])
    s.setKernelThreshold(THR)
    return s


def _lin(s, rows, T, keep):
    """linearize of `rows` at T on the solver s (one solver serves a whole test)."""
    s.init(T, rows[:, :3], rows[:, 3:])
    return s.linearize(_ident(len(rows)), keep_outliers=bool(keep))


def _ref_lin(O, K, rows, T, keep):
    return O.linearize_soa(T, K, E.ROWS, E.COLS, *E.soa(rows), THR, keep_outliers=keep, mode=O.MODE_F64)


def _assert_same_lin(a, b, keys=("H", "b", "chi_in", "chi_out", "n_in", "n_projected")):
    for k in keys:
        if k in ("n_in", "n_projected"):
            assert a[k] == b[k], k
        else:
            np.testing.assert_array_equal(_b64(a[k]), _b64(b[k]), err_msg=k)


def _check_linearize(s, O, K, p, T, keep):
    """clean vs every family of p at pose T: invariance, then oracle parity."""
    clean = _lin(s, p["clean"], T, keep)
    ref = _ref_lin(O, K, p["clean"], T, keep)
    assert (clean["n_in"], clean["n_projected"]) == (ref["n_in"], ref["n_projected"])
    _lin_close(clean, ref)
    # skipped extremes: everything, bit for bit; the oracle's edge result is the clean one
    # (test_skipped_items_are_invisible_to_the_oracle)
    got = _lin(s, p["skip"], T, keep)
    _assert_same_lin(got, clean)
    if not keep:  # projectable outliers in the slots: the iz-only side of the zeroing vote
        got = _lin(s, p["clean_out"], T, keep)
        rc = _ref_lin(O, K, p["clean_out"], T, keep)
        _assert_same_lin(got, clean, ("H", "b", "chi_in", "n_in"))
        assert got["n_projected"] == rc["n_projected"]
        _lin_close(got, rc)
    # valid outliers: the inlier sums bit for bit with keep_outliers = 0; the gate always
    got = _lin(s, p["out"], T, keep)
    ro = _ref_lin(O, K, p["out"], T, keep)
    assert (got["n_in"], got["n_projected"]) == (ro["n_in"], ro["n_projected"])
    if not keep:
        _assert_same_lin(got, clean, ("H", "b", "chi_in", "n_in"))
        if np.isinf(ro["chi_out"]):
            assert np.isposinf(got["chi_out"])
        else:
            _lin_close(got, ro)
    if "tiny_in" in p:
        # valid tiny-depth inliers: J^2 overflows float32 in the reference's own Matrix6f sums
        # (test_tiny_depth_inliers_overflow_the_reference_too), so H, b and chi are NOT compared:
        # the gate only
        got = _lin(s, p["tiny_in"], T, keep)
        ro = _ref_lin(O, K, p["tiny_in"], T, keep)
        assert (got["n_in"], got["n_projected"]) == (ro["n_in"], ro["n_projected"])


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 4099])
@pytest.mark.parametrize("base", ["depth", "free"])
def test_single_linearize(native, oracle, base, n, keep, kname):
    """Single-solver linearize (the round kernel's pair form: accumulate_pinhole2 with its per-pair
    RCP_CHECK vote and PICP_Z2 zeroing for the pinhole K, item_general for the skewed K), n = 1
    (63 padding lanes copy the one, dangerous, item), 65 (an edge item alone in wave 1, and last)
    and 4099.  At n < 100 every item of the skip family takes every slot in turn."""
    K = KS[kname]
    shifts = len(E.FAMILIES[base, "skip"]) if n < 100 else 1
    s = native.PICPSolver(rows=E.ROWS, cols=E.COLS, K=K)
    s.setKernelThreshold(THR)
    for shift in range(shifts):
        p = E.make(base, n, shift=shift)
        for T in ([p["T0"]] if base == "depth" else [p["T0"], p["T1"]]):
            _check_linearize(s, oracle, K, p, T, keep)
    s.close()


@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("base", ["depth", "free"])
def test_streaming_linearize(native, oracle, base, keep):
    """Graph mode with float4 lanes (more than 2^18 items, as
    test_streaming_sweep_directions_ragged_tail): four consecutive items per lane, the
    ragged tail (masked items behind the last -- edge -- item)."""
    n = 300003
    p = E.make(base, n)
    with _env(PICP_MODE="graph"):
        s = native.PICPSolver(rows=E.ROWS, cols=E.COLS, K=E.K_PIN)
        s.setKernelThreshold(THR)
        _check_linearize(s, oracle, E.K_PIN, p, p["T0"], keep)
        s.close()


def _solve_single(native, K, rows, T, R, keep):
    s = _solver(native, K, rows, T)
    st = s.solve(_ident(len(rows)), max_rounds=R, conv_eps=-1.0, keep_outliers=bool(keep))
    T1 = s.pose()
    s.close()
    return T1, dict(st)


def _solve_batch(native, mode, bt, variant, Ts, R, keep, split=None, K=None, grid=None):
    """grid: the hand-off grid the layout must have (block mode: 8 x split blocks for up to 8
    frames, 0 unsplit), so that a split the runtime did not grant fails the test."""
    kw = {} if K is None else {"K": K}
    with _env(PICP_BLOCK_SPLIT=split):
        b = _batch_mode(native, bt["sizes"], mode, **kw)
        assert b.info()["mode"] == mode
        if grid is not None:
            assert b.residency()["handoff_grid"] == grid, (b.residency(), grid)
        rows = bt[variant]
        b.set_data(rows[:, :3], rows[:, 3:])
        b.set_poses(Ts)
        b.solve(threshold=THR, max_rounds=R, conv_eps=-1.0, keep_outliers=keep)
        out = b.poses(), b.stats()
        b.close()
    return out


def _assert_stats_equal(a, b, keys):
    """The statistics of two batch solves, frame by frame: integers equal, floats bit for bit."""
    for i, (sa, sb) in enumerate(zip(a, b)):
        for k in keys:
            if isinstance(sa[k], float):
                assert _b32(sa[k])[0] == _b32(sb[k])[0], (i, k, sa[k], sb[k])
            else:
                assert sa[k] == sb[k], (i, k, sa[k], sb[k])


ALL_STATS = ("chi_in", "chi_out", "n_in", "ok", "rounds", "converged", "n_projected")


def _check_batch(native, O, mode, base, sizes, keep, split=None, K=None, seed=0, grid=None):
    """A batch solve of the clean, the skip and (keep_outliers = 0) the out variant from the base's
    start poses: invariance between the variants, then every frame against the oracle."""
    bt = E.make_batch(base, sizes, seed=seed)
    R = 1 if base == "depth" else 3
    Ts = np.stack([fr["T0"] if base == "depth" else fr["T1"] for fr in bt["frames"]])
    Kn = E.K_PIN if K is None else K
    Pc, Sc = _solve_batch(native, mode, bt, "clean", Ts, R, keep, split, K, grid)
    Ps, Ss = _solve_batch(native, mode, bt, "skip", Ts, R, keep, split, K, grid)
    np.testing.assert_array_equal(_b32(Ps), _b32(Pc))
    _assert_stats_equal(Ss, Sc, ALL_STATS)
    if not keep:
        Po, So = _solve_batch(native, mode, bt, "out", Ts, R, keep, split, K, grid)
        np.testing.assert_array_equal(_b32(Po), _b32(Pc))
        _assert_stats_equal(So, Sc, ("chi_in", "n_in", "ok", "rounds", "converged"))
        Pq, Sq = _solve_batch(native, mode, bt, "clean_out", Ts, R, keep, split, K, grid)
        np.testing.assert_array_equal(_b32(Pq), _b32(Pc))
        _assert_stats_equal(Sq, Sc, ("chi_in", "n_in", "ok", "rounds", "converged"))
    synth = _synth()
    for i, fr in enumerate(bt["frames"]):
        variants = [("skip", Ps, Ss)] + ([] if keep else [("out", Po, So)])
        for name, P, S in variants:
            T_ref, st_ref = O.solve_soa(Ts[i], Kn, E.ROWS, E.COLS, *E.soa(fr[name]), THR, keep_outliers=keep,
                                        mode=O.MODE_F64, max_rounds=R, conv_eps=-1.0)
            assert np.isfinite(P[i]).all()
            assert synth.se3_log_norm(P[i], T_ref) < _pose_tol(fr["n"]), (mode, name, i)
            assert S[i]["rounds"] == R and S[i]["ok"] == 1
            if R == 1:  # the statistics of round 1 are taken at the start pose: the gate is exact
                assert S[i]["n_in"] == st_ref["n_in"], (mode, name, i)
                np.testing.assert_allclose(S[i]["chi_in"], st_ref["chi_in"], rtol=1e-5)
                if name == "out":
                    assert np.isfinite(st_ref["chi_out"]) and np.isfinite(S[i]["chi_out"])
            else:
                # after 3 rounds the poses differ in the last bits: n_in equal or explained by the
                # ambiguous points, as test_gpu_parity holds every multi-round solve.  The slot
                # items are skipped or outliers at every pose (test_family_states) and are left out
                # of the float64 gate, which has no use for 3e38 and inf.
                ordinary = np.ones(fr["n"], bool)
                ordinary[fr["slots"]] = False
                _assert_n_in_explained(Kn, fr[name][ordinary, :3], fr[name][ordinary, 3:], P[i], T_ref,
                                       S[i]["n_in"], st_ref["n_in"])
                if name == "out":
                    assert np.isposinf(st_ref["chi_out"]) and np.isposinf(S[i]["chi_out"])


@pytest.mark.parametrize("split", ["1", "2", "4"])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("base", ["depth", "free"])
def test_block_mode_registers(native, oracle, base, keep, split):
    """Block mode, unsplit and split 2 and 4, 8 frames of about 1,750 items: accumulate_regs1 (one
    fast-reciprocal vote for the lane's whole register set, then accumulate_pinhole's zeroing vote
    per item); the last register slot is half empty, so its `__any` skip leaves whole waves out and
    the waves that stay hold the frame's last -- edge -- item and its padding copies.  The split
    layouts exchange the partial sums between partner blocks as hi + lo floats: the free base's out
    family sends an infinite chi_out through that exchange.  The split that took effect is asserted
    through the hand-off grid (8 x split blocks, none unsplit)."""
    _check_batch(native, oracle, "block", base, [1750, 1749, 1751, 1750, 1747, 1753, 1750, 1750], keep, split=split,
                 grid=0 if split == "1" else 8 * int(split))


@pytest.mark.parametrize("base", ["depth", "free"])
def test_block_mode_general_k(native, oracle, base):
    """Block mode with the skewed K: accumulate_regs1's general branch, accumulate_one (always
    zeroes all eight inputs of a skipped item, always the IEEE division)."""
    _check_batch(native, oracle, "block", base, [1750, 1749, 1751, 1750, 1747, 1753, 1750, 1750], 0, split="1",
                 K=E.K_SKEW, grid=0)


@pytest.mark.parametrize("split", ["4", "1"])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("base", ["depth", "free"])
def test_block_mode_lds_stream(native, oracle, base, keep, split):
    """Block mode with more items than the registers hold (6 x 20,000).  Split 4 (what the runtime
    picks for this shape; asserted through the hand-off grid of 32 blocks): 5,000 items per part,
    at most 4 in registers per lane (accumulate_regs1), the LDS-staged and streamed remainder
    through accumulate_stream1 / accumulate_item, whose loop is divergent and whose fast-reciprocal
    vote is taken per item by the lanes still in the loop.  Unsplit: 8 register items per lane
    (accumulate_regs) and the paired LDS and stream loops (accumulate2 with its per-pair
    RCP_CHECK vote)."""
    _check_batch(native, oracle, "block", base, [20000, 19999, 20001, 20000, 19997, 20003], keep, split=split,
                 grid=0 if split == "1" else 32)


@pytest.mark.parametrize("mode", ["persistent", "graph"])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("base", ["depth", "free"])
def test_one_frame_one_item_per_lane(native, oracle, base, keep, mode):
    """A batch of one frame of 100,003 items: one item per lane in persistent mode (accumulate:
    accumulate_pinhole with the division, its zeroing vote live), the pair form in graph mode."""
    _check_batch(native, oracle, mode, base, [100003], keep)


@pytest.mark.parametrize("mode", ["persistent", "graph"])
def test_one_frame_eight_items_per_lane(native, oracle, mode):
    """A batch of one frame of 1,000,003 items: eight register items per lane in persistent mode --
    the pair form accumulate_regs / accumulate_pinhole2, ONE vote for the four pairs, items 5 and
    5 + block size forming one (k, k + 1) pair of edge items -- and the float4 stream in graph mode.
    The depth base, one round (one oracle round per variant), keep_outliers = 0, which runs both the
    skip and the out family."""
    _check_batch(native, oracle, mode, "depth", [1000003], 0)


# ------------------------------------------------------------------------------------------------
# classify
# ------------------------------------------------------------------------------------------------
def _assert_classify_bits(got, ref, m):
    state, chi2, puv = ref
    np.testing.assert_array_equal(got["state"], state)
    # NaN payloads are compared with isnan, everything else bit for bit
    for g, r in ((got["chi2"], chi2),) + (((got["uv"], puv),) if "uv" in got else ()):
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r))
        ok = ~np.isnan(r)
        np.testing.assert_array_equal(_b32(g[ok]), _b32(r[ok]))
    assert len(got["state"]) == m


@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("base", ["depth", "free"])
def test_classify(native, base, kname):
    """picp_classify on every family (the NaN family included): state, chi2 and projection
    bit-identical to the float32 restatement of the oracle's gate, NaN compared with isnan; an edge
    item first and last."""
    K = KS[kname]
    s = native.PICPSolver(rows=E.ROWS, cols=E.COLS, K=K)
    s.setKernelThreshold(THR)
    for n in (1, 5, 257, 4099):
        p = E.make(base, n, shift=n % 5)
        for name in [k for (b, k) in E.FAMILIES if b == base]:
            for T in ([p["T0"]] if base == "depth" else [p["T0"], p["T1"]]):
                rows = p[name]
                s.init(T, rows[:, :3], rows[:, 3:])
                got = s.classify(_ident(n))
                ref = _np_classify(T, K, rows[:, :3], rows[:, 3:], THR)
                _assert_classify_bits(got, ref, n)
                want = E.EXPECTED_STATE[base, name]
                assert (got["state"][p["slots"]] == want).all()
                np.testing.assert_array_equal(got["inlier_idx"], np.nonzero(ref[0] == 1)[0])
                np.testing.assert_array_equal(got["counts"], np.bincount(ref[0], minlength=3))
    s.close()


@pytest.mark.parametrize("base", ["depth", "free"])
def test_batch_classify(native, base):
    """picp_batch_classify on the ragged sizes [0, 1, 5, 257, 4099], an edge item first and last in
    every frame (so the last item of one frame and the first of the next are both edge items)."""
    sizes = [0, 1, 5, 257, 4099]
    bt = E.make_batch(base, sizes)
    live = [fr for fr in bt["frames"] if fr is not None]
    Ts = np.stack([E.BASE_POSE[base]] + [fr["T0"] if base == "depth" else fr["T1"] for fr in live])
    for name in [k for (b, k) in E.FAMILIES if b == base]:
        rows = bt[name]
        b = native.Batch(sizes)
        b.set_data(rows[:, :3], rows[:, 3:])
        got = b.classify(THR, poses=Ts)
        b.close()
        off = 0
        for i, fr in enumerate(live):
            n = fr["n"]
            ref = _np_classify(Ts[i + 1], E.K_PIN, fr[name][:, :3], fr[name][:, 3:], THR)
            one = {"state": got["state"][off:off + n], "chi2": got["chi2"][off:off + n]}
            _assert_classify_bits(one, ref, n)
            np.testing.assert_array_equal(got["counts"][i + 1], np.bincount(ref[0], minlength=3))
            np.testing.assert_array_equal(got["inlier_idx"][got["inlier_off"][i + 1]:got["inlier_off"][i + 2]],
                                          np.nonzero(ref[0] == 1)[0])
            off += n


# ------------------------------------------------------------------------------------------------
# NaN passes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", sorted(KS))
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 4099])
def test_nan_passes(native, oracle, n, keep, kname):
    """NaN passes, as in the reference (src/camera.h:27-34 rejects with `<=`, `<` and `>`, which a
    NaN fails; src/picp_solver.cpp:77 gates with `>`): single solver, PICP_MODE=graph.  linearize:
    n_in and n_projected equal the oracle's, H, b and chi_in non-finite exactly where the oracle's
    are (everywhere); a 2-round solve: the pose's 3x4 block non-finite as the oracle's, ok and n_in
    equal.  With the pinhole K, H(0,1) consists only of terms the sparse Jacobian drops (the
    reference's NaN x 0 products); the pair form adds them in the waves that take the division
    (pinhole2_h01_dropped), which is what makes H(0,1) NaN here."""
    K = KS[kname]
    p = E.make("free", n)
    with _env(PICP_MODE="graph"):
        s = native.PICPSolver(rows=E.ROWS, cols=E.COLS, K=K)
        s.setKernelThreshold(THR)
        for T in (p["T0"], p["T1"]):
            got = _lin(s, p["nan"], T, keep)
            ref = _ref_lin(oracle, K, p["nan"], T, keep)
            assert (got["n_in"], got["n_projected"]) == (ref["n_in"], ref["n_projected"])
            for k in ("H", "b", "chi_in"):
                np.testing.assert_array_equal(np.isfinite(got[k]), np.isfinite(ref[k]), err_msg=k)
            assert not np.isfinite(got["H"]).any()
        s.close()
        Tg, st = _solve_single(native, K, p["nan"], p["T1"], 2, keep)
    Tr, sr = oracle.solve_soa(p["T1"], K, E.ROWS, E.COLS, *E.soa(p["nan"]), THR, keep_outliers=keep,
                              mode=oracle.MODE_F64, max_rounds=2, conv_eps=-1.0)
    np.testing.assert_array_equal(np.isfinite(Tg[:3, :]), np.isfinite(Tr[:3, :]))
    assert (st["ok"], st["n_in"]) == (sr["ok"], sr["n_in"])


# ------------------------------------------------------------------------------------------------
# the point refiner
# ------------------------------------------------------------------------------------------------
def _refine(native, case, **prm):
    r = native.PointRefiner(rows=case["rows"], cols=case["cols"], K=case["K"])
    r.set_poses(case["poses"])
    r.set_tracks(case["off"], case["obs_pose"], case["obs_uv"])
    r.set_points(case["start"])
    xyz, st = r.run(**prm)
    r.close()
    return xyz, st


@pytest.mark.parametrize("name,rounds", [("tied", 1), ("free", 10), ("nan", 10)])
def test_refiner_replacements(native, name, rounds):
    """refine_item (picp_refine.hip): "an unused observation, possibly with an infinite 1/z,
    contributes exact zeros".  Skipped observations of six well-observed points are replaced by
    observations at the pose-frame depth +0, -0 and 1e-40 ("tied", one round) or 3e38 ("free"), and
    other points start at +-3e38 ("free") or NaN ("nan").  The restatement's points, n_in, chi_in,
    ok and rounds do not change (test_refiner_replacements_are_invisible_to_the_restatement), so
    the GPU's points are bit-identical to its own clean run; a point at +-3e38 or NaN comes back
    unchanged with ok = 0, as the restatement with the kernel's float32 gate returns it; and the
    clean run is within 4 D of the float64 restatement (D measured here, as test_gpu_refine.py
    defines it)."""
    import refine_oracle as RO
    c = E.refine_case()
    prm = {**RO.BASE, "max_rounds": rounds}
    Xc, sc = _refine(native, c["clean"], **prm)
    Xe, se = _refine(native, c[name], **prm)
    keep = np.ones(len(Xc), bool)
    keep[c["moved"][name]] = False
    np.testing.assert_array_equal(_b32(Xe[keep]), _b32(Xc[keep]))
    for k in ("n_in", "ok", "rounds", "converged"):
        np.testing.assert_array_equal(se[k][keep], sc[k][keep], err_msg=k)
    np.testing.assert_array_equal(_b32(se["chi_in"][keep]), _b32(sc["chi_in"][keep]))
    _, s32, _ = RO.run_case(c[name], np.float32, **prm)
    for i in c["moved"][name]:
        assert se["ok"][i] == 0 and se["rounds"][i] == 0
        np.testing.assert_array_equal(_b32(Xe[i]), _b32(c[name]["start"][i]))
        assert (se["n_in"][i], se["n_projected"][i]) == (s32["n_in"][i], s32["n_projected"][i])
    # oracle parity of the clean run
    d, border, X64, st64 = RO.measure_d(c["clean"], **prm)
    ok = ~border
    worst = float(np.abs(Xc.astype(np.float64) - X64).max(1)[ok].max())
    print("refiner %s: D=%.3g max|gpu-oracle|=%.3g borderline=%d" % (name, d, worst, border.sum()))
    assert border.sum() <= 1 and worst <= 4 * d, (worst, d)
    for k in ("n_in", "n_projected", "rounds", "ok"):
        np.testing.assert_array_equal(sc[k][ok], st64[k][ok], err_msg=k)
