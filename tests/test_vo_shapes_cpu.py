"""What the frame-size schedules of tests/vo_shapes.py hold, proven on the CPU oracle alone
(oracle.vo_segment, oracle.match_points): the GPU tests of tests/test_gpu_vo_shapes.py run paths
only if these sizes and cases are really there.

Supplied by (schedule, step t = the step that queries frame t + 1; the tests print the full list):
  empty query frame                              fused8 t3, t6, tails t5
  n_corr == 0 on a non-empty query frame         fused8 t7 (two observations of unmapped landmarks),
                                                 tails t9 (one)
  n_corr == 1                                    fused8 t4: one observation of a mapped landmark,
                                                 80 px or more from where the step's start pose
                                                 puts it, so outside the inlier gate (n_in 0; a
                                                 single INLIER can be fitted exactly and its round
                                                 count is rounding: vo_shapes.NOISE)
  n_new == 0 with accepted curr->next pairs      step 0 of every schedule (every pair's next point
                                                 has a map match), streamed t0
  n_new == 0, empty current frame                fused8 t4, t7, tails t6
  n_new >= 1 from a current frame of <= 2        fused8 t8 (2 points from 2 observations)
  fused8 n_corr around slice and slot edges      n_corr 3606, 3263, 2775, 2760, 2023, 1, 0: the last
                                                 item in an even and in an odd 256-item pass, in
                                                 register slots 0, 3, 5, 6 and 7 (the last)
  tails: world match and selected pair >= 4096   t1, t4, t8 (both), t2, t12 (pairs), t3, t7, t11
  tail1: the pair at observation 4096 selected   t2
  streamed: more items than registers + stage    t0: n_corr 12000 > 11776; t1 fills the stage partly
"""
import numpy as np
import pytest

import vo_shapes as VS


@pytest.mark.parametrize("name", VS.NAMES)
def test_sizes_and_max_obs(name):
    S = VS.build(name)
    n = np.diff(S["frame_off"])
    assert n.tolist() == VS.sizes(name)
    assert int(n.max()) == S["max_obs"]
    # the driver's path rule restated (picp_vo_set_segments, picp_vo_block_fusable)
    npt = 1
    while npt < 8 and npt * 2 * 512 <= S["max_obs"]:
        npt *= 2
    assert npt == S["npt"]
    assert S["fused"] == (S["max_obs"] <= 4096)
    print("VO_SHAPE %s: max_obs %d npt %d %s" % (name, S["max_obs"], npt, "fused" if S["fused"] else "unfused"))


def test_listed_sizes_occur():
    """The sizes the path table depends on, in the schedule that is there for them."""
    have = {name: set(VS.sizes(name)) for name in VS.NAMES}
    for m in (1023, 1024, 2047, 2048, 4095):
        assert {m, m - 1, 512} <= have["npt_%d" % m]
    assert {4096, 4095, 3585, 1, 0, 2} <= have["fused8"]
    assert {4097, 64, 4096} <= have["tail1"]
    # gather tail chunks end at 4096 + 256 k, append tail chunks at 4096 + 512 k
    assert {4096, 4097, 4608, 4095, 0, 513, 1, 512, 4700, 257, 64, 5000, 4352, 4353, 4609} <= have["tails"]
    assert {12000, 11777, 300} <= have["streamed"]
    # the append's tail runs over the CURRENT frame, the gather's over the QUERY frame: both see
    # every size above 4096 (a frame is the query of one step and the current one of the next)
    for name in ("tail1", "tails", "streamed"):
        z = VS.sizes(name)
        big = [k for k, v in enumerate(z) if v > 4096]
        assert any(0 < k < len(z) - 1 for k in big), name


def _all_steps(names):
    for name in names:
        for rows in VS.oracle_steps(name):
            for r in rows:
                yield name, r


def _find(names, pred, what, need=True):
    hits = [(name, r) for name, r in _all_steps(names) if pred(r)]
    print("VO_CASE %-48s %s" % (what, ", ".join("%s seg %d t%d" % (n, r["seg"], r["t"]) for n, r in hits) or "-"))
    if need:
        assert hits, what
    return hits


def test_cases_present():
    single = [n for n in VS.NAMES if n != "tails_seg"]
    _find(single, lambda r: r["nq"] == 0, "empty query frame")
    _find(single, lambda r: r["nq"] > 0 and r["n_corr"] == 0, "n_corr == 0, non-empty query frame")
    _find(single, lambda r: r["n_corr"] == 1, "n_corr == 1")
    _find(single, lambda r: r["n_corr"] >= 1 and r["n_in"] == 0, "correspondences, none an inlier")
    _find(single, lambda r: r["n_new"] == 0 and r["pairs_accepted"] >= 1, "n_new == 0, accepted pairs")
    _find(single, lambda r: r["n_new"] == 0 and r["nc"] == 0, "n_new == 0, empty current frame")
    _find(single, lambda r: r["n_new"] >= 1 and r["nc"] <= 2, "n_new >= 1 from <= 2 observations")
    _find(["tails"], lambda r: r["corr_idx_max"] >= 4096, "tails: world match at observation >= 4096")
    _find(["tails"], lambda r: r["new_idx_max"] >= 4096, "tails: selected pair at observation >= 4096")
    _find(["tails_seg"], lambda r: r["corr_idx_max"] >= 4096, "tails_seg: world match at observation >= 4096")
    _find(["tails_seg"], lambda r: r["new_idx_max"] >= 4096 or r["nq"] == 0, "tails_seg: tail pair or empty frame")
    _find(["tail1"], lambda r: r["new_idx_max"] == 4096, "tail1: the one-observation append tail selects")
    _find(["streamed"], lambda r: r["n_corr"] > 4096 + 7680, "streamed: items past registers + LDS stage")
    _find(["streamed"], lambda r: 4096 < r["n_corr"] <= 4096 + 7680, "streamed: LDS stage partly filled")
    # npt_edges: a frame of 512 and the two largest frames are queried in every sequence
    for m in (1023, 1024, 2047, 2048, 4095):
        nq = {r["nq"] for _, r in _all_steps(["npt_%d" % m])}
        assert {m, m - 1, 512} <= nq


def test_fused8_counts_around_slice_and_slot_edges():
    """vo_gather_items moves the items to registers in passes of 256 (two per 512-item register
    slot).  The last item n_corr - 1 decides the last pass and which lanes take the clamp: it must
    fall in an even and in an odd pass (either side of a multiple of 256 that is no multiple of
    512), in more than one register slot (either side of a multiple of 512) and in the last slot."""
    nc = sorted({r["n_corr"] for _, r in _all_steps(["fused8"]) if r["n_corr"] > 0})
    print("VO_CASE fused8 n_corr values", nc)
    passes = {(n - 1) // 256 for n in nc}
    slots = {(n - 1) // 512 for n in nc}
    assert {p & 1 for p in passes} == {0, 1}
    assert len(slots) >= 3 and 7 in slots and 0 in slots
    assert any(r["n_corr"] == 0 for _, r in _all_steps(["fused8"]))


@pytest.mark.parametrize("name", VS.NAMES)
def test_no_zero_baseline_append_and_finite(name):
    for k, ref in enumerate(VS.reference(name)):
        assert np.isfinite(ref["poses"]).all() and np.isfinite(ref["map_xyz"]).all()
        assert ref["n_new"][0] > 0
    worst = np.inf
    for _, r in _all_steps([name]):
        if r["n_new"] > 0:
            worst = min(worst, r["baseline"])
            assert r["baseline"] >= 0.05, (name, r["seg"], r["t"], r["baseline"])
    print("VO_SHAPE %s: smallest baseline of an appending step %.3f m" % (name, worst))


@pytest.mark.parametrize("name", VS.NAMES)
def test_round_counts_are_a_property_of_the_data(oracle, name):
    """Every step stops after the same number of rounds, with the same inliers, whether the oracle
    accumulates in float32 (the reference's arithmetic) or in float64: the convergence test is
    decided by the data, not by rounding (vo_shapes.NOISE), so the GPU can be held to the
    teacher-forced oracle's round count."""
    for k, (a, b) in enumerate(zip(VS.reference(name), VS.reference(name, oracle.MODE_FAITHFUL))):
        print("VO_SHAPE %s segment %d: rounds %s n_in %s" % (name, k, a["rounds"].tolist(), a["n_in"].tolist()))
        np.testing.assert_array_equal(a["rounds"], b["rounds"])
        np.testing.assert_array_equal(a["n_in"], b["n_in"])
        np.testing.assert_array_equal(a["n_corr"], b["n_corr"])
        np.testing.assert_array_equal(a["n_new"], b["n_new"])
    # ... and no step stops at the rounding floor of chi_in, (an ulp of a pixel coordinate)^2 = 9.3e-10
    # per term: either nothing is an inlier (no update, two rounds) or the noise holds chi_in up
    for rows in VS.oracle_steps(name):
        for r in rows:
            assert r["n_in"] == 0 or r["chi_in"] >= 1e-4 * r["n_in"], (name, r["seg"], r["t"], r["n_in"], r["chi_in"])
            if r["n_in"] == 0:
                assert r["rounds"] == 2


def test_oracle_pose_of_a_step_without_correspondences(oracle):
    """What the reference's loop does with no correspondence: H = 0, b = 0, dx = 0, and the pose
    goes through previous.inverse() into the solver and through .inverse() out again.  The
    rotation keeps its bits; the translation is -(R (-(R^T t))) in float32, which need not be t.
    So the pin for the GPU is the double inverse, bit for bit -- not the previous pose."""
    n = 0
    for name, r in _all_steps(VS.NAMES):
        if r["n_in"] != 0:  # no correspondence, or none inside the inlier gate
            continue
        ref = VS.reference(name)[r["seg"]]
        a, b = ref["poses"][r["t"]], ref["poses"][r["t"] + 1]
        twice = oracle.iso_inverse(oracle.iso_inverse(a))
        np.testing.assert_array_equal(b.view(np.uint32), twice.view(np.uint32))
        np.testing.assert_array_equal(b[:3, :3].view(np.uint32), a[:3, :3].view(np.uint32))
        dt = np.abs(b[:3, 3].astype(np.float64) - a[:3, 3])
        assert dt.max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(a[:3, 3]).max())
        assert ref["n_in"][r["t"]] == 0
        print("VO_CASE %s seg %d t%d: n_corr %d, n_in 0, rounds %d, |dt| %.3g" % (
            name, r["seg"], r["t"], r["n_corr"], ref["rounds"][r["t"]], dt.max()))
        n += 1
    assert n >= 3
