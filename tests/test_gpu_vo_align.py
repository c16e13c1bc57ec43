"""GPU tests of picp_vo_align_segments (csrc/picp_vo_align_runtime.cpp): consecutive segments of a
device-resident VO run aligned through their shared landmarks, against the same pairs built on the
host (picp_vo_get_map, picp_match_batch in its full form) and run through picp_sim3_batch, and
against the pose-based stitch bench.py does today.

The run: three segments of 6 steps, about 300 observations per frame, no pixel noise.  Segment 1's
second bootstrap pose carries a baseline scaled by 1.5, so its map is 1.5 times too large (about
its first camera, the overlap frame with segment 0): S[0] (segment 1 into 0) has scale 1 / 1.5 and
S[1] (segment 2 into 1) has scale 1.5.
"""
import functools

import numpy as np
import pytest

import sim3_ref as R

pytestmark = pytest.mark.gpu

THR = 3000.0
SCALE = 1.5
PRM = dict(threshold=0.01, hypotheses=256, min_inliers=4, with_scale=1, refits=2, seed=17)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case():
    from picp_amd.vo_synth import VOSequence, segments
    n_frames = 19
    s = VOSequence(n_frames, obs_per_frame=300, seed=11, pixel_noise=0.0)
    F = s.frames(0, n_frames)
    first, steps = segments(n_frames, 6)
    assert list(first) == [0, 6, 12] and list(steps) == [6, 6, 6]
    boot = np.stack([[F["T_cw"][f], F["T_cw"][f + 1]] for f in first]).astype(np.float64)
    boot[1, 1, :3, 3] = boot[1, 0, :3, 3] + SCALE * (boot[1, 1, :3, 3] - boot[1, 0, :3, 3])
    return {"K": s.K, "frame_off": F["frame_off"], "uv": F["uv"].astype(np.float32),
            "desc": F["desc"].astype(np.float32), "first": first, "steps": steps, "boot": boot.astype(np.float32)}


def _open(native, C):
    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    return seq


def _state(seq, n):
    return {"poses": seq.poses(), "rec": seq.step_records(), "map": [seq.map(k) for k in range(n)]}


def _same_state(a, b):
    for x, y in zip(a["poses"], b["poses"]):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    for x, y in zip(a["rec"], b["rec"]):
        for k in x:
            np.testing.assert_array_equal(x[k].view(np.uint32) if x[k].dtype == np.float32 else x[k],
                                          y[k].view(np.uint32) if y[k].dtype == np.float32 else y[k])
    for (x0, d0), (x1, d1) in zip(a["map"], b["map"]):
        np.testing.assert_array_equal(_bits(x0), _bits(x1))
        np.testing.assert_array_equal(_bits(d0), _bits(d1))


def _host_pairs(native, maps):
    """The pairs of every problem s built on the host: segment s + 1's map matched against segment s's."""
    m = native.match_points_batch([maps[s + 1][1] for s in range(len(maps) - 1)],
                                  [maps[s][1] for s in range(len(maps) - 1)], form="full")
    out = []
    for s, ms in enumerate(m):
        j = np.flatnonzero(ms["accepted"])
        out.append((np.ascontiguousarray(maps[s + 1][0][j]), np.ascontiguousarray(maps[s][0][ms["best_idx"][j]])))
    return out


def _scaled(c):
    return np.diag([c, c, c, 1.0])


@pytest.fixture(scope="module")
def run(native):
    C = _case()
    seq = _open(native, C)
    seq.run()
    before = _state(seq, 3)
    got = seq.align_segments(**PRM)
    again = seq.align_segments(**PRM)
    after = _state(seq, 3)
    seq.run()  # a later call keeps its bits
    rerun = _state(seq, 3)
    seq.close()
    return {"before": before, "got": got, "again": again, "after": after, "rerun": rerun}


def test_align_is_read_only_and_repeats(run):
    _same_state(run["before"], run["after"])
    _same_state(run["before"], run["rerun"])
    for a, b in zip(run["got"], run["again"]):
        assert (a["inliers"], a["found"], a["n_pairs"]) == (b["inliers"], b["found"], b["n_pairs"])
        np.testing.assert_array_equal(_bits(a["S"]), _bits(b["S"]))
        assert np.float32(a["scale"]).view(np.uint32) == np.float32(b["scale"]).view(np.uint32)


def test_align_has_the_bits_of_the_batch_call_on_host_built_pairs(native, run):
    pairs = _host_pairs(native, run["before"]["map"])
    want = native.sim3_ransac_batch([p[0] for p in pairs], [p[1] for p in pairs], threshold=PRM["threshold"],
                                    hypotheses=PRM["hypotheses"], min_inliers=PRM["min_inliers"], with_scale=True,
                                    refits=PRM["refits"], seed=PRM["seed"])
    assert len(run["got"]) == 2
    for g, w, (src, dst) in zip(run["got"], want, pairs):
        assert g["n_pairs"] == len(src) and len(src) >= 50
        assert g["found"] and w["found"] and g["inliers"] == w["inliers"]
        np.testing.assert_array_equal(_bits(g["S"]), _bits(w["S"]))
        assert np.float32(g["scale"]).view(np.uint32) == np.float32(w["scale"]).view(np.uint32)


def test_align_recovers_the_scale_and_agrees_with_the_pose_based_stitch(native, run):
    """Both are estimates of one transform from different data: S[s] from the shared landmarks, the
    stitch from the overlap frame's pose in either segment (with the constructed scale, which the
    stitch cannot see).  The bound on the device's distance from the stitch is 4 times the
    distance the numpy reference pipeline (tests/sim3_ref.py, fed the same downloaded maps and
    matches) shows from it, on the probe discrepancy over the problem's own pairs; the scale is
    held to 4 times the reference's own relative distance from the constructed one, plus float32's
    1e-6.  Measured: DESIGN.md §4.13."""
    from picp_amd.evaluate import chain_similarities
    pairs = _host_pairs(native, run["before"]["map"])
    P = [np.asarray(p, np.float64) for p in run["before"]["poses"]]
    expect = [1.0 / SCALE, SCALE]
    for s, (g, (src, dst)) in enumerate(zip(run["got"], pairs)):
        # x_s = P_s[last] (c (P_{s+1}[0])^-1 x_{s+1}): the overlap camera sees the same points, c times as far
        stitch = P[s][-1] @ _scaled(expect[s]) @ np.linalg.inv(P[s + 1][0])
        ref = R.ransac(src, dst, PRM["threshold"], PRM["hypotheses"], PRM["min_inliers"], True, PRM["refits"],
                       PRM["seed"], s)
        assert ref["found"] and g["found"]
        d_ref, d_dev = R.discrepancy(ref["S"], stitch, src, dst), R.discrepancy(g["S"], stitch, src, dst)
        e_ref, e_dev = abs(ref["scale"] / expect[s] - 1), abs(g["scale"] / expect[s] - 1)
        print("s=%d: %d pairs, %d inliers; from the stitch: reference %.2e, device %.2e of the extent; scale %.6f "
              "(constructed %.6f): reference off by %.2e, device by %.2e"
              % (s, len(src), g["inliers"], d_ref, d_dev, g["scale"], expect[s], e_ref, e_dev))
        assert d_dev <= 4.0 * d_ref
        assert e_dev <= 4.0 * e_ref + 1e-6
        assert g["inliers"] >= len(src) // 2
    chain = chain_similarities([g["S"] for g in run["got"]])
    assert len(chain) == 3 and (chain[0] == np.eye(4)).all()
    np.testing.assert_allclose(chain[2], np.asarray(run["got"][0]["S"], np.float64) @ np.asarray(run["got"][1]["S"], np.float64))
    assert abs(R.scale_of(chain[2]) - 1.0) < 1e-2  # segment 2 is at segment 0's scale again


def test_segments_that_share_no_landmark_are_not_aligned(native):
    """Two segments 200 frames apart (the frames between them are left empty)."""
    from picp_amd.vo_synth import VOSequence
    s = VOSequence(207, obs_per_frame=300, seed=11, pixel_noise=0.0)
    A, B = s.frames(0, 7), s.frames(200, 207)
    counts = np.zeros(207, np.int64)
    counts[:7], counts[200:] = np.diff(A["frame_off"]), np.diff(B["frame_off"])
    off = np.zeros(208, np.int64)
    off[1:] = np.cumsum(counts)
    uv = np.concatenate([A["uv"], B["uv"]]).astype(np.float32)
    desc = np.concatenate([A["desc"], B["desc"]]).astype(np.float32)
    boot = np.stack([[A["T_cw"][0], A["T_cw"][1]], [B["T_cw"][0], B["T_cw"][1]]])
    seq = native.VOSequence(off, uv, desc, K=s.K)
    seq.set_segments([0, 200], [6, 6], boot, threshold=THR)
    seq.run()
    assert all(len(seq.map(k)[0]) > 100 for k in range(2))
    got = seq.align_segments(**PRM)
    seq.close()
    assert len(got) == 1 and not got[0]["found"] and got[0]["n_pairs"] < 4 and got[0]["inliers"] == 0
    assert (got[0]["S"] == np.eye(4, dtype=np.float32)).all() and got[0]["scale"] == 1.0


def test_one_segment_has_nothing_to_align(native):
    C = _case()
    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    with pytest.raises(native.PicpError):
        seq.align_segments()  # no segments set: picp_vo_get_map's condition
    seq.set_segments(C["first"][:1], C["steps"][:1], C["boot"][:1], threshold=THR)
    seq.run()
    assert seq.align_segments() == []
    seq.close()
