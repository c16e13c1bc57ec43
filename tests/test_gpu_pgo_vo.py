"""The pose-graph solver's first user: the segments of a device-resident VO run as a graph, with
one measurement more than the chain needs.  The run has the shape of tests/test_gpu_vo_align.py
(19 frames, three segments of 6 steps, about 300 observations per frame, seed 11; segment 1's
bootstrap baseline scaled by 1.5) with pixel noise 0.5.  Edges (0, 1) and (1, 2) come from
align_segments; edge (0, 2) from sim3_ransac_batch on pairs of segment 2's map matched against
segment 0's (segment 0's frames see the landmarks spawned at steps -3..36, segment 2's those at
9..48, so the two maps share landmarks).  The weights are the inlier counts.

Should the (0, 2) problem have fewer than 50 pairs or not be found, the segments are shortened to
4 steps (13 frames); the shape that was used is printed.  The edge is never dropped.  Measured
(DESIGN.md §4.14): the 6-step shape is used, its (0, 2) problem has 126 pairs and 14 inliers.
"""
import functools

import numpy as np
import pytest

import pgo_ref as R

pytestmark = pytest.mark.gpu

THR = 3000.0
SCALE = 1.5
PRM = dict(threshold=0.01, hypotheses=256, min_inliers=4, with_scale=1, refits=2, seed=17)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(seg_len):
    from picp_amd.vo_synth import VOSequence, segments
    n_frames = 3 * seg_len + 1
    s = VOSequence(n_frames, obs_per_frame=300, seed=11, pixel_noise=0.5)
    F = s.frames(0, n_frames)
    first, steps = segments(n_frames, seg_len)
    assert len(first) == 3 and list(steps) == [seg_len] * 3
    boot = np.stack([[F["T_cw"][f], F["T_cw"][f + 1]] for f in first]).astype(np.float64)
    boot[1, 1, :3, 3] = boot[1, 0, :3, 3] + SCALE * (boot[1, 1, :3, 3] - boot[1, 0, :3, 3])
    return {"K": s.K, "frame_off": F["frame_off"], "uv": F["uv"].astype(np.float32),
            "desc": F["desc"].astype(np.float32), "first": first, "steps": steps, "boot": boot.astype(np.float32)}


def _state(seq):
    return {"poses": seq.poses(), "map": [seq.map(k) for k in range(3)]}


def _edges(native, seg_len):
    """The run, its three measured similarities and their inlier counts; None when the (0, 2) problem
    has fewer than 50 pairs or is not found."""
    C = _case(seg_len)
    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    seq.run()
    chain = seq.align_segments(**PRM)
    maps = [seq.map(k) for k in range(3)]
    m = native.match_points_batch([maps[2][1]], [maps[0][1]], form="full")[0]
    j = np.flatnonzero(m["accepted"])
    src, dst = np.ascontiguousarray(maps[2][0][j]), np.ascontiguousarray(maps[0][0][m["best_idx"][j]])
    far = native.sim3_ransac_batch([src], [dst], threshold=PRM["threshold"], hypotheses=PRM["hypotheses"],
                                   min_inliers=PRM["min_inliers"], with_scale=True, refits=PRM["refits"],
                                   seed=PRM["seed"])[0] if len(j) >= 4 else {"found": False, "inliers": 0}
    print("segments of %d steps: (0, 2) has %d pairs, found %s, %d inliers; chain inliers %s"
          % (seg_len, len(j), far["found"], far["inliers"], [c["inliers"] for c in chain]))
    if len(j) < 50 or not far["found"]:
        seq.close()
        return None
    assert all(c["found"] for c in chain)
    return {"seq": seq, "chain": chain, "far": far, "seg_len": seg_len}


@pytest.fixture(scope="module")
def run(native):
    from picp_amd.evaluate import segment_graph
    E = _edges(native, 6) or _edges(native, 4)
    assert E is not None, "the (0, 2) edge must exist at one of the two shapes"
    seq = E["seq"]
    g = segment_graph([c["S"] for c in E["chain"]], extra=[(0, 2, E["far"]["S"])])
    g["weight"] = np.array([c["inliers"] for c in E["chain"]] + [E["far"]["inliers"]], np.float32)
    before = _state(seq)
    got = native.pose_graph_batch([g])[0]
    after = _state(seq)
    seq.close()
    return {"graph": g, "got": got, "before": before, "after": after, "seg_len": E["seg_len"]}


def test_segment_graph_is_the_chain_plus_the_extra_edge(run):
    from picp_amd.evaluate import chain_similarities
    g = run["graph"]
    assert g["edges"].tolist() == [[0, 1], [1, 2], [0, 2]] and g["fixed"].tolist() == [1, 0, 0]
    chain = chain_similarities([g["Z"][0], g["Z"][1]])
    np.testing.assert_array_equal(g["S"], np.stack(chain).astype(np.float32))
    assert g["S"].dtype == np.float32 and g["Z"].shape == (3, 4, 4)


def test_device_result_meets_the_reference_on_the_same_edges(run):
    g, o = run["graph"], run["got"]
    assert (o["status"], o["steps"]) == (R.OK, 10)
    ref = R.solve(g["S"], g["fixed"], g["edges"], g["Z"], g["weight"])
    d, t = R.discrepancy(o["S"], ref["S"]), R.tol(ref["S"])
    print("segments of %d steps: discrepancy %.3e, floor %.3e, tol %.3e; cost %.6g -> %.6g (reference %.6g)"
          % (run["seg_len"], d, R.floor(ref["S"]), t, o["cost_initial"], o["cost_final"], ref["cost_final"]))
    assert d <= t
    assert o["cost_final"] <= ref["cost_final"] * (1 + 1e-6)


def test_the_cycle_closes_better_than_the_chain(run):
    g, o = run["graph"], run["got"]
    Zi = np.linalg.inv(R.canonical(g["Z"][2]))

    def cycle(S):
        S = [R.canonical(s) for s in S]
        return float(np.linalg.norm(R.log(Zi @ np.linalg.inv(S[0]) @ S[2])))

    r0, r1 = cycle(g["S"]), cycle(o["S"])
    print("cycle residual: %.4e at the chain, %.4e after the solve" % (r0, r1))
    assert r1 < r0
    np.testing.assert_array_equal(_bits(o["S"][0]), _bits(g["S"][0]))  # the fixed node


def test_the_run_keeps_its_bits_across_the_call(run):
    for x, y in zip(run["before"]["poses"], run["after"]["poses"]):
        np.testing.assert_array_equal(_bits(x), _bits(y))
    for (x0, d0), (x1, d1) in zip(run["before"]["map"], run["after"]["map"]):
        np.testing.assert_array_equal(_bits(x0), _bits(x1))
        np.testing.assert_array_equal(_bits(d0), _bits(d1))
