"""GPU tests of picp_pgo_batch (csrc/picp_pgo.hip): ragged batches against tests/pgo_ref.py within
tol = 1e-6 + 4 floor of the probe discrepancy and the cost bound, the same bits on a second call
and alone, failures beside graphs that run, and the pr:: facade.  The reference of a case is
computed once per process (pgo_ref.reference).
"""
import os
import subprocess

import numpy as np
import pytest

import pgo_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu

EMPTY = {"S": np.zeros((0, 4, 4), np.float32), "fixed": np.zeros(0, np.uint8), "edges": np.zeros((0, 2), np.int32),
         "Z": np.zeros((0, 4, 4), np.float32), "weight": np.zeros(0, np.float32)}
# sizes 2, 12, 1 node with 0 edges, 65, 0 nodes, 300, 12 permuted
RAGGED = ["two", "a", None, "ring65", None, "ring300", "a_permuted"]


def _graph(name, k=0):
    if name is None:  # one free node without an edge, or nothing at all
        return dict(EMPTY, S=R.variants()["a"][0]["S"][3:4], fixed=np.zeros(1, np.uint8)) if k == 2 else EMPTY
    return R.variants()[name][0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    np.testing.assert_array_equal(_bits(a["S"]), _bits(b["S"]))
    fig = lambda o: np.array([o[k] for k in ("cost_initial", "cost_final", "grad_initial", "grad_final")]).view(np.uint64)
    np.testing.assert_array_equal(fig(a), fig(b))
    assert (a["steps"], a["status"]) == (b["steps"], b["status"])


@pytest.fixture(scope="module")
def ragged(native):
    graphs = [_graph(n, k) for k, n in enumerate(RAGGED)]
    return {"graphs": graphs, "got": native.pose_graph_batch(graphs), "again": native.pose_graph_batch(graphs),
            "solo": [native.pose_graph_batch([g])[0] for g in graphs]}


def test_ragged_batch_meets_the_reference(ragged):
    for name, g, o in zip(RAGGED, ragged["graphs"], ragged["got"]):
        assert o["status"] == R.OK
        if name is None:
            assert o["steps"] == 0 and o["cost_final"] == 0.0
            np.testing.assert_array_equal(_bits(o["S"]), _bits(g["S"]))
            continue
        assert o["steps"] == 10
        R.check_against(name, o["S"], o["cost_final"], "device ")
        ref = R.reference(name)
        assert abs(o["cost_initial"] - ref["cost_initial"]) <= 1e-9 * ref["cost_initial"] + 1e-14 * ref["cost_initial"] ** 0.5
        assert o["grad_final"] <= 1e-6 * o["grad_initial"]
        fixed = np.flatnonzero(g["fixed"])
        np.testing.assert_array_equal(_bits(o["S"][fixed]), _bits(g["S"][fixed]))
    two, o = ragged["graphs"][0], ragged["got"][0]  # one edge: S_1 = S_0 Z
    want = np.stack([two["S"][0].astype(np.float64), two["S"][0].astype(np.float64) @ two["Z"][0].astype(np.float64)])
    assert R.discrepancy(o["S"], want) <= R.tol(R.reference("two")["S"])


def test_second_call_and_each_graph_alone_give_the_same_bits(ragged):
    for a, b, c in zip(ragged["got"], ragged["again"], ragged["solo"]):
        _same(a, b)
        _same(a, c)


def test_the_other_cases_meet_the_reference(native):
    names = ["b", "c", "d", "triangle", "a_fixed5", "a_duplicate", "a_zero_weight"]
    got = native.pose_graph_batch([_graph(n) for n in names])
    for name, o in zip(names, got):
        assert (o["status"], o["steps"]) == (R.OK, 10)
        R.check_against(name, o["S"], o["cost_final"], "device ")
    assert got[2]["cost_final"] < 1e-12  # d: consistent measurements
    rigid = native.pose_graph_batch([_graph("a_rigid")], with_scale=False)[0]
    assert (rigid["status"], rigid["steps"]) == (R.OK, 10)
    R.check_against("a_rigid", rigid["S"], rigid["cost_final"], "device ")
    assert np.abs(np.cbrt(np.linalg.det(rigid["S"][:, :3, :3].astype(np.float64))) - 1).max() < 1e-6


def test_eps_ends_the_steps_early(native):
    a = _graph("a")
    full, early = native.pose_graph_batch([a])[0], native.pose_graph_batch([a], eps=1e-3)[0]
    assert 1 <= early["steps"] < 10 and early["status"] == R.OK
    assert early["cost_final"] <= full["cost_final"] * (1 + 1e-2)
    none = native.pose_graph_batch([a], iterations=0)[0]
    assert none["steps"] == 0 and none["cost_final"] == none["cost_initial"] == full["cost_initial"]
    np.testing.assert_array_equal(_bits(none["S"][0]), _bits(a["S"][0]))


def test_failures_in_a_batch_leave_the_others_alone(native):
    """Graphs 1, 3 and 4 of 6 fail the plan's checks (a NaN entry, a free node that nothing joins, an
    edge with i = j): they never reach the device."""
    a = _graph("a")
    copy = lambda: {k: np.array(v) for k, v in a.items()}
    nan = copy()
    nan["Z"][3, 1, 1] = np.nan
    loose = copy()
    loose["S"] = np.concatenate([a["S"], a["S"][:1]])
    loose["fixed"] = np.concatenate([a["fixed"], [0]]).astype(np.uint8)
    selfe = copy()
    selfe["edges"][6, 1] = selfe["edges"][6, 0]
    graphs = [a, nan, _graph("b"), loose, selfe, _graph("two")]
    got = native.pose_graph_batch(graphs)
    assert [o["status"] for o in got] == [R.OK, R.BAD_INPUT, R.OK, R.DISCONNECTED, R.BAD_EDGE, R.OK]
    for k in (1, 3, 4):
        np.testing.assert_array_equal(_bits(got[k]["S"]), _bits(graphs[k]["S"]))
        assert got[k]["steps"] == 0
    for k in (0, 2, 5):
        _same(got[k], native.pose_graph_batch([graphs[k]])[0])
        assert got[k]["steps"] == 10


def test_facade_reproduces_the_python_call(native, tmp_path):
    a = _graph("a")
    want = native.pose_graph_batch([a])[0]
    path = str(tmp_path / "batch.txt")
    R.write_batch(path, [a])
    out = subprocess.run([os.path.join(PKG, "bin", "pgo_main"), path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    tok = out.stdout.split()
    assert tok[:4] == ["pgo", "1", "0", "10"]
    fig = np.array([int(t, 16) for t in tok[4:8]], np.uint64).view(np.float64)
    assert list(fig) == [want["cost_initial"], want["cost_final"], want["grad_initial"], want["grad_final"]]
    S = np.array([int(t, 16) for t in tok[8:]], np.uint32).reshape(-1, 4, 4)
    np.testing.assert_array_equal(np.transpose(S, (0, 2, 1)), _bits(want["S"]).reshape(-1, 4, 4))
