"""CPU tests of the pose-graph solver (picp_pgo_batch): the reference's own checks, the argument
errors and every per-graph failure through the library (a batch in which no graph runs needs no
device), the plan (csrc/picp_pgo_plan.cpp) against a restatement, and the whole host solve of
bin/pgo_check -- csrc/picp_pgo_solve.h and csrc/picp_sim3_lie.h, the headers the kernel is made of,
with one worker, under ASan/UBSan -- against tests/pgo_ref.py on every case, within
tol = 1e-6 + 4 floor of the probe discrepancy and the cost bound.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import pgo_ref as R
from conftest import PKG

CHECK = os.path.join(PKG, "bin", "pgo_check")
MAX_BLOCKS = 1 << 18


def _run(mode, graphs, tmp_path, **kw):
    path = str(tmp_path / "batch.txt")
    R.write_batch(path, graphs, **kw)
    out = subprocess.run([CHECK, mode, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout)


def _S_of(out, lo, hi):
    bits = np.array(out["S_bits"], np.uint32)[16 * lo:16 * hi]
    return np.transpose(bits.view(np.float32).reshape(-1, 4, 4), (0, 2, 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_reference_checks_itself():
    fig = R.self_check()
    print(fig)


# ---------------------------------------------------------------------------------------------
# the host solve against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "d", "two", "triangle", "ring65", "ring300", "a_permuted",
                                  "a_fixed5", "a_duplicate", "a_zero_weight", "a_rigid"])
def test_host_solve_meets_the_reference(name, tmp_path):
    g, with_scale = R.variants()[name]
    out = _run("solve", [g], tmp_path, with_scale=with_scale)
    assert out["status"] == [R.OK] and out["steps"] == [10]
    R.check_against(name, _S_of(out, 0, len(g["S"])), out["cost_final"][0], "host ")
    ref = R.reference(name)
    # a residual is a logarithm next to the identity: its entries carry absolute rounding errors of about
    # 1e-16, so the cost (|r| ~ sqrt(cost)) carries about 1e-16 m sqrt(cost) beside its relative error
    assert abs(out["cost_initial"][0] - ref["cost_initial"]) <= 1e-9 * ref["cost_initial"] + 1e-14 * ref["cost_initial"] ** 0.5
    assert abs(out["grad_initial"][0] - ref["grad_initial"]) <= 1e-6 * ref["grad_initial"]
    assert out["grad_final"][0] <= 1e-6 * out["grad_initial"][0]
    fixed = np.flatnonzero(g["fixed"])
    np.testing.assert_array_equal(_bits(_S_of(out, 0, len(g["S"]))[fixed]), _bits(g["S"][fixed]))
    if name == "d":
        assert out["cost_final"][0] < 1e-12
    if name == "two":  # one edge: S_1 = S_0 Z
        want = g["S"][0].astype(np.float64) @ g["Z"][0].astype(np.float64)
        assert R.discrepancy(_S_of(out, 0, 2), np.stack([g["S"][0].astype(np.float64), want])) <= R.tol(ref["S"])


def test_host_solve_stops_on_eps_and_takes_damping(tmp_path):
    g, _ = R.variants()["a"]
    full = _run("solve", [g], tmp_path)
    early = _run("solve", [g], tmp_path, eps=1e-3)
    assert 1 <= early["steps"][0] < 10 and early["status"] == [R.OK]
    assert early["cost_final"][0] <= full["cost_final"][0] * (1 + 1e-2)
    damped = _run("solve", [g], tmp_path, iterations=1, damping=1e3)
    plain = _run("solve", [g], tmp_path, iterations=1)
    move = lambda o: np.abs(_S_of(o, 0, 12).astype(np.float64) - g["S"]).max()
    assert damped["steps"] == [1] and 0 < move(damped) < 0.1 * move(plain)
    none = _run("solve", [g], tmp_path, iterations=0)
    assert none["steps"] == [0] and none["cost_final"] == none["cost_initial"]


# ---------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------
def _restated_plan(n, fixed, edges, weight=None):
    """first[], the row offsets and the gather lists, straight from their definitions."""
    fidx, nf = [], 0
    for k in range(n):
        fidx.append(-1 if fixed[k] else nf)
        nf += 0 if fixed[k] else 1
    live = [e for e in range(len(edges)) if weight is None or weight[e] > 0]
    first = list(range(nf))
    for e in live:
        a, b = fidx[edges[e][0]], fidx[edges[e][1]]
        if a >= 0 and b >= 0:
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    row_off = [0]
    for a in range(nf):
        row_off.append(row_off[-1] + a - first[a] + 1)
    tasks = {}
    for e in live:
        a, b = fidx[edges[e][0]], fidx[edges[e][1]]
        if a >= 0:
            tasks.setdefault((0, a, a), []).append(4 * e + 0)
        if b >= 0:
            tasks.setdefault((0, b, b), []).append(4 * e + 3)
        if a >= 0 and b >= 0:
            tasks.setdefault((1, max(a, b), min(a, b)), []).append(4 * e + (1 if a > b else 2))
    for a in range(nf):
        tasks.setdefault((0, a, a), [])
    keys = sorted(tasks)
    slot = [row_off[a] + b - first[a] for _, a, b in keys]
    off = np.concatenate([[0], np.cumsum([len(tasks[k]) for k in keys])]).tolist()
    return {"fidx": fidx, "nf": nf, "first": first, "row_off": row_off, "n_blocks": row_off[-1],
            "task_slot": slot, "task_off": off, "entries": [c for k in keys for c in tasks[k]]}


def _structure(n, fixed, edges, weight=None):
    eye = np.broadcast_to(np.eye(4, dtype=np.float32), (n, 4, 4))
    g = {"S": eye, "fixed": np.asarray(fixed, np.uint8), "edges": np.asarray(edges, np.int32).reshape(-1, 2),
         "Z": np.broadcast_to(np.eye(4, dtype=np.float32), (len(edges), 4, 4))}
    if weight is not None:
        g["weight"] = np.asarray(weight, np.float32)
    return g


def _plan_cases():
    rng = np.random.default_rng(3)
    chain = (6, [1, 0, 0, 0, 0, 0], [(k, k + 1) for k in range(5)], None)
    ring = (8, [1, 0, 0, 0, 0, 0, 0, 0], [(k, k + 1) for k in range(7)] + [(7, 0), (6, 2), (2, 6)], None)
    perm = rng.permutation(9)
    edges = [(k, k + 1) for k in range(8)] + [(8, 0), (2, 6)]
    fixed = np.zeros(9, int)
    fixed[perm[0]] = 1
    permuted = (9, fixed.tolist(), [(int(perm[i]), int(perm[j])) for i, j in edges], None)
    star = (7, [0, 0, 0, 1, 0, 0, 1], [(3, k) for k in (0, 1, 2, 4, 5)] + [(5, 6), (1, 4), (0, 5)],
            [1, 2, 0.5, 1, 1, 1, 0, 3])  # two fixed nodes, one edge of weight 0
    return {"chain": chain, "ring": ring, "permuted ring": permuted, "star": star}


@pytest.mark.parametrize("name", ["chain", "ring", "permuted ring", "star"])
def test_plan_matches_its_restatement(name, tmp_path):
    n, fixed, edges, weight = _plan_cases()[name]
    # in a batch of two, so that the second graph's bases are not 0
    graphs = [_structure(3, [1, 0, 0], [(0, 1), (1, 2)], None if weight is None else [1, 1]),
              _structure(n, fixed, edges, weight)]
    out = _run("plan", graphs, tmp_path)
    assert out["status"] == [R.OK, R.OK] and len(out["graphs"]) == 2
    got, want = out["graphs"][1], _restated_plan(n, fixed, edges, weight)
    assert out["fidx"][3:] == want["fidx"]
    for k in ("nf", "first", "row_off", "n_blocks", "task_slot", "task_off", "entries"):
        assert got[k] == want[k], k
    assert (got["batch_index"], got["n"], got["m"]) == (1, n, len(edges))
    # the scratch: S, Z^-1, the edge records, the envelope, the gradient and the step, after the first graph's
    size = lambda n, m, nf, nb: 16 * n + 16 * m + 112 * m + 49 * nb + 14 * nf
    assert got["scratch0"] == size(3, 2, 2, 3)
    assert out["scratch"] == got["scratch0"] + size(n, len(edges), want["nf"], want["n_blocks"])
    if name == "chain":
        assert got["first"] == [0, 0, 1, 2, 3] and got["n_blocks"] == 9
    if name == "ring":  # node 7 closes on the fixed node: no long row; (6, 2) twice shares one block
        assert got["first"] == [0, 0, 1, 2, 3, 1, 5]


# ---------------------------------------------------------------------------------------------
# through the library, without a device
# ---------------------------------------------------------------------------------------------
def test_argument_errors():
    import picp_amd
    L = picp_amd.lib()
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)
    S = np.eye(4, dtype=np.float32).reshape(-1).copy()
    out = np.zeros(16, np.float32)
    fixed = np.ones(1, np.uint8)
    fp, u8 = picp_amd._fptr, lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    call = lambda n, no, eo, prm=None, S=S: L.picp_pgo_batch(0, n, no, eo, fp(S) if S is not None else None, u8(fixed),
                                                            None, None, None, prm, fp(out), None, None, None, None,
                                                            None, None)
    assert call(-1, i64(0), i64(0)) == picp_amd.ERR_ARG
    assert call(1, None, i64(0, 0)) == picp_amd.ERR_ARG
    assert call(1, i64(1, 2), i64(0, 0)) == picp_amd.ERR_ARG  # offsets start at 0
    assert call(2, i64(0, 1, 0), i64(0, 0, 0)) == picp_amd.ERR_ARG  # descend
    assert call(1, i64(0, 1), i64(0, 1)) == picp_amd.ERR_ARG  # an edge but no edge arrays
    assert call(1, i64(0, 1), i64(0, 0), S=None) == picp_amd.ERR_ARG
    assert L.picp_last_error()
    for bad in (dict(iterations=-1), dict(iterations=1001), dict(damping=-1.0), dict(damping=float("nan")),
                dict(eps=-1e-3), dict(eps=float("inf"))):
        assert call(1, i64(0, 1), i64(0, 0), ctypes.byref(picp_amd.default_pgo_params(**bad))) == picp_amd.ERR_ARG
    assert call(0, i64(0), i64(0)) == picp_amd.OK
    assert call(1, i64(0, 1), i64(0, 0)) == picp_amd.OK and (out == S).all()  # nothing to solve: no device needed
    us = np.zeros(1, np.float32)
    assert L.picp_pgo_batch_time(0, 1, i64(0, 1), i64(0, 0), fp(S), u8(fixed), None, None, None, None, 0,
                                 fp(us)) == picp_amd.ERR_ARG
    p = picp_amd.default_pgo_params()
    assert (p.with_scale, p.iterations, p.damping, p.eps) == (1, 10, 0.0, 0.0)


def _failing_graphs():
    a, _ = R.variants()["a"]

    def edit(**kw):
        g = {k: np.array(v) for k, v in a.items()}
        for k, (i, v) in kw.items():
            g[k][i] = v
        return g

    nan_S = edit(S=((3, 1, 2), np.nan))
    inf_Z = edit(Z=((5, 0, 3), np.inf))
    mirrored = edit(Z=((2, slice(None), 0), -a["Z"][2, :, 0]))  # det < 0
    singular = edit(S=((4, slice(0, 3), slice(0, 3)), 0.0))
    neg_w = edit(weight=(7, -1.0))
    nan_w = edit(weight=(0, np.nan))
    self_edge = edit(edges=((6, 1), a["edges"][6, 0]))
    high = edit(edges=((12, 0), 12))
    low = edit(edges=((0, 1), -1))
    loose = {k: np.array(v) for k, v in a.items()}  # node 12 joins nothing
    loose["S"] = np.concatenate([a["S"], a["S"][:1]])
    loose["fixed"] = np.concatenate([a["fixed"], [0]]).astype(np.uint8)
    cut = edit(weight=(4, 0.0))  # weight 0 on (4, 5), (11, 0) and (3, 9): nodes 5..11 reach no fixed node
    cut["weight"][11] = 0.0
    cut["weight"][12] = 0.0
    no_anchor = edit(fixed=(0, 0))
    n = 800  # a star about free node 1: row a of the envelope reaches back to it
    wide = _structure(n, [1] + [0] * (n - 1), [(0, 1)] + [(1, k) for k in range(2, n)])
    return {"nan_S": (nan_S, R.BAD_INPUT), "inf_Z": (inf_Z, R.BAD_INPUT), "mirrored": (mirrored, R.BAD_INPUT),
            "singular": (singular, R.BAD_INPUT), "neg_w": (neg_w, R.BAD_INPUT), "nan_w": (nan_w, R.BAD_INPUT),
            "self_edge": (self_edge, R.BAD_EDGE), "high": (high, R.BAD_EDGE), "low": (low, R.BAD_EDGE),
            "loose": (loose, R.DISCONNECTED), "cut": (cut, R.DISCONNECTED), "no_anchor": (no_anchor, R.DISCONNECTED),
            "wide": (wide, R.TOO_LARGE)}


def test_every_failure_gives_its_status_and_unchanged_outputs():
    """None of these graphs runs, so the library answers without a device."""
    import picp_amd
    F = _failing_graphs()
    assert sum(a - 0 + 1 for a in range(1, 799)) > MAX_BLOCKS  # `wide` is past the cap
    for with_w in (True, False):
        names = [k for k in F if with_w == ("weight" in F[k][0])]
        got = picp_amd.pose_graph_batch([F[k][0] for k in names])
        for k, o in zip(names, got):
            assert o["status"] == F[k][1], k
            assert o["steps"] == 0 and o["cost_initial"] == 0.0 and o["cost_final"] == 0.0
            np.testing.assert_array_equal(_bits(o["S"]), _bits(F[k][0]["S"]), err_msg=k)
    # an input failure comes before an edge failure, and that before the connectivity
    both = {k: np.array(v) for k, v in F["self_edge"][0].items()}
    both["S"][1, 0, 0] = np.nan
    both["fixed"][0] = 0
    edge = {k: np.array(v) for k, v in F["self_edge"][0].items()}
    edge["fixed"][0] = 0
    got = picp_amd.pose_graph_batch([both, edge])
    assert [o["status"] for o in got] == [R.BAD_INPUT, R.BAD_EDGE]


def test_graphs_with_nothing_to_solve_succeed_unchanged():
    import picp_amd
    a, _ = R.variants()["a"]
    no_edge = {"S": a["S"][:3], "fixed": np.zeros(3, np.uint8), "edges": np.zeros((0, 2), np.int32),
               "Z": np.zeros((0, 4, 4), np.float32)}
    empty = {"S": np.zeros((0, 4, 4), np.float32), "fixed": np.zeros(0, np.uint8), "edges": np.zeros((0, 2), np.int32),
             "Z": np.zeros((0, 4, 4), np.float32)}
    got = picp_amd.pose_graph_batch([no_edge, empty])
    assert [o["status"] for o in got] == [R.OK, R.OK] and [o["steps"] for o in got] == [0, 0]
    np.testing.assert_array_equal(_bits(got[0]["S"]), _bits(no_edge["S"]))
    assert got[1]["S"].shape == (0, 4, 4)
    assert picp_amd.pose_graph_batch([]) == []


def test_host_solve_fails_per_graph_and_the_others_still_run(tmp_path):
    """The statuses of the plan and of the solve itself in one batch of the host program: a graph
    whose numbers leave double's range ends NOT_PD with its inputs, its neighbours are solved."""
    a, _ = R.variants()["a"]
    F = _failing_graphs()
    huge = {k: np.array(v) for k, v in a.items()}
    huge["S"][1:, :3, :3] *= np.float32(1e-30)  # scales 1e-30 against 1 and translations of 1e30:
    huge["S"][1:, :3, 3] = np.float32(1e30)     # the normal equations overflow
    huge["Z"][:, :3, 3] = np.float32(-3e38)
    graphs = [a, F["nan_S"][0], huge, F["loose"][0], a]
    out = _run("solve", graphs, tmp_path)
    assert out["status"] == [R.OK, R.BAD_INPUT, R.NOT_PD, R.DISCONNECTED, R.OK]
    off = np.concatenate([[0], np.cumsum([len(g["S"]) for g in graphs])])
    for k in (1, 2, 3):
        np.testing.assert_array_equal(_bits(_S_of(out, off[k], off[k + 1])), _bits(graphs[k]["S"]))
    np.testing.assert_array_equal(_bits(_S_of(out, off[0], off[1])), _bits(_S_of(out, off[4], off[5])))
    R.check_against("a", _S_of(out, off[0], off[1]), out["cost_final"][0], "host, in a failing batch ")
    assert out["steps"][0] == 10 and out["steps"][1] == 0 and out["steps"][3] == 0


def test_segment_graph_builds_the_chain_and_the_extra_edges():
    from picp_amd.evaluate import chain_similarities, segment_graph
    Z = R.exp(np.random.default_rng(5).normal(0, 0.3, (4, 7))).astype(np.float32)
    g = segment_graph(Z[:3], extra=[(0, 3, Z[3]), (2, 0, Z[0])])
    assert g["edges"].tolist() == [[0, 1], [1, 2], [2, 3], [0, 3], [2, 0]] and g["edges"].dtype == np.int32
    assert g["fixed"].tolist() == [1, 0, 0, 0] and g["fixed"].dtype == np.uint8
    np.testing.assert_array_equal(g["Z"], np.stack([Z[0], Z[1], Z[2], Z[3], Z[0]]))
    np.testing.assert_array_equal(g["S"], np.stack(chain_similarities(Z[:3])).astype(np.float32))
    # the chain initialisation satisfies the chain edges: only the extra edges have a residual
    Zi = R.inv(np.stack([R.canonical(z) for z in g["Z"]]))
    r = np.linalg.norm(R.residuals(np.stack([R.canonical(s) for s in g["S"]]), g["edges"].astype(np.int64), Zi), axis=1)
    assert (r[:3] < 1e-6).all() and (r[3:] > 1e-2).all()
    lone = segment_graph([])
    assert lone["S"].shape == (1, 4, 4) and lone["edges"].shape == (0, 2) and lone["Z"].shape == (0, 4, 4)
