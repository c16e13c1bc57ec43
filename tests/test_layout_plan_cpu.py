"""The layout plan of a batch (csrc/picp_layout.cpp) on the CPU: bin/layout_plan, a host-only
program built with ASan/UBSan from that file alone, prints the plan of one case as JSON.

Every case is held to the invariants of a layout (each item in exactly one block-table row, the
rows of a problem contiguous, offsets multiples of 4, the sync area's regions disjoint, in bounds
and on 128-B lines, a hand-off grid no larger than what is resident, no hand-off after a timed-out
one), and to the decisions of the build before the plan was split out of the runtime: TABLE was
obtained by compiling that build's layout code verbatim with the same stubbed limits (a block
holds 4096 items, 512 threads at every split, 4 register items per lane at split 4 and 8
otherwise, 512-thread persistent blocks) and occupancy answers (persistent 2 per CU, block split 1
or 2: 1, split 4: 2)."""
import json
import os
import subprocess

import pytest

from conftest import PKG

BIN = os.path.join(PKG, "bin", "layout_plan")
GRAPH, PERSISTENT, BLOCK = 0, 1, 2
OCC = dict(persistent=2, block1=1, block2=1, block4=2)
OVERRIDES = ("PICP_MODE", "PICP_ITEMS_PER_BLOCK", "PICP_BLOCK_NPT", "PICP_PERSIST_BLOCKS", "PICP_BLOCK_SPLIT",
             "PICP_STREAM_SHARE", "PICP_RESIDENT_BLOCKS_PER_CU")


def plan(cus, sizes, env=None, no_handoff=False, **occ):
    o = dict(OCC, **occ)
    e = {k: v for k, v in os.environ.items() if k not in OVERRIDES}
    e.update(env or {})
    args = [BIN, str(cus), str(int(no_handoff)), str(o["persistent"]), str(o["block1"]), str(o["block2"]), str(o["block4"])]
    r = subprocess.run(args + [str(n) for n in sizes], env=e, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])  # the sanitizers report there
    return json.loads(r.stdout)


def check_invariants(P, sizes, no_handoff):
    assert len(P["probs"]) == len(sizes) == len(P["plane_off"])
    assert P["nblk"] == len(P["blocks"]) == sum(p[3] for p in P["probs"])
    assert P["total"] == sum(sizes) and P["max_n"] == max(sizes)
    blk, end = 0, 0
    for i, (n, (off, pn, blk0, nb)) in enumerate(zip(sizes, P["probs"])):
        assert pn == n and off == P["plane_off"][i] and off % 4 == 0 and off >= end
        assert blk0 == blk and nb >= 1  # the rows of problem i are [blk0, blk0 + nb)
        rows = P["blocks"][blk0:blk0 + nb]
        assert all(r[0] == i and r[2] >= 0 for r in rows)
        covered = sorted((r[1], r[1] + r[2]) for r in rows if r[2] > 0)
        at = 0
        for first, last in covered:  # every item in exactly one row
            assert first == at, (i, first, at)
            at = last
        assert at == n and sum(r[2] for r in rows) == n
        assert all(r[1] % 4 == 0 for r in rows if r[2] > 0)  # float4 lanes start on a float4
        blk += nb
        end = off + n
    assert P["plane_len"] >= max(end, 4) and P["plane_len"] % 4 == 0
    if P["uniform"]:
        assert len(set(sizes)) == 1 and P["n_u"] == sizes[0] and P["stride_u"] % 4 == 0 and P["stride_u"] >= P["n_u"]
        assert all(off == i * P["stride_u"] for i, off in enumerate(P["plane_off"]))
    hands_off = P["mode"] == PERSISTENT or (P["mode"] == BLOCK and P["split"] > 1)
    S = P["sync"]
    if hands_off:
        assert not no_handoff
        assert 1 <= P["handoff_grid"] <= P["handoff_resident"]
        regions = [S[k] for k in ("err", "pose", "gran", "tag") if S[k][1] > 0]
        assert ("pose" in S and S["pose"][1] > 0) == (P["mode"] == PERSISTENT)
        at = 0
        for off, size in sorted(regions):  # disjoint, in bounds
            assert off >= at
            at = off + size
        assert at <= S["bytes"]
        for k in ("err", "pose", "gran"):
            assert S[k][0] % 128 == 0
        assert S["tag"][0] % 4 == 0
        # the sizes the kernels index: 16 sets of 16 8-B granules per problem; 2 parities of 32 8-B
        # words per block; 2 parities of 64 8-B granules and one tag base per block of a split grid
        if P["mode"] == PERSISTENT:
            assert P["handoff_grid"] == P["nblk"]
            assert S["pose"][1] == len(sizes) * 16 * 16 * 8 and S["gran"][1] == 2 * P["nblk"] * 32 * 8
            assert S["tag"][1] == 4 * len(sizes)
        else:
            assert S["gran"][1] == 2 * P["handoff_grid"] * 64 * 8 and S["tag"][1] == 4 * P["handoff_grid"]
            assert P["handoff_grid"] >= P["split"] * len(sizes)
    else:
        assert P["handoff_grid"] == 0 and P["handoff_resident"] == 0 and S["bytes"] == 0
    if no_handoff:
        assert not hands_off
    assert P["vec"] == (4 if P["mode"] == GRAPH and P["ipb"] >= 1024 else 1)


NO_RES = {"PICP_RESIDENT_BLOCKS_PER_CU": "0"}
G1024 = {"PICP_MODE": "graph", "PICP_ITEMS_PER_BLOCK": "1024"}
# (CUs, sizes, overrides, no_handoff, occupancy), (mode, split, npt, ipb, vec, nblk, grid, resident), more
TABLE = [
    ((256, [300], {}, False, {}), (PERSISTENT, 1, 1, 512, 1, 1, 1, 512), {}),
    ((256, [131072], {}, False, {}), (PERSISTENT, 1, 1, 512, 1, 256, 256, 512), {}),
    ((256, [140000], {}, False, {}), (PERSISTENT, 1, 2, 1024, 1, 137, 137, 512), {}),
    ((256, [1200000], {}, False, {}), (GRAPH, 1, None, 2048, 4, 586, 0, 0), {}),
    ((256, [9000000], {}, False, {}), (GRAPH, 1, None, 17580, 4, 512, 0, 0), {"share": True}),
    ((256, [5000] * 8, {}, False, {}), (BLOCK, 2, 8, 512, 1, 80, 16, 256), {}),
    ((256, [5000] * 8, {"PICP_BLOCK_SPLIT": "1"}, False, {}), (BLOCK, 1, 8, 512, 1, 80, 0, 0), {}),
    ((256, [20000] * 6, {}, False, {}), (BLOCK, 4, 4, 512, 1, 240, 32, 512), {}),
    ((256, [20000] * 6, {}, False, {"block4": 0}), (BLOCK, 2, 8, 512, 1, 240, 16, 256), {}),
    ((256, [20000] * 6, NO_RES, False, {}), (BLOCK, 1, 8, 512, 1, 240, 0, 0), {}),
    ((256, [20000] * 6, {}, True, {}), (BLOCK, 1, 8, 512, 1, 240, 0, 0), {}),
    ((256, [300], NO_RES, False, {}), (GRAPH, 1, None, 512, 1, 1, 0, 0), {}),
    ((256, [300], {}, True, {}), (GRAPH, 1, None, 512, 1, 1, 0, 0), {}),
    ((256, [5000, 200, 0, 5000], {}, False, {}), (BLOCK, 2, 8, 512, 1, 22, 16, 256), {"plane_len": 10200}),
    ((256, [70000, 100], {}, False, {}), (GRAPH, 1, None, 512, 1, 138, 0, 0), {"plane_len": 70100}),
    ((256, [4096], {"PICP_MODE": "graph"}, False, {}), (GRAPH, 1, None, 512, 1, 8, 0, 0), {}),
    ((256, [5000], G1024, False, {}), (GRAPH, 1, None, 1024, 4, 5, 0, 0), {}),
    ((4, [8192], {}, False, {}), (PERSISTENT, 1, 4, 2048, 1, 4, 4, 8), {}),
    ((4, [8192], G1024, False, {}), (GRAPH, 1, None, 1024, 4, 8, 0, 0), {"share": True}),
]


def _even_blocks(sizes, ipb):
    return [[i, k * ipb, max(0, min(ipb, n - k * ipb))] for i, n in enumerate(sizes)
            for k in range(max(1, -(-n // ipb)))]


@pytest.mark.parametrize("case,expect,more", TABLE, ids=["%d-%s" % (i, "x".join(map(str, sorted(set(t[0][1])))))
                                                           for i, t in enumerate(TABLE)])
def test_plan_matches_the_table(case, expect, more):
    cus, sizes, env, no_handoff, occ = case
    P = plan(cus, sizes, env, no_handoff, **occ)
    print(case, {k: P[k] for k in P if k not in ("blocks", "probs", "plane_off")})
    check_invariants(P, sizes, no_handoff)
    mode, split, npt, ipb, vec, nblk, grid, resident = expect
    got = (P["mode"], P["split"], P["npt"] if npt is not None else None, P["ipb"], P["vec"], P["nblk"],
           P["handoff_grid"], P["handoff_resident"])
    assert got == expect
    if "plane_len" in more:
        assert P["plane_len"] == more["plane_len"]
    # the streaming-share re-partition replaces the even table and clears `uniform`
    assert (P["blocks"] != _even_blocks(sizes, P["ipb"])) == bool(more.get("share"))
    assert P["uniform"] == (0 if more.get("share") else int(len(set(sizes)) == 1))


def test_streaming_share_table():
    """4 CUs, 8192 items on 8 blocks of 1024: CU q's pair of blocks shares [2048 q, 2048 q + 2048),
    the older block q taking 0.64 of it rounded up to whole float4s."""
    P = plan(4, [8192], G1024)
    want = [None] * 8
    for q in range(4):
        want[q] = [0, 2048 * q, 1312]
        want[q + 4] = [0, 2048 * q + 1312, 736]
    assert P["blocks"] == want and P["uniform"] == 0
    check_invariants(P, [8192], False)
    P = plan(4, [8192], dict(G1024, PICP_STREAM_SHARE="0.5"))
    assert P["blocks"] == _even_blocks([8192], 1024) and P["uniform"] == 1


@pytest.mark.parametrize("env", [{}, {"PICP_BLOCK_NPT": "2"}, {"PICP_PERSIST_BLOCKS": "3"}, {"PICP_MODE": "persistent"},
                                 {"PICP_MODE": "block"}, {"PICP_BLOCK_SPLIT": "4"}, {"PICP_ITEMS_PER_BLOCK": "1022"}])
@pytest.mark.parametrize("no_handoff", [False, True])
def test_invariants_over_shapes(env, no_handoff):
    """Odd sizes, sizes around the tile and the mode thresholds, empty problems, more problems than
    CUs: the invariants alone."""
    shapes = [(256, [1]), (256, [0]), (256, [511, 513]), (256, [4095] * 3), (256, [4097, 8191, 0, 65536]),
              (256, [65537, 5]), (256, [7] * 300), (256, [100003]), (8, [9000] * 9), (256, [262145]),
              (2, [1 << 21])]
    for cus, sizes in shapes:
        check_invariants(plan(cus, sizes, env, no_handoff), sizes, no_handoff)


def test_argument_errors_keep_their_messages():
    assert plan(256, [])["error"] == "batch: n_problems must be >= 1"
    assert plan(256, [5, -1])["error"] == "batch: corr_offsets must be a prefix sum from 0"
    assert plan(256, [1 << 31])["error"] == "batch: a problem has more than 2^31-1 correspondences"
