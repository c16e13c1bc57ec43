"""What the batched RANSAC solvers share (csrc/picp_ransac.h, csrc/picp_ransac_plan.h) on the CPU:
bin/ransac_check, a host-only program built with ASan/UBSan from those sources, prints the sampling
function's triples and the plan of a score grid.  The triples are held to tests/pnp_ref.py, the plan
to the invariants of the grid (every item in exactly one block, the blocks in order, the slicing
rule) and to its two limits."""
import json
import os
import subprocess

import pytest

import pnp_ref as R
from conftest import PKG

BIN = os.path.join(PKG, "bin", "ransac_check")
I32 = 2 ** 31 - 1
SCORE_TILE, HYP_TILE = 1024, 64  # any tiles do for the plan; these are the solvers'


def _run(*args):
    out = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


# ---------------------------------------------------------------------------------------------
# the sampling function
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 6, 7, 64, I32 - 1024])
def test_samples_equal_the_reference(n):
    H = 257  # h in 0..256
    for seed in (0, 0xDEADBEEFCAFE1234):
        for i in (0, 1, 65535, 2 ** 24 - 1):
            got = [tuple(int(v) for v in line.split()) for line in _run("samples", seed, i, H, n).splitlines()]
            assert len(got) == H
            for h, t in enumerate(got):
                assert t == tuple(int(v) for v in R.sample_triple(seed, i, h, n)), (seed, i, h)
                assert len(set(t)) == 3 and min(t) >= 0 and max(t) < n, (seed, i, h)


# ---------------------------------------------------------------------------------------------
# the plan of the score grid
# ---------------------------------------------------------------------------------------------
def _plan(sizes, hyp, score_tile=SCORE_TILE, hyp_tile=HYP_TILE):
    return json.loads(_run("plan", score_tile, hyp_tile, hyp, *sizes))


def _expand(sizes):
    out = []
    for s in sizes:
        if isinstance(s, str):
            size, count = s.split("x")
            out += [int(size)] * int(count)
        else:
            out.append(s)
    return out


PLAN_CASES = [
    ([1025], 130), ([5] * 400, 130), ([0], 64), ([], 64), ([0, 3, 0, 1024, 1025, 0, 2049, 1], 256),
    ([1], 1), ([1024] * 1024, 65536), ([1024] * 1025, 65536), ([7] * 513, 200), ([100000], 16),
    (["4x70001"], 1), ([3000, 0, 0, 5], 65536),
]


@pytest.mark.parametrize("sizes,hyp", PLAN_CASES, ids=[str(i) for i in range(len(PLAN_CASES))])
@pytest.mark.parametrize("tiles", [(SCORE_TILE, HYP_TILE), (7, 3)])
def test_plan_covers_every_item_once_in_order(sizes, hyp, tiles):
    score_tile, hyp_tile = tiles
    p = _plan(sizes, hyp, score_tile, hyp_tile)
    n = _expand(sizes)
    assert "error" not in p
    want = [(i, first) for i, size in enumerate(n) for first in range(0, size, score_tile)]
    # every item of every problem lies in exactly one block; problem order, then by offset; an
    # empty problem has no block
    assert [tuple(b) for b in p["blk"]] == want
    assert p["nb"] == len(want) == sum(-(-size // score_tile) for size in n)
    tiles_h = -(-hyp // hyp_tile)
    assert p["hsplit"] == min(tiles_h, max(1, 1024 // max(p["nb"], 1)))
    assert 1 <= p["hsplit"] <= tiles_h


def test_plan_of_the_two_pinned_shapes():
    """The shapes tests/test_gpu_pnp.py and tests/test_gpu_sim3.py pin the tile walk with."""
    a = _plan([1025], 130)
    assert a["blk"] == [[0, 0], [0, 1024]] and a["hsplit"] == 3
    b = _plan([5] * 400, 130)
    assert b["nb"] == 400 and b["hsplit"] == 2


def test_plan_limits():
    tile = SCORE_TILE
    big = 2 ** 20  # a tile at which the largest accepted problem has few blocks
    ok = _plan([I32 - big], 64, score_tile=big)
    assert "error" not in ok and ok["nb"] == 2047 and ok["blk"][-1] == [0, 2046 * big]
    assert _plan([I32 - big + 1], 64, score_tile=big) == {"error": "check: a problem has too many items"}
    assert _plan([I32 - tile + 1], 64) == {"error": "check: a problem has too many items"}
    assert _plan([5, I32 - tile + 1, 5], 64) == {"error": "check: a problem has too many items"}
    # more blocks than INT32_MAX / 4: rejected before any table is built (it would hold 629 million entries)
    assert _plan(["%dx300" % (I32 - 1025)], 64) == {"error": "check: too many items in one call"}
