"""The layouts of a batch that tests/test_gpu_round_tail.py does not reach, solved on the device.

Graph mode with one item per lane, with float4 lanes and a ragged last block, with ragged tables
and an empty problem, and with the streaming-share block table; a persistent and a block candidate
laid out without hand-offs (PICP_RESIDENT_BLOCKS_PER_CU=0: residency 0/0, no fallback); and a
batch created after a smaller one of the same process was solved and destroyed.  The cases and how
one is run are in tools/layout_golden.py, which also writes the golden file.

Each case is held to
  * the oracle, under the rule of test_gpu_parity.py (its pose tolerance, its helpers);
  * two replays bit-identical;
  * the mode, block count, residency and fallback count, and the poses and statistics of two
    consecutive solves, of the build before the layout became a plan (csrc/picp_layout.cpp), bit
    for bit (tests/golden/layout/parent.npz, written with that build): the plan changes no kernel
    and no kernel argument.

The streaming-share case is sized by the device's CU count (cu_dependent in the case table): its
golden arrays were written on an MI355X (256 CUs) together with its block count, and are compared
only where the block count matches the recorded one.  The resident block count of a hand-off
layout scales with the CU count and is compared where that matches the recorded one.  Every
other case asserts the recorded layout and the golden arrays unconditionally.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_parity import THR, _assert_n_in_explained, _pose_tol

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "layout", "parent.npz")

_spec = importlib.util.spec_from_file_location("layout_golden", os.path.join(ROOT, "tools", "layout_golden.py"))
LG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(LG)
CASES = LG.CASES
assert LG.THR == THR


@functools.lru_cache(maxsize=None)
def _oracle_ref(name):
    import oracle as O
    return [O.solve_soa(p["T_init"], p["K"], 480, 640, p["x"], p["y"], p["z"], p["u"], p["v"], THR,
                        mode=O.MODE_F64, max_rounds=LG.ROUNDS, conv_eps=-1.0) for p in LG.problems(name)]


@pytest.mark.parametrize("name", list(CASES))
def test_layout(native, oracle, name):
    from picp_amd import synth
    c = CASES[name]
    got = LG.run_case(native, name)
    layout = dict(zip(LG.LAYOUT, (int(v) for v in got["layout"])))
    print(name, layout)
    assert LG.MODES[layout["mode"]] == c["expect_mode"]
    assert layout["fallbacks"] == 0
    if "PICP_RESIDENT_BLOCKS_PER_CU" in c["env"]:  # laid out without hand-offs
        assert layout["handoff_grid"] == 0 and layout["resident_blocks"] == 0
    # two replays: bit-identical
    for k in ("poses", "stats", "chi"):
        np.testing.assert_array_equal(got[k], got[k + "2"])
    # the oracle
    for i, (p, (T_ref, st_ref)) in enumerate(zip(LG.problems(name), _oracle_ref(name))):
        n = len(p["xyz"])
        st = dict(zip(LG.STAT_INT, (int(v) for v in got["stats"][i])))
        print("%s[%d] n %d se3 %.3g stats %s oracle %s" % (name, i, n, synth.se3_log_norm(got["poses"][i], T_ref), st, st_ref))
        assert synth.se3_log_norm(got["poses"][i], T_ref) < _pose_tol(n), (name, i)
        _assert_n_in_explained(p["K"], p["xyz"], p["uv"], got["poses"][i], T_ref, st["n_in"], st_ref["n_in"])
        assert st["rounds"] == LG.ROUNDS, (name, i)  # conv_eps < 0: every round runs
        if n >= 3:
            assert st_ref["rounds"] == LG.ROUNDS, (name, i)
    # the build before the plan, bit for bit
    with np.load(GOLDEN_FILE) as g:
        assert name + "/poses" in g.files, "no golden for %s" % name
        want = dict(zip(LG.LAYOUT, (int(v) for v in g[name + "/layout"])))
        same_partition = want["n_blocks"] == layout["n_blocks"]
        if not c["cu_dependent"]:
            assert same_partition, (name, want, layout)
        if same_partition:
            if int(g["num_cu"]) != LG.num_cu():
                want["resident_blocks"] = layout["resident_blocks"]
            assert layout == want, name
            for k in ("poses", "stats", "chi"):
                np.testing.assert_array_equal(got[k], g[name + "/" + k], err_msg="%s %s" % (name, k))
