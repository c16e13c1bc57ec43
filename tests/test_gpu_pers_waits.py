"""The follower's pose wait and the solvers' sweep of the persistent kernel: what a round waits for.

A follower block leaves one pose poll in flight when it has the round's pose; the poll keeps its
registers until the next round's wait consumes it, and nothing on the way there may wait for it
(DESIGN.md 4.2).  How a block waits must never change what it computes, so every case is held,
bit for bit, to arrays recorded from the build before the waits were changed
(tests/golden/pers_waits/parent.npz, written by tools/pers_waits_golden.py with that build).

Shapes: the smallest persistent frames at which a follower's wait takes another path -- one
follower (9 x 512 - 5), one solver with two followers and the rest with one (17 x 512), a follower
block that holds a single item (17 x 512 + 1), two items per lane (140000, the solvers' sweep of
that shape) -- each with both outlier policies, and the 100k frame of the headline workload solved
on a quiet device and beside device-to-device copies on a second stream: a hand-off must not
depend on timing.  The 17 x 512 case is also held to the oracle under the rule of
test_gpu_parity.py, which guards the golden file itself.

The 140000 frame is partitioned by the device's CU count; its golden arrays were written on an
MI355X (256 CUs) together with the block count, and the comparison applies where the block count
matches the recorded one (as in test_gpu_round_tail.py).  Every other case asserts the recorded
block count."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_parity import THR, _assert_n_in_explained, _pose_tol

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "pers_waits", "parent.npz")

_spec = importlib.util.spec_from_file_location("pers_waits_golden", os.path.join(ROOT, "tools", "pers_waits_golden.py"))
PW = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PW)
CASES = PW.CASES
assert PW.THR == THR


def _assert_golden(name, nb, run):
    with np.load(GOLDEN_FILE) as g:
        assert name + "/poses" in g.files, "no golden for %s" % name
        same_partition = int(g[name + "/n_blocks"]) == int(nb)
        if not CASES[name]["cu_dependent"]:
            assert same_partition, (name, int(g[name + "/n_blocks"]), int(nb))
        if same_partition:
            for k in ("poses", "stats", "chi"):
                np.testing.assert_array_equal(run[k], g[name + "/" + k], err_msg="%s %s" % (name, k))


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("c2_100k")])
def test_follower_wait_shapes_match_parent(native, name):
    nb, runs = PW.run_case(native, name)
    for k in ("poses", "stats", "chi"):  # two replays: bit-identical
        np.testing.assert_array_equal(runs[0][k], runs[1][k])
    _assert_golden(name, nb, runs[0])


@pytest.mark.parametrize("keep", [0, 1])
def test_two_followers_match_oracle(native, oracle, keep):
    from picp_amd import synth
    name = "followers2_keep%d" % keep
    c, p = CASES[name], PW.problem(name)
    _, runs = PW.run_case(native, name, solves=1)
    T_ref, st_ref = oracle.solve_soa(p["T_init"], p["K"], 480, 640, p["x"], p["y"], p["z"], p["u"], p["v"], THR,
                                     max_rounds=c["rounds"], conv_eps=-1.0, keep_outliers=keep,
                                     mode=oracle.MODE_F64)
    st = dict(zip(PW.STAT_INT, (int(v) for v in runs[0]["stats"][0])))
    err = synth.se3_log_norm(runs[0]["poses"][0], T_ref)
    print("%s se3 %.3g stats %s oracle %s" % (name, err, st, st_ref))
    assert err < _pose_tol(c["n"])
    assert st["rounds"] == st_ref["rounds"] == c["rounds"]
    _assert_n_in_explained(p["K"], p["xyz"], p["uv"], runs[0]["poses"][0], T_ref, st["n_in"], st_ref["n_in"])


def test_headline_frame_quiet_and_beside_copies(native):
    name = "c2_100k_keep0"
    nb, quiet = PW.run_case(native, name, solves=1)
    _assert_golden(name, nb, quiet[0])
    with PW.busy_copies():
        nb2, busy = PW.run_case(native, name, solves=3)
    assert int(nb2) == int(nb)
    for run in busy:
        _assert_golden(name, nb, run)
