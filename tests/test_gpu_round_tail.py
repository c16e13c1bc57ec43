"""The serial finish of a round (combine, solve, publish) of the persistent and block kernels.

Every shape is the smallest at which that tail takes another path: a solver block without
followers, all eight solvers, one follower, sweep lanes with one and with two granule loads (the
unguarded double sums add the never-loaded zeros), every lane with eight loads (256 blocks), two
items per lane (the staggered sweep); both outlier policies, the general-K kernels, a damping
whose sum with the diagonal rounds (a wrong per-lane addend shows), and the block kernel unsplit,
split, and with a frame that stops at the min-inlier check (total_word's words go through the
early-out of finish_round_pose).  The cases and how one is run are in tools/round_tail_golden.py,
which also writes the golden file.

Each case is held to
  * the oracle, under the rule of test_gpu_parity.py (its pose tolerance, its helpers);
  * rounds, n_in, n_projected, ok and converged equal to the oracle's (n_projected: the oracle's
    linearization at its pose before the last round, where the last round's statistics are taken);
  * two replays bit-identical;
  * the poses and statistics of the build before the tail was rewritten, bit for bit
    (tests/golden/round_tail/parent.npz, written with that build).

Cases that depend on the device's CU count (cu_dependent in the case table): a single frame of
more than 512 x CUs correspondences (131072, 140000) is partitioned by the CU count, and so is
the default split of a block-mode batch (6 x 20000, the min-inlier batch).  Their golden arrays
were written on an MI355X (256 CUs) together with each case's block count; on a device that
partitions such a case differently its sums run in another order, so for these cases alone the
golden comparison applies only where the block count matches the recorded one.  Every other case
asserts the recorded block count and the golden arrays unconditionally.  The oracle and replay
assertions hold for all of them everywhere.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_parity import THR, _assert_n_in_explained, _pose_tol

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "round_tail", "parent.npz")

_spec = importlib.util.spec_from_file_location("round_tail_golden", os.path.join(ROOT, "tools", "round_tail_golden.py"))
RT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(RT)
CASES = RT.CASES
assert RT.THR == THR


@functools.lru_cache(maxsize=None)
def _oracle_ref(name):
    """Per frame: the oracle's pose and statistics, and n_projected of its last round."""
    import oracle as O
    c = CASES[name]
    ref = []
    for p in RT.problems(name):
        a = (p["K"], 480, 640, p["x"], p["y"], p["z"], p["u"], p["v"], THR)
        kw = dict(damping=c["damping"], min_inliers=c["min_inliers"], keep_outliers=c["keep"], mode=O.MODE_F64)
        T, st = O.solve_soa(p["T_init"], *a, max_rounds=c["rounds"], conv_eps=c["conv_eps"], **kw)
        # the pose the last round linearized at: conv_eps < 0 there, so that the loop rule cannot end it sooner
        T_prev, _ = O.solve_soa(p["T_init"], *a, max_rounds=st["rounds"] - 1, conv_eps=-1.0, **kw)
        lin = O.linearize_soa(T_prev, *a, keep_outliers=c["keep"], mode=O.MODE_F64)
        ref.append((T, st, lin["n_projected"]))
    return ref


@pytest.mark.parametrize("name", list(CASES))
def test_round_tail(native, oracle, tmp_path, name):
    from picp_amd import synth
    c = CASES[name]
    if c["own_process"]:
        got = RT.run_case_in_own_process(name, str(tmp_path / "case.npz"))
    else:
        got = RT.run_case(native, name)
    # two replays: bit-identical
    np.testing.assert_array_equal(got["poses"], got["poses2"])
    np.testing.assert_array_equal(got["stats"], got["stats2"])
    np.testing.assert_array_equal(got["chi"], got["chi2"])
    # the oracle
    for i, (p, (T_ref, st_ref, nproj_ref)) in enumerate(zip(RT.problems(name), _oracle_ref(name))):
        n = c["sizes"][i]
        st = dict(zip(RT.STAT_INT, (int(v) for v in got["stats"][i])))
        print("%s[%d] se3 %.3g stats %s oracle %s n_projected %d" % (
            name, i, synth.se3_log_norm(got["poses"][i], T_ref), st, st_ref, nproj_ref))
        assert synth.se3_log_norm(got["poses"][i], T_ref) < _pose_tol(n), (name, i)
        _assert_n_in_explained(p["K"], p["xyz"], p["uv"], got["poses"][i], T_ref, st["n_in"], st_ref["n_in"])
        assert st["rounds"] == st_ref["rounds"], (name, i)
        assert st["n_in"] == st_ref["n_in"], (name, i)
        assert st["n_projected"] == nproj_ref, (name, i)
        assert st["ok"] == st_ref["ok"], (name, i)
        assert st["converged"] == int(st_ref["converged"]), (name, i)
    # the build before the rewrite, bit for bit
    with np.load(GOLDEN_FILE) as g:
        assert name + "/poses" in g.files, "no golden for %s" % name
        same_partition = int(g[name + "/n_blocks"]) == int(got["n_blocks"])
        if not c["cu_dependent"]:
            assert same_partition, (name, int(g[name + "/n_blocks"]), int(got["n_blocks"]))
        if same_partition:
            for k in ("poses", "stats", "chi"):
                np.testing.assert_array_equal(got[k], g[name + "/" + k], err_msg="%s %s" % (name, k))
