"""The timed first pass of the persistent solvers' sweep: when a pass is issued must never change
what a round computes.

A solver block issues the first pass of its granule sweep PICP_SWEEP_LAG_NS after its
post-linearize barrier; only the granules' tags are trusted, so the lag can only
cost time.  Every case of tools/sweep_lag_cases.py -- one block, eight solvers and no follower, nine
blocks, the smallest frame with two items per lane -- is solved with the lag at 0 (the pass straight
after the barrier), at the shipped default and at 20 us (far past every follower's publish), each in
a fresh process because the variable is read once, with the pinhole and with the general-K kernels.
The results must be bit-identical across the three lags and across a replay on the same batch, no
solve may have fallen back to graph mode, and each result is held to the oracle under the rule of
test_gpu_parity.py."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import THR, _assert_n_in_explained, _pose_tol

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("sweep_lag_cases", os.path.join(ROOT, "tools", "sweep_lag_cases.py"))
SL = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(SL)
assert SL.THR == THR

LAGS = ("0", None, "20000")  # None: the shipped default (the variable unset)


def _run(tmp_path, lag, general_k):
    out = str(tmp_path / ("lag_%s_%d.npz" % (lag, general_k)))
    env = {k: v for k, v in os.environ.items() if k not in ("PICP_SWEEP_LAG_NS", "PICP_FORCE_GENERAL_K", "PICP_MODE")}
    if lag is not None:
        env["PICP_SWEEP_LAG_NS"] = lag
    cmd = [sys.executable, os.path.join(ROOT, "tools", "sweep_lag_cases.py"), "--out", out]
    subprocess.run(cmd + (["--general-k"] if general_k else []), check=True, env=env, timeout=120)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("general_k", [0, 1])
def test_results_do_not_depend_on_the_lag(native, oracle, tmp_path, general_k):
    from picp_amd import synth
    runs = [_run(tmp_path, lag, general_k) for lag in LAGS]
    for name, (n, rounds) in SL.CASES.items():
        for lag, r in zip(LAGS, runs):
            assert int(r[name + "/fallbacks"]) == 0, (name, lag)
            for k in ("poses", "stats", "chi"):
                key = "%s/%s" % (name, k)
                np.testing.assert_array_equal(r[key], r[key + "2"], err_msg="%s lag %s replay" % (key, lag))
                np.testing.assert_array_equal(r[key], runs[0][key], err_msg="%s lag %s against lag 0" % (key, lag))
            assert int(r[name + "/n_blocks"]) == int(runs[0][name + "/n_blocks"])
        p = SL.problem(name)
        T_ref, st_ref = oracle.solve_soa(p["T_init"], p["K"], 480, 640, p["x"], p["y"], p["z"], p["u"], p["v"], THR,
                                         max_rounds=rounds, conv_eps=-1.0, mode=oracle.MODE_F64)
        pose = runs[0][name + "/poses"][0]
        st = dict(zip(SL.STAT_INT, (int(v) for v in runs[0][name + "/stats"][0])))
        err = synth.se3_log_norm(pose, T_ref)
        print("%s generalK %d blocks %d se3 %.3g stats %s" % (name, general_k, int(runs[0][name + "/n_blocks"]), err, st))
        assert err < _pose_tol(n)
        assert st["rounds"] == st_ref["rounds"] == rounds
        _assert_n_in_explained(p["K"], p["xyz"], p["uv"], pose, T_ref, st["n_in"], st_ref["n_in"])
