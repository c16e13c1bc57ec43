#!/usr/bin/env python3
"""The cases of tests/test_gpu_sweep_lag.py and how they are run.

    PICP_SWEEP_LAG_NS=<ns> python tools/sweep_lag_cases.py --out FILE [--general-k]

solves every case twice in persistent mode in this process (the lag of the solvers' first sweep
pass and the camera path are read once per process) and writes <case>/poses, /stats, /chi of both
solves (the second with suffix 2), /n_blocks and /fallbacks to FILE.  The cases are the smallest
frames at which the timed pass takes another path: one block (the sweep has nothing to wait for),
eight solver blocks and no follower, nine blocks (one follower), and the smallest frame with two
items per lane on a device of up to 256 CUs (the staggered sweep: the second pass keeps its offset
from the timed first one).  Needs a GPU."""
import argparse
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "02-visualodometry_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

THR = 3000.0  # exec/icp_test.cpp:86
STAT_INT = ("n_in", "ok", "rounds", "converged", "n_projected")
# name: (correspondences, rounds): 50 rounds where the oracle is cheap
CASES = {"block1": (500, 50), "solvers8": (4096, 50), "blocks9": (9 * 512 - 5, 50), "npt2": (256 * 512 + 1, 5)}


@functools.lru_cache(maxsize=None)
def problem(name):
    from picp_amd import synth
    n = CASES[name][0]
    return synth.make_problem(n, seed=6000 + n % 997, outlier_frac=0.1, pixel_noise=0.5, shuffle=False)


def run_all(native):
    out = {}
    os.environ["PICP_MODE"] = "persistent"  # read when a batch is created
    for name, (n, rounds) in CASES.items():
        p = problem(name)
        b = native.Batch([n])
        info = b.info()
        assert info["mode"] == "persistent", info
        b.set_data(p["xyz"], p["uv"])
        for suffix in ("", "2"):
            b.set_poses(p["T_init"][None])
            b.solve(threshold=THR, max_rounds=rounds, conv_eps=-1.0)
            st = b.stats()
            out["%s/poses%s" % (name, suffix)] = b.poses()
            out["%s/stats%s" % (name, suffix)] = np.array([[s[k] for k in STAT_INT] for s in st], np.int32)
            out["%s/chi%s" % (name, suffix)] = np.array([[s["chi_in"], s["chi_out"]] for s in st], np.float32)
        out[name + "/n_blocks"] = np.array(info["n_blocks"], np.int32)
        # a timed-out hand-off re-runs the solve in graph mode, which sums in another order
        out[name + "/fallbacks"] = np.array(b.residency()["fallbacks"], np.int32)
        b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--general-k", action="store_true", help="the general-K kernels (PICP_FORCE_GENERAL_K=1)")
    args = ap.parse_args()
    if args.general_k:
        os.environ["PICP_FORCE_GENERAL_K"] = "1"  # before the library first looks at a camera
    import picp_amd
    np.savez(args.out, **run_all(picp_amd))


if __name__ == "__main__":
    main()
