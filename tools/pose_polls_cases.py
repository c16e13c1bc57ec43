#!/usr/bin/env python3
"""The cases of tests/test_gpu_pose_polls.py and how they are run.

    PICP_POSE_LAG_NS=<ns> python tools/pose_polls_cases.py --out FILE [--cases A,B] [--busy]

solves every case of tools/pers_waits_golden.py (or the ones named) twice on one persistent-mode
batch in this process -- the lag of the followers' first pose poll is read once per process -- and
writes <case>/poses, /stats, /chi of both solves (the second with suffix 2), /n_blocks and
/fallbacks to FILE.  With --busy the solves run beside the device-to-device copies of
pers_waits_golden.busy_copies().  The cases are the smallest persistent frames at which a
follower's pose wait takes another path (one follower; a solver with two followers; a follower
block that holds one item; two items per lane, whose kernels keep the two-poll wait) and the 100k
frame of the headline workload.  Needs a GPU."""
import argparse
import contextlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "02-visualodometry_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

_spec = importlib.util.spec_from_file_location("pers_waits_golden", os.path.join(ROOT, "tools", "pers_waits_golden.py"))
PW = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(PW)
CASES = PW.CASES
HEADLINE = "c2_100k_keep0"
KEYS = ("poses", "stats", "chi")


def run_all(native, names, busy=False):
    out = {}
    native.lib()  # loads the HIP runtime, which busy_copies looks up
    for name in names:
        with (PW.busy_copies() if busy else contextlib.nullcontext()):
            # run_case asserts that no solve fell back to graph mode (a timed-out hand-off)
            nb, runs = PW.run_case(native, name, solves=2)
        for suffix, run in zip(("", "2"), runs):
            for k in KEYS:
                out["%s/%s%s" % (name, k, suffix)] = run[k]
        out[name + "/n_blocks"] = nb
        out[name + "/fallbacks"] = np.array(0, np.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated case names")
    ap.add_argument("--busy", action="store_true", help="solve beside device-to-device copies on a second stream")
    args = ap.parse_args()
    import picp_amd
    np.savez(args.out, **run_all(picp_amd, [n for n in args.cases.split(",") if n], busy=args.busy))


if __name__ == "__main__":
    main()
