#!/usr/bin/env python3
"""The cases of tests/test_gpu_round_tail.py, how one is run, and the golden file of a build.

    PICP_LIB=<library of the build to record> python tools/round_tail_golden.py

writes tests/golden/round_tail/parent.npz (keys <case>/poses, /stats, /chi, /n_blocks); the test
compares every later build with it bit for bit.  --case NAME --out FILE runs one case and writes
all of run_case's arrays: the test starts it for the case whose environment is read once per
process (PICP_FORCE_GENERAL_K).  The test loads this file for CASES and run_case; nothing here
depends on the tests.  Writing the golden file needs a GPU."""
import argparse
import functools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "02-visualodometry_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

THR = 3000.0  # exec/icp_test.cpp:86
STAT_INT = ("n_in", "ok", "rounds", "converged", "n_projected")


def _case(name, mode, sizes, rounds, seed, keep=0, of=0.1, conv_eps=-1.0, damping=1.0, min_inliers=0,
          env=None, own_process=False, cu_dependent=False):
    return dict(name=name, mode=mode, sizes=list(sizes), rounds=rounds, seed=seed, keep=keep, of=of,
                conv_eps=conv_eps, damping=damping, min_inliers=min_inliers, env=dict(env or {}),
                own_process=own_process, cu_dependent=cu_dependent)


def _cases():
    out = []
    # persistent mode, one frame; 50 rounds only where the oracle is cheap.  A frame of more than
    # 512 x CUs correspondences is partitioned by the CU count (picp_layout.cpp)
    for tag, n, rounds in (("solo", 300, 50), ("solvers8", 4096, 50), ("follower1", 9 * 512 - 5, 5),
                           ("blocks33", 33 * 512, 5), ("blocks256", 131072, 5), ("npt2", 140000, 5)):
        for keep in (0, 1):
            out.append(_case("pers_%s_keep%d" % (tag, keep), "persistent", [n], rounds, seed=4000 + n % 997,
                             keep=keep, cu_dependent=n > 33 * 512))
    # the launch-time camera path is read once per process: this case runs in a process of its own
    out.append(_case("pers_follower1_generalK", "persistent", [9 * 512 - 5], 5, seed=4101,
                     env={"PICP_FORCE_GENERAL_K": "1"}, own_process=True))
    out.append(_case("pers_blocks33_damping", "persistent", [33 * 512], 5, seed=4102, damping=0.3))
    out.append(_case("block_8x5000", "block", [5000] * 8, 50, seed=4200, conv_eps=1e-5,
                     env={"PICP_BLOCK_SPLIT": "1"}))
    # the default split of a block-mode batch is chosen by the CU count
    out.append(_case("block_6x20000", "block", [20000] * 6, 5, seed=4300, cu_dependent=True))
    out.append(_case("block_min_inliers", "block", [5000, 200, 5000], 5, seed=4400, min_inliers=1000,
                     cu_dependent=True))
    return out


CASES = {c["name"]: c for c in _cases()}


@functools.lru_cache(maxsize=None)
def problems(name):
    from picp_amd import synth
    c = CASES[name]
    return [synth.make_problem(n, seed=c["seed"] + i, outlier_frac=c["of"], pixel_noise=0.5, shuffle=False)
            for i, n in enumerate(c["sizes"])]


def run_case(native, name):
    """Solve the case twice on one batch.  Returns poses (P, 4, 4), the integer statistics (P, 5,
    STAT_INT order), chi (P, 2: chi_in, chi_out), the block count, and the second solve's arrays."""
    c = CASES[name]
    probs = problems(name)
    env = dict(c["env"], PICP_MODE=c["mode"])  # read when the batch is created
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        b = native.Batch(c["sizes"])
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    info = b.info()
    assert info["mode"] == c["mode"], info
    b.set_data(np.concatenate([p["xyz"] for p in probs]), np.concatenate([p["uv"] for p in probs]))
    runs = []
    for _ in range(2):
        b.set_poses(np.stack([p["T_init"] for p in probs]))
        b.solve(threshold=THR, max_rounds=c["rounds"], conv_eps=c["conv_eps"], keep_outliers=c["keep"],
                damping=c["damping"], min_inliers=c["min_inliers"])
        st = b.stats()
        runs.append((b.poses(), np.array([[s[k] for k in STAT_INT] for s in st], np.int32),
                     np.array([[s["chi_in"], s["chi_out"]] for s in st], np.float32)))
    b.close()
    return {"poses": runs[0][0], "stats": runs[0][1], "chi": runs[0][2],
            "n_blocks": np.array(info["n_blocks"], np.int32),
            "poses2": runs[1][0], "stats2": runs[1][1], "chi2": runs[1][2]}


def run_case_in_own_process(name, out):
    """run_case in a fresh process with the case's environment; returns its arrays."""
    subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name, "--out", out], check=True,
                   env=dict(os.environ, **CASES[name]["env"]), timeout=120)
    with np.load(out) as z:
        return {k.split("/", 1)[1]: z[k] for k in z.files}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "round_tail", "parent.npz"))
    args = ap.parse_args()
    import picp_amd
    if args.case:
        got = run_case(picp_amd, args.case)
        np.savez(args.out, **{args.case + "/" + k: v for k, v in got.items()})
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    arrays = {}
    for name, c in CASES.items():
        if c["own_process"]:
            tmp = args.out + "." + name + ".tmp.npz"
            got = run_case_in_own_process(name, tmp)
            os.remove(tmp)
        else:
            got = run_case(picp_amd, name)
        for k in ("poses", "stats", "chi"):
            assert np.array_equal(got[k], got[k + "2"]), (name, k)
            arrays[name + "/" + k] = got[k]
        arrays[name + "/n_blocks"] = got["n_blocks"]
        print(name, "blocks", int(got["n_blocks"]), "rounds", got["stats"][:, 2].tolist(), flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
