#!/usr/bin/env python3
"""The cases of tests/test_gpu_pers_waits.py, how one is run, and the golden file of a build.

    PICP_LIB=<library of the build to record> python tools/pers_waits_golden.py

writes tests/golden/pers_waits/parent.npz (keys <case>/poses, /stats, /chi, /n_blocks); the test
compares every later build with it bit for bit.  The cases are the smallest persistent-mode frames
at which a follower's pose wait takes another path (one follower; a solver with two followers; a
follower block that holds one item; two items per lane, the staggered sweep), and the 100k frame
of the headline workload, which the test also solves beside device-to-device copies on a second
stream (busy_copies).  The test loads this file for CASES, run_case and busy_copies; nothing here
depends on the tests.  Writing the golden file needs a GPU."""
import argparse
import contextlib
import ctypes
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


def _cases():
    out = {}
    # a frame of more than 512 x CUs correspondences is partitioned by the CU count (picp_layout.cpp)
    for tag, n, rounds in (("follower1", 9 * 512 - 5, 50), ("followers2", 17 * 512, 50),
                           ("follower_1item", 17 * 512 + 1, 50), ("npt2", 140000, 5), ("c2_100k", 100000, 50)):
        for keep in (0, 1):
            if tag == "c2_100k" and keep:
                continue
            name = "%s_keep%d" % (tag, keep)
            out[name] = dict(name=name, n=n, rounds=rounds, keep=keep, seed=5000 + n % 997,
                             of=0.0 if tag == "c2_100k" else 0.1, cu_dependent=n > 33 * 512)
    return out


CASES = _cases()


@functools.lru_cache(maxsize=None)
def problem(name):
    from picp_amd import synth
    c = CASES[name]
    return synth.make_problem(c["n"], seed=c["seed"], outlier_frac=c["of"], pixel_noise=0.5, shuffle=False)


def run_case(native, name, solves=2):
    """Solve the case `solves` times on one persistent-mode batch.  Returns the block count and,
    per solve, poses (1, 4, 4), the integer statistics (1, 5, STAT_INT order) and chi (1, 2)."""
    c = CASES[name]
    p = problem(name)
    old = os.environ.get("PICP_MODE")
    os.environ["PICP_MODE"] = "persistent"  # read when the batch is created
    try:
        b = native.Batch([c["n"]])
    finally:
        if old is None:
            os.environ.pop("PICP_MODE", None)
        else:
            os.environ["PICP_MODE"] = old
    info = b.info()
    assert info["mode"] == "persistent", info
    b.set_data(p["xyz"], p["uv"])
    runs = []
    for _ in range(solves):
        b.set_poses(p["T_init"][None])
        b.solve(threshold=THR, max_rounds=c["rounds"], conv_eps=-1.0, keep_outliers=c["keep"])
        st = b.stats()
        runs.append({"poses": b.poses(), "stats": np.array([[s[k] for k in STAT_INT] for s in st], np.int32),
                     "chi": np.array([[s["chi_in"], s["chi_out"]] for s in st], np.float32)})
    # a timed-out hand-off makes the batch re-run the solve in graph mode, which sums in another
    # order: the arrays compared here must come from the persistent kernel
    fallbacks = b.residency()["fallbacks"]
    b.close()
    assert fallbacks == 0, "%s: %d solves fell back to graph mode (a hand-off timed out)" % (name, fallbacks)
    return np.array(info["n_blocks"], np.int32), runs


def _hip():
    """The HIP runtime that the native library has loaded."""
    with open("/proc/self/maps") as f:
        paths = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    assert paths, "the HIP runtime is not loaded"
    return ctypes.CDLL(paths[0])


@contextlib.contextmanager
def busy_copies(nbytes=256 << 20, copies=48):
    """Device-to-device copies of nbytes each, queued on a stream of their own, run while the
    body does; the stream is drained and everything freed on the way out."""
    hip = _hip()
    src, dst, stream = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(src), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipMalloc(ctypes.byref(dst), ctypes.c_size_t(nbytes)) == 0
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), ctypes.c_uint(1)) == 0  # non-blocking
    try:
        assert hip.hipMemsetAsync(src, 1, ctypes.c_size_t(nbytes), stream) == 0
        for _ in range(copies):
            assert hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), ctypes.c_int(3), stream) == 0  # D2D
        yield
        assert hip.hipStreamQuery(stream) in (0, 600), "the copy stream failed"  # success / not ready
    finally:
        hip.hipStreamSynchronize(stream)
        hip.hipStreamDestroy(stream)
        hip.hipFree(src)
        hip.hipFree(dst)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pers_waits", "parent.npz"))
    args = ap.parse_args()
    import picp_amd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    arrays = {}
    for name in CASES:
        nb, runs = run_case(picp_amd, name)
        for k in ("poses", "stats", "chi"):
            assert np.array_equal(runs[0][k], runs[1][k]), (name, k)
            arrays[name + "/" + k] = runs[0][k]
        arrays[name + "/n_blocks"] = nb
        print(name, "blocks", int(nb), "rounds", runs[0]["stats"][:, 2].tolist(), flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
