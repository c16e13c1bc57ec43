#!/usr/bin/env python3
"""The cases of tests/test_gpu_layout.py, how one is run, and the golden file of a build.

    PICP_LIB=<library of the build to record> python tools/layout_golden.py

writes tests/golden/layout/parent.npz (keys <case>/poses, /stats, /chi, /layout, and num_cu); the
test compares every later build with it bit for bit.  The file in the repository was written with
the build before the batch layout became a plan (csrc/picp_layout.cpp).  The test loads this file
for CASES and run_case; nothing here depends on the tests.  Writing the golden file needs a GPU.

The cases are the layouts tools/round_tail_golden.py does not reach: graph mode with one item per
lane, with float4 lanes and a ragged last block, with ragged tables and an empty problem, and
with the streaming-share block table; the persistent and block candidates laid out without
hand-offs (PICP_RESIDENT_BLOCKS_PER_CU=0); and a batch created after a smaller one of the same
process was solved and destroyed."""
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
ROUNDS = 5
STAT_INT = ("n_in", "ok", "rounds", "converged", "n_projected")
LAYOUT = ("mode", "n_blocks", "handoff_grid", "resident_blocks", "fallbacks")
MODES = ("graph", "persistent", "block")


def _case(name, sizes, seed, mode=None, env=None, expect_mode=None, before=None, cu_dependent=False):
    """sizes: a list, or a function of the CU count.  mode: PICP_MODE, None leaves the choice to the
    library.  before: sizes of a batch solved and destroyed first."""
    env = dict(env or {})
    if mode:
        env["PICP_MODE"] = mode
    return dict(name=name, sizes=sizes, seed=seed, env=env, expect_mode=expect_mode or mode, before=before,
                cu_dependent=cu_dependent)


def _cases():
    ipb = {"PICP_ITEMS_PER_BLOCK": "1024"}
    no_handoff = {"PICP_RESIDENT_BLOCKS_PER_CU": "0"}
    return [
        _case("graph_vec1", [4096], 5000, mode="graph"),
        _case("graph_vec4_ragged", [5000], 5100, mode="graph", env=ipb),
        _case("graph_tables_empty", [3000, 17, 0, 5000], 5200, mode="graph"),
        # 2 x CUs blocks of float4 lanes on one frame: the streaming-share block table
        _case("graph_stream_share", lambda cus: [2 * cus * 1024], 5300, mode="graph", env=ipb, cu_dependent=True),
        _case("persistent_no_handoff", [300], 5400, env=no_handoff, expect_mode="graph"),
        _case("block_no_handoff", [20000] * 6, 5500, env=no_handoff, expect_mode="block"),
        _case("relayout_larger", [3000, 5000, 4000], 5600, before=[1000, 2000], expect_mode="block"),
    ]


CASES = {c["name"]: c for c in _cases()}


@functools.lru_cache(maxsize=None)
def num_cu():
    """Compute units of device 0, asked of the HIP runtime the library is linked against."""
    import ctypes

    import picp_amd
    n = ctypes.c_int(0)
    attr = 63  # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)
    rc = picp_amd.lib().hipDeviceGetAttribute(ctypes.byref(n), ctypes.c_int(attr), ctypes.c_int(0))
    assert rc == 0 and 1 <= n.value <= 4096, (rc, n.value)
    return n.value


def sizes_of(name):
    s = CASES[name]["sizes"]
    return list(s(num_cu())) if callable(s) else list(s)


@functools.lru_cache(maxsize=None)
def _problems(seed, sizes):
    from picp_amd import synth
    out = []
    for i, n in enumerate(sizes):  # an empty problem: one made, none of it kept
        p = synth.make_problem(max(n, 1), seed=seed + i, outlier_frac=0.1, pixel_noise=0.5, shuffle=False)
        out.append({k: (p[k][:n] if k in ("xyz", "uv", "x", "y", "z", "u", "v") else p[k]) for k in p})
    return out


def problems(name):
    return _problems(CASES[name]["seed"], tuple(sizes_of(name)))


def _solve_twice(native, sizes, probs, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)  # read when the batch is created
    try:
        b = native.Batch(sizes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    info = b.info()
    b.set_data(np.concatenate([p["xyz"] for p in probs]), np.concatenate([p["uv"] for p in probs]))
    runs = []
    for _ in range(2):
        b.set_poses(np.stack([p["T_init"] for p in probs]))
        b.solve(threshold=THR, max_rounds=ROUNDS, conv_eps=-1.0)
        st = b.stats()
        runs.append((b.poses(), np.array([[s[k] for k in STAT_INT] for s in st], np.int32),
                     np.array([[s["chi_in"], s["chi_out"]] for s in st], np.float32)))
    res = b.residency()  # after the solves: a fallback would show
    b.close()
    layout = np.array([MODES.index(info["mode"]), info["n_blocks"], res["handoff_grid"], res["resident_blocks"],
                       res["fallbacks"]], np.int32)
    return {"poses": runs[0][0], "stats": runs[0][1], "chi": runs[0][2], "layout": layout,
            "poses2": runs[1][0], "stats2": runs[1][1], "chi2": runs[1][2]}


def run_case(native, name):
    """Solve the case twice on one batch.  Returns poses (P, 4, 4), the integer statistics (P, 5,
    STAT_INT order), chi (P, 2: chi_in, chi_out), the layout (LAYOUT order), and the second solve's
    arrays."""
    c = CASES[name]
    if c["before"]:
        before = tuple(c["before"])
        _solve_twice(native, list(before), _problems(c["seed"] + 50, before), c["env"])
    return _solve_twice(native, sizes_of(name), problems(name), c["env"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "layout", "parent.npz"))
    args = ap.parse_args()
    import picp_amd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    arrays = {"num_cu": np.array(num_cu(), np.int32)}
    for name in CASES:
        got = run_case(picp_amd, name)
        for k in ("poses", "stats", "chi"):
            assert np.array_equal(got[k], got[k + "2"]), (name, k)
            arrays[name + "/" + k] = got[k]
        arrays[name + "/layout"] = got["layout"]
        print(name, dict(zip(LAYOUT, got["layout"].tolist())), "rounds", got["stats"][:, 2].tolist(), flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
