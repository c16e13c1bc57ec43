#!/usr/bin/env python3
"""The cases of tests/test_gpu_vo_plan.py, how one is run, and the golden file of a build.

    PICP_LIB=<library of the build to record> python tools/vo_plan_golden.py

writes tests/golden/vo_plan/parent.npz (keys <case>/<array> and num_cu); the test compares every
later build with it bit for bit.  The file in the repository was written with the build before the
VO segment layout became a plan (csrc/picp_vo_plan.cpp).  The test loads this file for CASES,
SCHEDULES and run_case; nothing here depends on the tests.  Writing the golden file needs a GPU.

Every case runs under three schedules (the default one, the serial order, the world match split
by map age) with the track log and the guard pads on.  Every schedule gives the same bits, so the
file holds the default schedule's arrays once per case; writing it asserts that the two other
schedules of the recorded build agree with them."""
import argparse
import ctypes
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "02-visualodometry_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

THR = 3000.0
SEED = 23
NOISE = 0.5  # the round counts stay a property of the data (tests/vo_shapes.py)
ENV_KEYS = ("PICP_VO_FUSE", "PICP_VO_OVERLAP", "PICP_VO_CHAINS", "PICP_VO_SPLIT", "PICP_VO_GRAPH", "PICP_VO_GUARD",
            "PICP_VO_PHASE", "PICP_VO_MATCH_FULL", "PICP_VO_PRIO", "PICP_MATCH_KSPLIT")
SCHEDULES = {
    "default": {},
    "serial": {"PICP_VO_OVERLAP": "0", "PICP_VO_CHAINS": "1"},
    "split": {"PICP_VO_SPLIT": "1"},
}

# name -> (frames, observations per frame, first, steps, frames emptied)
# seg3: segments 1 and 2 overlap (frames 7, 8) inside one chain's group, so both chains run
CASES = {
    "seg3": (12, 300, [0, 5, 7], [4, 3, 4], []),
    "seg3_empty": (12, 300, [0, 5, 7], [4, 3, 4], [2]),
    # the largest frame has a little over 1,024 observations: npt 2, and steps with more than
    # 2 * 512 correspondences take the block kernel's streamed remainder
    "npt2": (7, 1250, [0, 3], [3, 3], []),
    "one_seg": (6, 300, [0], [5], []),
}
STEP_KEYS = ("n_corr", "n_in", "rounds", "n_new", "chi_in", "chi_out", "converged", "n_projected")
STAT_KEYS = ("chi_in", "chi_out", "n_in", "ok", "rounds", "converged", "n_projected")


@functools.lru_cache(maxsize=None)
def num_cu():
    """Compute units of device 0, asked of the HIP runtime the library is linked against."""
    import picp_amd
    n = ctypes.c_int(0)
    attr = 63  # hipDeviceAttributeMultiprocessorCount (hip/hip_runtime_api.h)
    rc = picp_amd.lib().hipDeviceGetAttribute(ctypes.byref(n), ctypes.c_int(attr), ctypes.c_int(0))
    assert rc == 0 and 1 <= n.value <= 4096, (rc, n.value)
    return n.value


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(K, frame_off, uv, desc, first, steps, boot) of a case."""
    from picp_amd.vo_synth import VOSequence
    n, obs, first, steps, empty = CASES[name]
    s = VOSequence(n, obs_per_frame=obs, seed=SEED, pixel_noise=NOISE)
    fs = [s.frame(k) for k in range(n)]
    keep = [0 if k in empty else len(f["uv"]) for k, f in enumerate(fs)]
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(keep)
    T_cw = np.stack([s.T_cw(k) for k in range(n)]).astype(np.float32)
    first, steps = np.asarray(first, np.int64), np.asarray(steps, np.int32)
    return {"K": s.K, "frame_off": off,
            "uv": np.ascontiguousarray(np.concatenate([f["uv"][:z] for f, z in zip(fs, keep)]), np.float32),
            "desc": np.ascontiguousarray(np.concatenate([f["desc"][:z] for f, z in zip(fs, keep)]), np.float32),
            "first": first, "steps": steps, "boot": np.stack([[T_cw[f], T_cw[f + 1]] for f in first])}


def _stats(st):
    return np.stack([np.asarray(st[k]).astype(np.float32 if k.startswith("chi") else np.int32).view(np.int32)
                     for k in STAT_KEYS], 1) if len(st["n_in"]) else np.zeros((0, len(STAT_KEYS)), np.int32)


def run_case(native, name, schedule):
    """One run of the case under the schedule, the track log and the guard pads on.  Returns a dict
    of arrays: info (n_obs, n_slots, map_slots, npt), poses, steps (STEP_KEYS order, the floats'
    bits), guard (bad bytes, first bad pad), and per segment k map_xyz/k, map_desc/k, track_off/k,
    obs_slot/k, obs_index/k, ref_xyz/k, ref_stats/k (STAT_KEYS order, the floats' bits), adj_xyz/k,
    adj_stats/k; poses_wc and adj_poses_wc."""
    C = build(name)
    env = dict(SCHEDULES[schedule], PICP_VO_GUARD="1")
    old = {k: os.environ.get(k) for k in ENV_KEYS}
    for k in ENV_KEYS:
        os.environ.pop(k, None)
    os.environ.update(env)  # read when the sequence is created
    try:
        seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    seq.track_log(True)
    seq.run()
    n = len(C["first"])
    info = seq.info()
    out = {"info": np.array([info[k] for k in ("n_obs", "n_slots", "map_slots", "npt")], np.int64),
           "poses": np.concatenate(seq.poses())}
    rec = seq.step_records()
    out["steps"] = np.concatenate([np.stack([r[k].astype(np.float32 if k.startswith("chi") else np.int32)
                                             .view(np.int32) for k in STEP_KEYS], 1) for r in rec])
    for k in range(n):
        out["map_xyz/%d" % k], out["map_desc/%d" % k] = seq.map(k)
        out["track_off/%d" % k], out["obs_slot/%d" % k], out["obs_index/%d" % k] = seq.tracks(k)
    out["poses_wc"] = np.concatenate(seq.poses_wc())
    seq.refine_map()
    for k in range(n):
        xyz, st = seq.refined_map(k)
        out["ref_xyz/%d" % k], out["ref_stats/%d" % k] = xyz, _stats(st)
    seq.adjust()
    out["adj_poses_wc"] = np.concatenate(seq.adjusted_poses_wc())
    for k in range(n):
        xyz, st = seq.adjusted_map(k)
        out["adj_xyz/%d" % k], out["adj_stats/%d" % k] = xyz, _stats(st)
    bad, buf = ctypes.c_int64(-1), ctypes.c_int(-2)
    assert native.lib().picp_vo_debug_guard(seq._h, ctypes.byref(bad), ctypes.byref(buf)) == 0
    out["guard"] = np.array([bad.value, buf.value], np.int64)
    seq.close()
    return out


def assert_same(got, want, what, skip=()):
    """Every array of want equals got's, bit for bit (floats by their bits: NaN equals NaN)."""
    for k, w in want.items():
        if k.startswith(tuple(skip)):
            continue
        g = np.asarray(got[k])
        w = np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        assert g.tobytes() == w.tobytes(), (what, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vo_plan", "parent.npz"))
    args = ap.parse_args()
    import picp_amd
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    arrays = {"num_cu": np.array(num_cu(), np.int32)}
    for name in CASES:
        got = run_case(picp_amd, name, "default")
        for sched in SCHEDULES:
            if sched != "default":
                assert_same(run_case(picp_amd, name, sched), got, "%s %s" % (name, sched))
        assert got["guard"].tolist() == [0, -1], (name, got["guard"])
        for k, v in got.items():
            arrays[name + "/" + k] = v
        print(name, "info", got["info"].tolist(), "n_corr", got["steps"][:, 0].tolist(), "rounds",
              got["steps"][:, 2].tolist(), "map", [len(got["map_xyz/%d" % k]) for k in range(len(CASES[name][2]))],
              flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
