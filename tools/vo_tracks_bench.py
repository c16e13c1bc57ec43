#!/usr/bin/env python3
"""Measurements of the VO sequence's track log and map refinement.  Every mode
prints JSON lines and appends them to a file under --out (default profiles/r11/vo_tracks/).

  vo_tracks_bench.py time  --shape 8e|250x40 --state off|on   picp_vo_time samples of one state (--pkg: the
                                                 package directory to import picp_amd from)
  vo_tracks_bench.py ab    --parent-tree PATH    a built checkout of the parent commit and this tree
                                                 alternating (a child process per state: parent, off,
                                                 on), both shapes, two rounds (the order rotates), 5 samples of 2 runs each
  vo_tracks_bench.py build [--shape ...]         picp_vo_refine_time's build_us and refine_us, beside
                                                 picp_refine_time of a standalone refiner on the same tracks
  vo_tracks_bench.py map   [--frames 2501]       map error before and after picp_vo_refine_map on a
                                                 synthetic sequence (pixel noise 0.5), 40- and 1,250-step segments
  vo_tracks_bench.py bench --parent-tree PATH    the default bench line, parent and this alternating, 3 runs each

Shapes (bench.py's C5 sequence: 10,000 frames x 2,000 observations, seed 42, each segment in its
first camera's frame): 8e = 8 segments x 1,250 steps, 250x40 = 250 segments x 40 steps.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "02-visualodometry_amd")
THRESHOLD = 3000.0
SHAPES = {"8e": 1250, "250x40": 40}


def emit(out_dir, name, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name), "a") as f:
        f.write(line + "\n")


def sequence(frames, obs, seg_len, noise=0.0, seed=42):
    """bench.py's C5 setup: -> (synthetic sequence, packed frames, first, steps, boot, rel) with
    every segment in its first camera's frame (rel[k]: synthetic world -> segment k's world)."""
    from picp_amd.vo_synth import VOSequence, segments
    seq = VOSequence(frames, obs_per_frame=obs, seed=seed, pixel_noise=noise)
    D = seq.frames(0, frames)
    first, steps = segments(frames, seg_len)
    rel = [np.linalg.inv(D["T_cw"][f].astype(np.float64)) for f in first]
    boot = np.stack([[np.eye(4), rel[k] @ D["T_cw"][f + 1]] for k, f in enumerate(first)]).astype(np.float32)
    return seq, D, first, steps, boot, rel


def open_vo(picp_amd, seq, D, first, steps, boot, log):
    vo = picp_amd.VOSequence(D["frame_off"], D["uv"], D["desc"], K=seq.K)
    vo.set_segments(first, steps, boot, threshold=THRESHOLD)
    if log:
        vo.track_log(True)
    return vo


def mode_time(a, picp_amd):
    seq, D, first, steps, boot, _ = sequence(a.frames, a.obs, SHAPES[a.shape])
    vo = open_vo(picp_amd, seq, D, first, steps, boot, a.state == "on")  # (the parent has no log: off only)
    for _ in range(2):
        vo.run()
    ms = [vo.time(a.reps) for _ in range(a.samples)]
    vo.close()
    emit(a.out, "vo_time.jsonl", {"vo_time": a.shape, "state": a.label or a.state,
                                  "segments": len(first), "steps": int(steps.max()), "reps": a.reps,
                                  "ms": [round(m, 4) for m in ms]})


def mode_ab(a):
    """parent, off, on in turn, each in a process of its own (the package loads one library)."""
    res = {}
    for shape in a.shapes:
        for rnd in range(a.rounds):
            parent_pkg = os.path.join(os.path.abspath(a.parent_tree), os.path.basename(PKG))
            states = [("parent", parent_pkg, "off"), ("off", PKG, "off"), ("on", PKG, "on")]
            # the order rotates from round to round, so a drift over the session does not fall on one state
            for label, pkg, state in states[rnd % 3:] + states[:rnd % 3]:
                env = dict(os.environ)
                env.pop("PICP_LIB", None)
                cmd = [sys.executable, os.path.abspath(__file__), "time", "--shape", shape, "--state", state, "--label",
                       label, "--samples", str(a.samples), "--reps", str(a.reps), "--frames", str(a.frames), "--obs",
                       str(a.obs), "--out", a.out, "--pkg", pkg]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("vo_tracks_bench: %s %s failed (%d)" % (shape, label, p.returncode))
                sys.stdout.write(p.stdout)
                sys.stdout.flush()
                res.setdefault((shape, label), []).extend(json.loads(p.stdout.strip().splitlines()[-1])["ms"])
    for shape in a.shapes:
        par, off, on = (res[(shape, k)] for k in ("parent", "off", "on"))
        steps = SHAPES[shape]
        emit(a.out, "vo_time_summary.jsonl", {
            "vo_time_summary": shape, "parent_ms": [min(par), max(par)], "off_ms": [min(off), max(off)],
            "on_ms": [min(on), max(on)], "off_inside_parent_spread": bool(min(par) <= min(off) and max(off) <= max(par)),
            "on_minus_off_us_per_step": [round(1e3 * (min(on) - max(off)) / steps, 2),
                                         round(1e3 * (max(on) - min(off)) / steps, 2)]})


def mode_build(a, picp_amd):
    for shape in a.shapes:
        seq, D, first, steps, boot, _ = sequence(a.frames, a.obs, SHAPES[shape])
        vo = open_vo(picp_amd, seq, D, first, steps, boot, True)
        vo.run()
        vo.refine_time(2)  # warm-up
        t = [vo.refine_time(a.reps) for _ in range(3)]
        tr = [vo.tracks(k) for k in range(len(first))]
        slot0 = np.concatenate([[0], np.cumsum(steps.astype(np.int64) + 1)])
        lens = np.concatenate([np.diff(o) for o, _, _ in tr])
        off = np.concatenate([[0], np.cumsum(lens)])
        r = picp_amd.PointRefiner(K=seq.K)
        r.set_poses(np.concatenate(vo.poses_wc()))
        r.set_tracks(off, np.concatenate([slot0[k] + s for k, (_, s, _) in enumerate(tr)]).astype(np.int32),
                     D["uv"][np.concatenate([i for _, _, i in tr])])
        start = np.concatenate([vo.map(k)[0] for k in range(len(first))])

        def alone_us(reps):
            # picp_refine_time leaves the refined points behind: every sample starts from the run's
            # map again, as picp_vo_refine_time's repetitions do
            r.set_points(start)
            return r.time(reps)

        alone_us(2)
        alone = min(alone_us(a.reps) for _ in range(3))
        r.close()
        vo.close()
        emit(a.out, "build_refine.jsonl", {
            "build_refine": shape, "segments": len(first), "n_points": int(len(lens)), "n_obs": int(off[-1]),
            "mean_len": round(float(lens.mean()), 2), "max_len": int(lens.max()), "reps": a.reps,
            "build_us": round(min(b for b, _ in t), 1), "refine_us": round(min(r_ for _, r_ in t), 1),
            "standalone_refine_us": round(alone, 1)})


def truth_of(seq, ids, rel):
    """The true positions of the landmarks `ids` (vo_synth's numbering) in a segment's world."""
    n = seq.per_step
    k = ids // n + seq._k0
    out = np.zeros((len(ids), 3))
    for kk in np.unique(k):
        sel = k == kk
        out[sel] = seq.landmarks(int(kk))[1][ids[sel] % n]
    return out @ rel[:3, :3].T + rel[:3, 3]


def mode_map(a, picp_amd):
    for seg_len in a.seg_lens:
        seq, D, first, steps, boot, rel = sequence(a.frames, a.obs, seg_len, noise=0.5)
        vo = open_vo(picp_amd, seq, D, first, steps, boot, True)
        vo.run()
        vo.refine_map()
        before, after, lens, okf, pose_err = [], [], [], [], []
        for k in range(len(first)):
            off, slot, idx = vo.tracks(k)
            x = idx[off[:-1]]  # the track's first entry is the observation x that created the point
            same = np.ones(len(x), bool)
            truth = truth_of(seq, D["id_real"][x], rel[k])
            m0 = vo.map(k)[0].astype(np.float64)
            m1, st = vo.refined_map(k)
            before.append(np.linalg.norm(m0 - truth, axis=1)[same])
            after.append(np.linalg.norm(m1.astype(np.float64) - truth, axis=1)[same])
            lens.append(np.diff(off)[same])
            okf.append(st["ok"][same] == 1)
            P = vo.poses()[k]
            gt = rel[k] @ D["T_cw"][int(first[k]) + int(steps[k])].astype(np.float64)
            pose_err.append(float(np.linalg.norm(P[-1][:3, 3] - gt[:3, 3])))
        b, c, n, ok = (np.concatenate(v) for v in (before, after, lens, okf))
        fin = np.isfinite(b) & np.isfinite(c)
        rec = {"map_error": seg_len, "frames": a.frames, "segments": len(first), "pixel_noise": 0.5,
               "points": int(len(b)), "finite": int(fin.sum()), "refine_ok": int(ok.sum()),
               "end_pose_error_m_median": round(float(np.median(pose_err)), 4),
               "end_pose_error_m_max": round(float(np.max(pose_err)), 4)}
        for name, sel in (("all", fin), ("len_ge_3", fin & (n >= 3)), ("len_ge_6", fin & (n >= 6))):
            rec[name] = {"points": int(sel.sum()),
                         "before_m": [round(float(np.percentile(b[sel], q)), 5) for q in (50, 95)] if sel.any() else None,
                         "after_m": [round(float(np.percentile(c[sel], q)), 5) for q in (50, 95)] if sel.any() else None}
        vo.close()
        emit(a.out, "map_error.jsonl", rec)


def mode_bench(a):
    trees = [("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)]
    for rnd in range(a.rounds):
        for label, tree in trees[rnd % 2:] + trees[:rnd % 2]:  # who goes first alternates
            env = dict(os.environ)
            env.pop("PICP_LIB", None)
            p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                               env=env, capture_output=True, text=True, timeout=600, cwd=tree)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("vo_tracks_bench: bench.py failed (%d)" % p.returncode)
            line = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            emit(a.out, "default_line.jsonl", {"default_line": label, "run": rnd, "value": line.get("value"),
                                               "unit": line.get("unit"), "metric": line.get("metric")})


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "ab", "build", "map", "bench"])
    ap.add_argument("--shape", default="8e", choices=sorted(SHAPES))
    ap.add_argument("--shapes", nargs="*", default=["8e", "250x40"], choices=sorted(SHAPES))
    ap.add_argument("--state", default="off", choices=["off", "on"])
    ap.add_argument("--label", default=None)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--pkg", default=PKG, help="time: the directory to import picp_amd from")
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=None, help="runs per sample (time: 2) / repetitions (build: 10)")
    ap.add_argument("--rounds", type=int, default=None, help="ab: 2, bench: 3")
    ap.add_argument("--frames", type=int, default=None, help="sequence length (10000; map: 2501)")
    ap.add_argument("--obs", type=int, default=2000)
    ap.add_argument("--seg-lens", nargs="*", type=int, default=[40, 1250])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "vo_tracks"))
    a = ap.parse_args()
    if a.frames is None:
        a.frames = 2501 if a.mode == "map" else 10000
    if a.rounds is None:
        a.rounds = 3 if a.mode == "bench" else 2
    if a.reps is None:
        a.reps = 10 if a.mode == "build" else 2
    if a.mode in ("ab", "bench"):
        if not a.parent_tree or not os.path.exists(os.path.join(a.parent_tree, "bench.py")):
            ap.error("--parent-tree: a built checkout of the parent commit is needed")
        return mode_ab(a) if a.mode == "ab" else mode_bench(a)
    sys.path.insert(0, a.pkg if a.mode == "time" else PKG)
    import picp_amd
    {"time": mode_time, "build": mode_build, "map": mode_map}[a.mode](a, picp_amd)


if __name__ == "__main__":
    main()
