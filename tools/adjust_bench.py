#!/usr/bin/env python3
"""Measurements of the alternating pose / point adjustment.  Every mode prints
JSON lines and appends them to a file under --out (default profiles/r12/adjust/).

  adjust_bench.py maps  [--shapes data 10k 180k]   picp_refine_adjust_time on the maps of tools/refine_bench.py
                                                   (pose 0 fixed, 3 sweeps of 10 + 10 rounds)
  adjust_bench.py vo    [--shapes 8e 250x40]       the same on a standalone refiner given the tracks, poses
                                                   and maps of a VO run (tools/vo_tracks_bench.py's shapes)
  adjust_bench.py map   [--frames 2501]            map error of the run's map, of picp_vo_refine_map and of
                                                   picp_vo_adjust on a synthetic sequence (pixel noise 0.5)
  adjust_bench.py bench --parent-tree PATH         the default bench line, parent and this alternating, 3 runs each

Times are the minimum of three samples of --reps repetitions: the view build once per track set, the
gather + write-back kernels, the pose batch's solve and the point step per sweep.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "02-visualodometry_amd")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_bench as RB  # noqa: E402
import vo_tracks_bench as VB  # noqa: E402

POINTS = dict(RB.PARAMS)
POSES = dict(threshold=3000.0, damping=1.0, min_inliers=0, keep_outliers=0, max_rounds=10, conv_eps=-1.0)
SWEEPS = 3


def timed(r, reps, label, extra, out):
    """adjust_time of a loaded refiner -> one JSON line."""
    kw = dict(sweeps=SWEEPS, points=POINTS, poses=POSES)
    r.adjust_time(1, **kw)  # warm-up: the view, the batch and its layout exist afterwards
    t = np.array([r.adjust_time(reps, **kw) for _ in range(3)]).min(0)
    off, _, _ = r.pose_view()
    lens = np.diff(off)
    rec = dict(extra)
    rec.update({"n_poses": int(len(lens)), "list_mean": round(float(lens.mean()), 1), "list_max": int(lens.max()),
                "sweeps": SWEEPS, "reps": reps, "build_us": round(float(t[0]), 1),
                "gather_us_per_sweep": round(float(t[1]), 1), "pose_us_per_sweep": round(float(t[2]), 1),
                "point_us_per_sweep": round(float(t[3]), 1), "sweep_records": r.sweeps()})
    VB.emit(out, label, rec)


def mode_maps(a, picp_amd):
    for name in a.shapes:
        case = RB.make_shape(name)
        r = picp_amd.PointRefiner(rows=case["rows"], cols=case["cols"], K=case["K"])
        r.set_poses(case["poses"])
        r.set_tracks(case["off"], case["obs_pose"], case["obs_uv"])
        r.set_points(case["start"])
        fixed = np.zeros(len(case["poses"]), bool)
        fixed[0] = True
        r.set_fixed_poses(fixed)
        timed(r, a.reps, "adjust_time.jsonl", {"adjust_time": name, "n_points": int(len(case["off"]) - 1),
                                               "n_obs": int(case["off"][-1])}, a.out)
        r.close()


def mode_vo(a, picp_amd):
    for shape in a.shapes:
        seq, D, first, steps, boot, _ = VB.sequence(a.frames, a.obs, VB.SHAPES[shape])
        vo = VB.open_vo(picp_amd, seq, D, first, steps, boot, True)
        vo.run()
        tr = [vo.tracks(k) for k in range(len(first))]
        slot0 = np.concatenate([[0], np.cumsum(steps.astype(np.int64) + 1)])
        lens = np.concatenate([np.diff(o) for o, _, _ in tr])
        off = np.concatenate([[0], np.cumsum(lens)])
        r = picp_amd.PointRefiner(K=seq.K)
        r.set_poses(np.concatenate(vo.poses_wc()))
        r.set_tracks(off, np.concatenate([slot0[k] + s for k, (_, s, _) in enumerate(tr)]).astype(np.int32),
                     D["uv"][np.concatenate([i for _, _, i in tr])])
        r.set_points(np.concatenate([vo.map(k)[0] for k in range(len(first))]))
        fixed = np.zeros(int(slot0[-1]), bool)
        fixed[slot0[:-1]] = True
        r.set_fixed_poses(fixed)
        vo.close()
        timed(r, a.reps, "adjust_time.jsonl", {"adjust_time": "vo_" + shape, "segments": len(first),
                                               "n_points": int(len(lens)), "n_obs": int(off[-1])}, a.out)
        r.close()


def mode_map(a, picp_amd):
    for seg_len in a.seg_lens:
        seq, D, first, steps, boot, rel = VB.sequence(a.frames, a.obs, seg_len, noise=0.5)
        vo = VB.open_vo(picp_amd, seq, D, first, steps, boot, True)
        vo.run()
        vo.refine_map()
        vo.adjust(sweeps=a.sweeps, points=POINTS, poses=POSES)
        cols = {"run": [], "refined": [], "adjusted": []}
        lens, end = [], {"run": [], "adjusted": []}
        adj_wc = vo.adjusted_poses_wc()
        for k in range(len(first)):
            off, slot, idx = vo.tracks(k)
            truth = VB.truth_of(seq, D["id_real"][idx[off[:-1]]], rel[k])
            for name, m in (("run", vo.map(k)[0]), ("refined", vo.refined_map(k)[0]), ("adjusted", vo.adjusted_map(k)[0])):
                cols[name].append(np.linalg.norm(m.astype(np.float64) - truth, axis=1))
            lens.append(np.diff(off))
            gt = rel[k] @ D["T_cw"][int(first[k]) + int(steps[k])].astype(np.float64)
            end["run"].append(float(np.linalg.norm(vo.poses()[k][-1][:3, 3] - gt[:3, 3])))
            end["adjusted"].append(float(np.linalg.norm(np.linalg.inv(adj_wc[k][-1].astype(np.float64))[:3, 3] - gt[:3, 3])))
        vo.close()
        n = np.concatenate(lens)
        cols = {k: np.concatenate(v) for k, v in cols.items()}
        fin = np.all([np.isfinite(v) for v in cols.values()], axis=0)
        rec = {"map_error": seg_len, "frames": a.frames, "segments": len(first), "pixel_noise": 0.5, "sweeps": a.sweeps,
               "points": int(len(n)), "finite": int(fin.sum()),
               "end_pose_error_m_median": {k: round(float(np.median(v)), 4) for k, v in end.items()},
               "end_pose_error_m_max": {k: round(float(np.max(v)), 4) for k, v in end.items()}}
        for name, sel in (("all", fin), ("len_ge_3", fin & (n >= 3)), ("len_ge_6", fin & (n >= 6))):
            rec[name] = {"points": int(sel.sum())}
            for k, v in cols.items():
                rec[name][k + "_m"] = [round(float(np.percentile(v[sel], q)), 5) for q in (50, 95)] if sel.any() else None
        VB.emit(a.out, "map_error.jsonl", rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["maps", "vo", "map", "bench"])
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweeps", type=int, default=SWEEPS, help="map: sweeps of picp_vo_adjust")
    ap.add_argument("--rounds", type=int, default=3, help="bench: runs of each tree")
    ap.add_argument("--parent-tree", default=None, help="bench: a built checkout of the parent commit")
    ap.add_argument("--frames", type=int, default=None, help="sequence length (vo: 10000; map: 2501)")
    ap.add_argument("--obs", type=int, default=2000)
    ap.add_argument("--seg-lens", nargs="*", type=int, default=[40, 1250])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "adjust"))
    a = ap.parse_args()
    if a.frames is None:
        a.frames = 2501 if a.mode == "map" else 10000
    if a.shapes is None:
        a.shapes = ["data", "10k", "180k"] if a.mode == "maps" else ["8e", "250x40"]
    if a.mode == "bench":
        if not a.parent_tree or not os.path.exists(os.path.join(a.parent_tree, "bench.py")):
            ap.error("--parent-tree: a built checkout of the parent commit is needed")
        return VB.mode_bench(a)
    sys.path.insert(0, PKG)
    import picp_amd
    {"maps": mode_maps, "vo": mode_vo, "map": mode_map}[a.mode](a, picp_amd)


if __name__ == "__main__":
    main()
