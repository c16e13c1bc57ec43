#!/usr/bin/env python3
"""Per-stage device times of the Sim(3) RANSAC: picp_sim3_batch_time's samples,
hypotheses, score, select and refit stages at 1, 128 and 1,024 problems of 2,000 pairs (30 %
outliers uniform in the cloud's box, 1 cm noise, seed 42), 256 hypotheses, threshold 0.01, two
refits: the minimum of three timings of ten runs, stage by stage.  With --vo, beside them, the
wall time of picp_vo_align_segments (a blocking call: match, compaction, the one read-back and the
five stages) after a run of 63 segments of 40 steps over 2,501 frames of 2,000 observations, pixel
noise 0.5 (the shape of §4.10's map table), at thresholds 0.01, 0.25 and 1.  One JSON line per shape, printed and written to --out.

  sim3_bench.py [--problems 1 128 1024] [--n 2000] [--hyp 256] [--reps 10] [--vo] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 0.01


def cloud(np, n, seed, outlier_frac=0.3, noise=0.01):
    rng = np.random.default_rng([seed, n])
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    c, t = rng.uniform(0.5, 2.0), rng.uniform(-5, 5, 3)
    src = rng.uniform(-5, 5, (n, 3))
    dst = c * src @ R.T + t
    lo, hi = dst.min(0), dst.max(0)
    dst += rng.normal(0, noise, dst.shape)
    k = int(round(outlier_frac * n))
    dst[rng.permutation(n)[:k]] = rng.uniform(lo, hi, (k, 3))
    return src.astype(np.float32), dst.astype(np.float32)


def vo_shape(np, picp_amd, reps):
    from picp_amd.vo_synth import VOSequence, segments
    n_frames, obs, seg_len = 2501, 2000, 40
    s = VOSequence(n_frames, obs_per_frame=obs, seed=42, pixel_noise=0.5)
    F = s.frames(0, n_frames)
    first, steps = segments(n_frames, seg_len)
    boot = np.stack([[F["T_cw"][f], F["T_cw"][f + 1]] for f in first])
    seq = picp_amd.VOSequence(F["frame_off"], F["uv"], F["desc"], K=s.K)
    seq.set_segments(first, steps, boot, threshold=3000.0)
    seq.run()
    seq.align_segments()  # untimed: first-launch costs
    points = sum(len(seq.map(k)[0]) for k in range(len(first)))
    recs = []
    for thr in (THR, 0.25, 1.0):  # 10 cm, 50 cm, 1 m: the maps carry the run's drift and triangulation noise
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = seq.align_segments(threshold=thr)
            ms.append(1e3 * (time.perf_counter() - t0))
        sc = np.array([d["scale"] for d in out if d["found"]])
        recs.append({"shape": "vo 63 x 40", "threshold": thr, "segments": len(first), "map_points": int(points),
                     "pairs": int(sum(d["n_pairs"] for d in out)), "found": int(sum(d["found"] for d in out)),
                     "inliers": int(sum(d["inliers"] for d in out)), "align_ms_min": round(min(ms), 3),
                     "align_ms_median": round(float(np.median(ms)), 3),
                     "scale_min": round(float(sc.min()), 4) if len(sc) else None,
                     "scale_median": round(float(np.median(sc)), 4) if len(sc) else None,
                     "scale_max": round(float(sc.max()), 4) if len(sc) else None})
    seq.close()
    return recs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 128, 1024])
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vo", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18", "sim3", "sim3_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "02-visualodometry_amd"))
    import numpy as np
    import picp_amd
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for P in a.problems:
            src, dst = zip(*[cloud(np, a.n, 42 + i) for i in range(P)])
            res = picp_amd.sim3_ransac_batch(src, dst, threshold=THR, hypotheses=a.hyp, debug=True)
            valid = int(sum(int(d["hyp_valid"].sum()) for d in res))
            us = np.min([picp_amd.sim3_ransac_time(src, dst, a.reps, threshold=THR, hypotheses=a.hyp)
                         for _ in range(3)], 0)
            emit({"problems": P, "n": a.n, "hypotheses": a.hyp, "refits": 2, "valid_hypotheses": valid,
                  "found": int(sum(d["found"] for d in res)), "inliers": int(sum(d["inliers"] for d in res)),
                  "samples_us": round(float(us[0]), 2), "hyp_us": round(float(us[1]), 2),
                  "score_us": round(float(us[2]), 2), "select_us": round(float(us[3]), 2),
                  "refit_us": round(float(us[4]), 2),
                  "scored_pair_hyps_per_s": round(a.n * valid / (us[2] * 1e-6), 0)})
        if a.vo:
            for rec in vo_shape(np, picp_amd, a.reps):
                emit(rec)


if __name__ == "__main__":
    main()
