#!/usr/bin/env python3
"""Per-stage device times of the P3P RANSAC: picp_pnp_batch_time's samples,
solve, score and select stages at 1, 128 and 1,024 problems of 2,000 correspondences (30 %
outliers, 0.5 px noise, seed 42), 256 hypotheses, and beside them picp_batch_classify_time of the
same batch: the classify pass evaluates the same gate once per item, the score stage once per
(item, pose).  One JSON line per shape, printed and written to --out.

  pnp_bench.py [--problems 1 128 1024] [--n 2000] [--hyp 256] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 9.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, nargs="*", default=[1, 128, 1024])
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--hyp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "pnp", "pnp_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "02-visualodometry_amd"))
    import numpy as np
    import picp_amd
    from picp_amd import synth
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for P in a.problems:
            B = synth.make_batch(P, a.n, base_seed=42, outlier_frac=0.3, pixel_noise=0.5)
            xyz = list(B["xyz"].reshape(P, a.n, 3))
            uv = list(B["uv"].reshape(P, a.n, 2))
            res = picp_amd.pnp_ransac_batch(xyz, uv, threshold=THR, hypotheses=a.hyp, debug=True)
            poses = int(sum(int(d["n_roots"].sum()) for d in res))
            found = sum(d["found"] for d in res)
            # the minimum of three timings of `reps` runs each, stage by stage
            us = np.min([picp_amd.pnp_ransac_time(xyz, uv, a.reps, threshold=THR, hypotheses=a.hyp) for _ in range(3)], 0)
            b = picp_amd.Batch([a.n] * P)
            b.set_data(B["xyz"], B["uv"])
            b.set_poses(np.stack([d["T"] for d in res]))
            b.classify(THR, want_chi2=False)
            cls_us = min(b.classify_time(THR, a.reps) for _ in range(3))
            b.close()
            items = P * a.n
            rec = {"problems": P, "n": a.n, "hypotheses": a.hyp, "poses": poses, "found": found,
                   "samples_us": round(float(us[0]), 2), "solve_us": round(float(us[1]), 2),
                   "score_us": round(float(us[2]), 2), "select_us": round(float(us[3]), 2),
                   "scored_item_poses_per_s": round(a.n * poses / (us[2] * 1e-6), 0),
                   "classify_us": round(cls_us, 2), "classify_items_per_s": round(items / (cls_us * 1e-6), 0)}
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
