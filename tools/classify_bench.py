#!/usr/bin/env python3
"""Timings of the observation layer: the classify pass beside the streaming
round kernel, and the VO sequence with the track counters off and on.  One JSON line per figure.

  classify_bench.py --classify 100000 1000000 16000000 [--reps 20]
      per size (one frame, PICP_MODE=graph): picp_batch_classify_time with state only and with
      chi2 (algorithmic bytes: 21 / 25 B per item + 4 B per inlier; the projection output exists
      only on the single-problem call and has no device timer), and from the same process
      picp_batch_time's launch_us of the streaming round kernel at the same shape.
  classify_bench.py --vo 8e 250 [--reps 2] [--samples 5] [--pkg DIR]
      picp_vo_time of the bench's C5 sequence (10,000 frames x 2,000 observations, seed 42) as 8
      segments of 1,250 steps (8e) or 250 of 40; with tracking off, then on when the library has
      the switch.  --pkg DIR imports picp_amd from DIR (another build of the package, e.g. the
      parent commit's, for the same-session comparison).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 3000.0


def classify(sizes, reps):
    import numpy as np
    import picp_amd
    from picp_amd import synth
    os.environ["PICP_MODE"] = "graph"  # the streaming round kernel, one launch per round
    for n in sizes:
        p = synth.make_problem(n, seed=42, outlier_frac=0.3, pixel_noise=0.5, shuffle=False)
        b = picp_amd.Batch([n])
        b.set_data(p["xyz"], p["uv"])
        b.set_poses(p["T_init"][None])
        c = b.classify(THR, want_chi2=False)
        n_in = int(c["counts"][0, 1])
        t_state = min(b.classify_time(THR, reps) for _ in range(3))
        b.classify(THR)
        t_chi2 = min(b.classify_time(THR, reps) for _ in range(3))
        b.set_poses(p["T_init"][None])
        launch = min(b.time(2, threshold=THR, max_rounds=10, conv_eps=-1.0)[1] for _ in range(3))
        info = b.info()
        b.close()
        by_state, by_chi2 = 21 * n + 4 * n_in, 25 * n + 4 * n_in
        print(json.dumps({"classify": n, "inliers": n_in, "state_us": round(t_state, 2),
                          "state_GBps": round(by_state / t_state / 1e3, 1), "chi2_us": round(t_chi2, 2),
                          "chi2_GBps": round(by_chi2 / t_chi2 / 1e3, 1), "round_kernel_launch_us": round(launch, 2),
                          "round_kernel_GBps": round(20 * n / launch / 1e3, 1), "mode": info["mode"],
                          "round_blocks": info["n_blocks"]}), flush=True)


def vo(shapes, reps, samples):
    import numpy as np
    import picp_amd
    from picp_amd.vo_synth import VOSequence, segments
    F, obs = 10000, 2000
    seq = VOSequence(F, obs_per_frame=obs, seed=42)
    D = seq.frames(0, F)
    for shape in shapes:
        L = -(-(F - 1) // 8) if shape == "8e" else 40
        first, steps = segments(F, L)
        rel = [np.linalg.inv(D["T_cw"][f].astype(np.float64)) for f in first]
        boot = np.stack([[np.eye(4), rel[k] @ D["T_cw"][f + 1]] for k, f in enumerate(first)]).astype(np.float32)
        h = picp_amd.VOSequence(D["frame_off"], D["uv"], D["desc"], K=seq.K)
        h.set_segments(first, steps, boot, threshold=THR)
        h.run()
        out = {"vo": shape, "segments": len(first), "steps": int(steps.max()), "lib": picp_amd.LIB_PATH}
        modes = [("off", False)] + ([("on", True), ("off_again", False)] if hasattr(h, "track_stats") else [])
        for name, on in modes:
            if hasattr(h, "track_stats"):
                h.track_stats(on)
            h.run()
            out[name + "_ms"] = [round(h.time(reps), 3) for _ in range(samples)]
        if "on_ms" in out:
            off = min(out["off_ms"] + out["off_again_ms"])
            out["on_added_us_per_chain_step"] = round(1e3 * (min(out["on_ms"]) - off) / int(steps.max()), 3)
        h.close()
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--classify", type=int, nargs="*", default=[])
    ap.add_argument("--vo", nargs="*", default=[], choices=["8e", "250"])
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "02-visualodometry_amd"))
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    if a.classify:
        classify(a.classify, a.reps or 20)
    if a.vo:
        vo(a.vo, a.reps or 2, a.samples)


if __name__ == "__main__":
    main()
