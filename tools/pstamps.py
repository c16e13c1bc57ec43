#!/usr/bin/env python3
"""Phase breakdown of the persistent kernel (diagnostic stamp build), rounds 11 and 12.
Stamps: 0 round start, 1 partial published, 2 leader: sweep done / others: pose received,
3 leader: solve done; the sweep passes (issue, return) of each of the leader's 8 waves (its first lane still sweeping),
with the wave's post-linearize barrier and pass count; and what a round waits
for besides its hand-offs (6, 7): in a follower, wave 1's round start and pose barrier beside the
polling wave's (0, 2); in a solver, the sweep's exit and the end of the double sums.
Slot 8 is a solver's pose stores (wave 0), so a follower's detection delay is its pose barrier (2)
less its solver's slot 8; slots 9 and 10 are one pose poll of the follower, issued and returned
right after its publish (the round trip of an sc1 load when no pose can be there yet), and slot 11
says whether it polls the L2 copy of the pose."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "02-visualodometry_amd"))
os.environ["PICP_LIB"] = os.environ.get("PICP_STAMPS_LIB") or os.path.join(ROOT, "02-visualodometry_amd", "lib", "libpicp_amd_stamps.so")


def hist40(x):
    """Counts in 40 ns steps (the stamps' own step), as 'from:count' pairs."""
    import numpy as np
    b = (np.asarray(x) // 40) * 40
    return " ".join("%d:%d" % (v, int((b == v).sum())) for v in sorted(set(b.tolist())))


def pose_fanout(st, ns, nb):
    """Solver pose stores (slot 8) -> each follower's pose barrier (slot 2), by solver; the
    followers' own poll round trip (slots 9, 10) and which pose copy they poll (slot 11)."""
    import numpy as np
    kb = np.arange(ns, nb)
    delay = (st[kb, 2] - st[kb % ns, 8]) * 10
    print("  pose stored -> follower pose barrier (%d followers): min %d median %d max %d, spread %d ns" % (
        len(kb), delay.min(), np.median(delay), delay.max(), delay.max() - delay.min()))
    print("    histogram (ns:followers): %s" % hist40(delay))
    for g in range(ns):
        d = delay[kb % ns == g]
        if len(d):
            print("    solver %d (%2d followers): min %d median %d max %d  %s" % (g, len(d), d.min(), np.median(d), d.max(), hist40(d)))
    first = (st[:ns, 8].min() - st[:, 0].min()) * 10
    last_f = (st[kb, 2].max() - st[:, 0].min()) * 10
    print("    first pose store at %d, last at %d, last follower barrier at %d (ns from the first round start)" % (
        first, (st[:ns, 8].max() - st[:, 0].min()) * 10, last_f))
    rtt = (st[kb, 10] - st[kb, 9]) * 10
    print("  follower poll round trip (issue -> returned, right after the publish): min %d median %d max %d  %s" % (
        rtt.min(), np.median(rtt), rtt.max(), hist40(rtt)))
    l2 = st[kb, 11]
    print("  followers polling the L2 copy: %d, the agent-scope copy: %d%s" % (
        int((l2 != 0).sum()), int((l2 == 0).sum()),
        "" if (l2 != 0).all() else "  (agent-scope: blocks %s, delays %s)" % (kb[l2 == 0].tolist(), delay[l2 == 0].tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--outlier", type=float, default=0.0)
    args = ap.parse_args()
    import numpy as np
    import picp_amd
    from picp_amd import synth
    p = synth.make_problem(args.n, seed=42, outlier_frac=args.outlier, pixel_noise=0.5, shuffle=False)
    b = picp_amd.Batch([args.n])
    info = b.info()
    assert info["mode"] == "persistent", info
    b.set_data(p["xyz"], p["uv"])
    b.set_poses(p["T_init"][None])
    L = picp_amd.lib()
    L.picp_debug_sweepstamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    sw = np.zeros((2, 8, 64), np.uint64)  # round, wave, slot (picp_persistent.hip picp_sweepstamps)
    for _ in range(3):
        assert L.picp_debug_sweepstamps(sw.ctypes.data, sw.size) == 0  # read = clear
        b.solve(threshold=3000.0, max_rounds=50, conv_eps=-1.0)
    assert L.picp_debug_sweepstamps(sw.ctypes.data, sw.size) == 0
    nb = info["n_blocks"]
    L.picp_debug_pstamps.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    buf = np.zeros((2, 256, 12), np.uint64)  # round, block, slot (picp_persistent.hip picp_pstamps)
    assert L.picp_debug_pstamps(buf.ctypes.data, buf.size) == 0
    for r in (0, 1):
        st = buf[r, :nb].astype(np.int64)
        t0 = st[:, 0].min()
        rel = (st - t0) * 10
        print("round %d (%d blocks), ns from first round start" % (11 + r, nb))
        print("  leader: start %d published %d swept(all threads) %d combined %d solve_start %d solve_end %d" % (rel[0,0], rel[0,1], rel[0,2], rel[0,3], rel[0,4], rel[0,5]))
        # blocks 1..7 are the other solvers (picp_persistent.hip PICP_PSOLVERS), the rest followers
        ns = min(8, nb)
        if ns > 1:
            sol = rel[1:ns]
            print("  solvers 1-%d: published median %d, swept median %d (max %d), solve_end median %d (max %d)" % (
                ns - 1, np.median(sol[:, 1]), np.median(sol[:, 2]), sol[:, 2].max(), np.median(sol[:, 5]), sol[:, 5].max()))
        others = rel[ns:] if nb > ns else rel[1:]
        for k, nm in enumerate(["start", "published", "pose_received"]):
            print("  followers %-11s median %6d  min %6d  max %6d" % (nm, np.median(others[:, k]), others[:, k].min(), others[:, k].max()))
        # what the round waits for besides its hand-offs (stamps 6 and 7)
        print("  solver sweep exit -> double sums done: leader %d, solvers median %d (max %d)" % (
            rel[0, 7] - rel[0, 6], np.median(rel[:ns, 7] - rel[:ns, 6]), (rel[:ns, 7] - rel[:ns, 6]).max()))
        if r == 1 and nb > ns:
            # a follower's pose barrier of round 11 -> its start of round 12: the polling wave
            # (thread 0: stamps 2, 0) beside wave 1, which has nothing in flight (stamps 7, 6)
            w0 = (buf[1, ns:nb, 0].astype(np.int64) - buf[0, ns:nb, 2].astype(np.int64)) * 10
            w1 = (buf[1, ns:nb, 6].astype(np.int64) - buf[0, ns:nb, 7].astype(np.int64)) * 10
            print("  followers pose barrier r11 -> start r12: polling wave median %d (min %d max %d), wave 1 median %d (min %d max %d)" % (
                np.median(w0), w0.min(), w0.max(), np.median(w1), w1.min(), w1.max()))
            # and on to the block's publish of round 12 (every wave's row is needed)
            pub = (buf[1, ns:nb, 1].astype(np.int64) - buf[0, ns:nb, 2].astype(np.int64)) * 10
            print("  followers pose barrier r11 -> published r12: median %d (min %d max %d)" % (
                np.median(pub), pub.min(), pub.max()))
        if nb > ns:
            pose_fanout(st, ns, nb)
        last_pub = int(rel[:, 1].max())
        # the leader's sweep passes of every wave: issue -> loads returned, ns from the round
        # start (slot 62: the wave's post-linearize barrier, 63: its pass count)
        first = []
        for w in range(sw.shape[1]):
            p = sw[r, w].astype(np.int64)
            n = int(p[63])
            passes = [((p[2 * i] - t0) * 10, (p[2 * i + 1] - t0) * 10) for i in range(min(n, 31)) if p[2 * i + 1]]
            print("  leader wave %d: barrier %d, %d passes (issue..return ns): %s" % (
                w, (p[62] - t0) * 10 if p[62] else -1, n, "  ".join("%d..%d" % x for x in passes)))
            if passes:
                first.append(passes[0][0])
                dur = [b - a for a, b in passes]
                after = [x for x in passes if x[0] >= last_pub]
                print("    pass duration median %d ns (min %d max %d); %d issued after the last publish (%d)" %
                      (np.median(dur), min(dur), max(dur), len(after), last_pub))
        if first:
            print("  first pass issued: wave 0 at %d, waves 1-7 at %s; spread %d ns" % (
                first[0], " ".join(str(x) for x in first[1:]), max(first) - min(first)))
            print("  last publish %d -> swept(all threads) %d: %d ns; swept -> pose stored (solve_end) %d ns" % (
                last_pub, rel[0, 2], rel[0, 2] - last_pub, rel[0, 5] - rel[0, 2]))
    nxt = (buf[1, :nb, 0].astype(np.int64).min() - buf[0, :nb, 0].astype(np.int64).min()) * 10
    print("round period (first start r11 -> first start r12): %d ns" % nxt)


if __name__ == "__main__":
    main()
