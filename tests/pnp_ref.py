"""numpy float64 restatement of the device P3P RANSAC (csrc/picp_pnp.hip): the sampling function
(include/picp_c.h picp_pnp_batch), Grunert's P3P and the selection rule.  Inlier counts are never
restated here: they come from the CPU oracle's linearize at the float32 pose, as for picp_classify.
"""
import numpy as np

M64 = (1 << 64) - 1
# (n, seed) of the end-to-end cases (50 % outliers, 0.5 px noise) the CPU and the GPU tests share
E2E_CASES = [(n, seed) for n in (64, 500) for seed in (100, 101, 102, 103)]


def mix64(x):
    """splitmix64's output function of the state x + golden gamma."""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_triple(seed, i, h, n):
    """Three distinct indices in [0, n) of hypothesis h of problem i (n >= 3): a pure function."""
    key = mix64((seed & M64) ^ mix64(((i & 0xFFFFFFFF) << 32) | (h & 0xFFFFFFFF)))
    r = [mix64((key + j) & M64) >> 32 for j in range(3)]
    a = (r[0] * n) >> 32
    b = (r[1] * (n - 1)) >> 32
    b += b >= a                      # skip past a
    c = (r[2] * (n - 2)) >> 32
    lo, hi = min(a, b), max(a, b)
    c += c >= lo                     # skip past the smaller, then the larger
    c += c >= hi
    return a, b, c


def samples(seed, i, H, n):
    """(H, 3) int32; zeros when n < 4 (no hypothesis is formed)."""
    out = np.zeros((H, 3), np.int32)
    if n >= 4:
        for h in range(H):
            out[h] = sample_triple(seed, i, h, n)
    return out


def bearings(K, uv):
    """Unit bearings K^-1 (u, v, 1) of (m, 2) pixels."""
    Kinv = np.linalg.inv(np.asarray(K, np.float64))
    f = (Kinv @ np.column_stack([np.asarray(uv, np.float64), np.ones(len(uv))]).T).T
    return f / np.linalg.norm(f, axis=1, keepdims=True)


def _triad(A, B, C):
    e1 = (B - A) / np.linalg.norm(B - A)
    e3 = np.cross(e1, C - A)
    e3 /= np.linalg.norm(e3)
    return np.column_stack([e1, np.cross(e3, e1), e3])


def _conic_residual(g, x, y):
    """The two distance-ratio conics divided by b^2 at x = s2/s1 - 1, y = s3/s1 - 1, as sums of
    small terms (csrc/picp_p3p.h p3p_residual) -> (F, the sum of the magnitudes of F's terms)."""
    ma, mb, mg, cb2, ab2 = g
    t0, t1 = x * x + 2 * (1 + x) * mg, y * y + 2 * (1 + y) * mb
    t2 = (x - y) ** 2 + 2 * (1 + x) * (1 + y) * ma
    return np.array([t0 - cb2 * t1, ab2 * t1 - t2]), abs(t0) + cb2 * abs(t1) + ab2 * abs(t1) + abs(t2)


def _polish(g, x, y):
    """Up to six Newton steps on both conics, each taken only while it lowers |F0| + |F1|
    -> (x, y, whether the point ends on both conics to 1e-12 of the terms)."""
    ma, mb, mg, cb2, ab2 = g
    F, size = _conic_residual(g, x, y)
    best, cx, cy = np.abs(F).sum(), x, y
    on = best <= 1e-12 * size
    for _ in range(6):
        j00, j01 = 2 * (cx + mg), -2 * cb2 * (cy + mb)
        j10 = -2 * ((cx - cy) + (1 + cy) * ma)
        j11 = 2 * ab2 * (cy + mb) - 2 * ((cy - cx) + (1 + cx) * ma)
        det = j00 * j11 - j01 * j10
        if not abs(det) > 0:
            break
        cx, cy = cx - (F[0] * j11 - F[1] * j01) / det, cy - (F[1] * j00 - F[0] * j10) / det
        F, size = _conic_residual(g, cx, cy)
        if not np.abs(F).sum() < best:
            break
        best, x, y = np.abs(F).sum(), cx, cy
        on = best <= 1e-12 * size
    return x, y, on


def p3p(P, f, K=None, uv=None, tol_px=1e-3):
    """Grunert's P3P as csrc/picp_p3p.h has it (numpy.roots in place of the bisection).  P (3, 3)
    world points, f (3, 3) unit bearings -> list of at most four float64 4x4 world-in-camera poses
    with three positive depths.  The quartic is in y = s3/s1 - 1, built from 1 - cos of the
    bearings' angles.  Candidates for y: its real roots and, when fewer than four, its critical
    points where it all but vanishes (roots of even multiplicity); x = s2/s1 - 1 by the
    elimination's quotient, or by the first conic where the quotient's denominator is small; every
    (x, y) polished on both conics and kept only if it ends on them; copies dropped.  With K and uv
    a root is kept only if it reprojects its own three points within tol_px (the device's rule)."""
    P = np.asarray(P, np.float64)
    f = np.asarray(f, np.float64)
    if not (np.all(np.isfinite(P)) and np.all(np.isfinite(f))):
        return []
    a2 = np.sum((P[1] - P[2]) ** 2)
    b2 = np.sum((P[0] - P[2]) ** 2)
    c2 = np.sum((P[0] - P[1]) ** 2)
    nrm = np.cross(P[1] - P[0], P[2] - P[0])
    if not (a2 > 0 and b2 > 0 and c2 > 0 and nrm @ nrm > 1e-10 * b2 * c2):
        return []
    ma, mb, mg = (0.5 * np.sum((f[i] - f[j]) ** 2) for i, j in ((1, 2), (0, 2), (0, 1)))
    cb2, ab2, q = c2 / b2, a2 / b2, (a2 - c2) / b2
    g = (ma, mb, mg, cb2, ab2)
    # descending in y, as numpy has polynomials
    D = np.array([1 - ma, mg - ma])
    N = np.array([q - 1, 2 * (q * mb - ma), 2 * ((mg - ma) + q * mb)])
    c0 = np.array([-cb2, -2 * cb2 * mb, 2 * (mg - cb2 * mb)])
    coef = np.polyadd(np.polysub(np.polymul(N, N), 4 * mg * np.polymul(N, D)), 4 * np.polymul(np.polymul(D, D), c0))
    coef = np.concatenate([np.zeros(5 - len(coef)), coef])
    if not np.all(np.isfinite(coef)) or not np.any(coef[:-1] != 0):
        return []

    def real(roots):
        return sorted(z.real for z in roots if abs(z.imag) <= 1e-9 * max(1.0, abs(z.real)))

    ys = real(np.roots(coef))
    if len(ys) < 4:
        for c in real(np.roots(np.polyder(coef))):
            if abs(np.polyval(coef, c)) <= 1e-12 * np.polyval(np.abs(coef), abs(c)):
                ys.append(c)
    out, kept = [], []
    Pc = P.mean(0)
    W = _triad(P[0], P[1], P[2])
    for y0 in ys:
        if not y0 > -1:
            continue
        den = D[1] + D[0] * y0
        if abs(den) >= 1e-4 * (abs(D[1]) + abs(D[0] * y0)):
            xs = [-np.polyval(N, y0) / (2 * den)]
        else:
            cy = np.polyval(c0, y0)
            disc = mg * mg - cy
            sq = np.sqrt(max(disc, 0.0))
            xs = [] if not disc >= -1e-9 * (mg * mg + abs(cy)) else [-mg + sq, -mg - sq] if sq > 0 else [-mg + sq]
        for x in xs:
            if len(out) == 4:
                break
            x, y, on = _polish(g, x, y0)
            u, v = 1 + x, 1 + y
            d1 = y * y + 2 * v * mb
            if not (on and u > 0 and v > 0 and d1 > 0):
                continue
            if any(abs(x - xk) + abs(y - yk) <= 1e-6 * (abs(x) + abs(y) + ma + mb + mg) for xk, yk in kept):
                continue
            s1 = np.sqrt(b2 / d1)
            Q = np.array([s1, u * s1, v * s1])[:, None] * f
            R = _triad(Q[0], Q[1], Q[2]) @ W.T
            T = np.eye(4)
            T[:3, :3] = R
            T[:3, 3] = Q.mean(0) - R @ Pc
            if not np.all(np.isfinite(T)):
                continue
            if K is not None and reproj_err(T, K, P, uv).max() > tol_px:
                continue
            out.append(T)
            kept.append((x, y))
    return out


def reproj_err(T, K, P, uv):
    """Pixel distance of each of P projected at T (float64) from uv."""
    pc = (np.asarray(T, np.float64)[:3, :3] @ np.asarray(P, np.float64).T).T + np.asarray(T, np.float64)[:3, 3]
    ph = (np.asarray(K, np.float64) @ pc.T).T
    return np.linalg.norm(ph[:, :2] / ph[:, 2:3] - np.asarray(uv, np.float64), axis=1)


def hypotheses(xyz, uv, K, seed, i, H):
    """Per hypothesis the list of float32 4x4 poses (what the device stores, scores and returns)."""
    n = len(xyz)
    f = bearings(K, uv) if n else np.zeros((0, 3))
    S = samples(seed, i, H, n)
    out = []
    for h in range(H):
        if n < 4:
            out.append([])
            continue
        idx = S[h]
        out.append([T.astype(np.float32) for T in p3p(xyz[idx], f[idx], K, uv[idx])])
    return out


def count(O, T, K, rows, cols, xyz, uv, thr):
    """Inliers of the packed correspondences at T: the oracle's own gate."""
    n = len(xyz)
    pairs = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    return int(O.linearize(T, K, rows, cols, xyz, uv, pairs, thr)["n_in"])


def select(counts, n_roots):
    """Winner of (H, 4) counts with n_roots (H,) valid roots each: the largest count, then the
    lowest hypothesis, then the lowest root.  -> (h, r, count) or None when no hypothesis has a root."""
    best = None
    for h in range(len(n_roots)):
        for r in range(int(n_roots[h])):
            c = int(counts[h][r])
            if best is None or c > best[2]:
                best = (h, r, c)
    return best


def ransac(O, xyz, uv, K, rows, cols, thr=9.0, H=256, min_inliers=4, seed=0, i=0):
    """The whole reference: dict(T, inliers, found, hyps, counts, n_roots)."""
    xyz = np.asarray(xyz, np.float32)
    uv = np.asarray(uv, np.float32)
    hyps = hypotheses(xyz, uv, K, seed, i, H)
    n_roots = np.array([len(x) for x in hyps], np.int32)
    counts = np.zeros((H, 4), np.int32)
    for h, Ts in enumerate(hyps):
        for r, T in enumerate(Ts):
            counts[h, r] = count(O, T, K, rows, cols, xyz, uv, thr)
    w = select(counts, n_roots)
    found = w is not None and w[2] >= min_inliers and len(xyz) >= 4
    T = hyps[w[0]][w[1]] if found else np.eye(4, dtype=np.float32)
    return {"T": T, "inliers": w[2] if w else 0, "found": bool(found), "hyps": hyps, "counts": counts,
            "n_roots": n_roots}
