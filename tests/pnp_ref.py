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


def p3p(P, f, K=None, uv=None, tol_px=1e-3):
    """Grunert's P3P.  P (3, 3) world points, f (3, 3) unit bearings -> list of float64 4x4
    world-in-camera poses with three positive depths.  With K and uv a root is kept only if it
    reprojects its own three points within tol_px (the device's acceptance rule)."""
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
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    q, r = (a2 - c2) / b2, (a2 + c2) / b2
    cb2, ab2 = c2 / b2, a2 / b2
    A4 = (q - 1) ** 2 - 4 * cb2 * ca ** 2
    A3 = 4 * (q * (1 - q) * cb - (1 - r) * ca * cg + 2 * cb2 * ca ** 2 * cb)
    A2 = 2 * (q ** 2 - 1 + 2 * q ** 2 * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2 - 4 * r * ca * cb * cg
              + 2 * ((b2 - a2) / b2) * cg ** 2)
    A1 = 4 * (-q * (1 + q) * cb + 2 * ab2 * cg ** 2 * cb - (1 - r) * ca * cg)
    A0 = (1 + q) ** 2 - 4 * ab2 * cg ** 2
    coef = np.array([A4, A3, A2, A1, A0])
    if not np.all(np.isfinite(coef)) or not np.any(coef[:-1] != 0):
        return []
    out = []
    Pc = P.mean(0)
    W = _triad(P[0], P[1], P[2])
    for root in np.roots(coef):
        if abs(root.imag) > 1e-9 * max(1.0, abs(root.real)) or not root.real > 0:
            continue
        v = root.real
        den = cg - v * ca
        if abs(den) < 1e-9:
            continue
        u = ((q - 1) * v * v - 2 * q * cb * v + 1 + q) / (2 * den)
        d1 = 1 + v * v - 2 * v * cb
        if not (u > 0 and d1 > 0):
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
