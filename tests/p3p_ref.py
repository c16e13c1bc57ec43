"""An independent P3P in numpy float64 and the triangle families the solver is pinned on.

The device solver (csrc/picp_p3p.h) and its restatement (tests/pnp_ref.py) eliminate u from the two
distance-ratio conics and solve Grunert's quartic in v.  This file does not: it intersects the two
conics through the degenerate members of their pencil, polishes every intersection by Newton on
both conics, and takes the pose by Kabsch/SVD.  Only `bearings` and `reproj_err` are shared.

Unknowns u = s2/s1, v = s3/s1 (s_i the distances of the three points from the camera centre), with
a = |P2 P3|, b = |P1 P3|, c = |P1 P2| and alpha, beta, gamma the angles between the bearings
(f2, f3), (f1, f3), (f1, f2):
    C1: b^2 (1 + u^2 - 2 u cos gamma) = c^2 (1 + v^2 - 2 v cos beta)
    C2: a^2 (1 + v^2 - 2 v cos beta)  = b^2 (u^2 + v^2 - 2 u v cos alpha)
The matrices are written in x = u - 1, y = v - 1 with 1 - cos taken as |f_i - f_j|^2 / 2, since
1 + u^2 - 2 u cos = (u - 1)^2 + 2 u (1 - cos): for a triangle that spans a hundredth of a radian
x, y and 1 - cos are near 1e-4, and in (u, v) the conics' values there would be rounding noise.
"""
import numpy as np

from pnp_ref import bearings, reproj_err

K_PIN = np.array([[180.0, 0.0, 320.0], [0.0, 180.0, 240.0], [0.0, 0.0, 1.0]], np.float32)
K_SKEW = np.array([[183.0, 0.75, 318.5], [0.0, 176.5, 243.25], [0.0, 0.0, 1.0]], np.float32)  # test_gpu_pnp.K_SKEW
N_CASES = 64
N_PROBES = 5
ACCEPT_PX = 1e-3   # the solver's own acceptance radius
TOL_FACTOR = 4.0   # tol_r = ACCEPT_PX + TOL_FACTOR * floor_r
ISOLATED_PX = 1.0


# ------------------------------------------------------------------------------------------------
# the solver
# ------------------------------------------------------------------------------------------------
def _conics(P, f):
    """C1, C2 as symmetric matrices on (x, y, 1), and (1 - cos alpha, 1 - cos beta, 1 - cos gamma)."""
    a2 = np.sum((P[1] - P[2]) ** 2)
    b2 = np.sum((P[0] - P[2]) ** 2)
    c2 = np.sum((P[0] - P[1]) ** 2)
    ma, mb, mg = (0.5 * np.sum((f[i] - f[j]) ** 2) for i, j in ((1, 2), (0, 2), (0, 1)))
    C1 = np.array([[b2, 0.0, b2 * mg], [0.0, -c2, -c2 * mb], [b2 * mg, -c2 * mb, 2 * (b2 * mg - c2 * mb)]])
    C2 = np.array([[-b2, b2 * (1 - ma), -b2 * ma], [b2 * (1 - ma), a2 - b2, a2 * mb - b2 * ma],
                   [-b2 * ma, a2 * mb - b2 * ma, 2 * (a2 * mb - b2 * ma)]])
    s = max(a2, b2, c2)
    return C1 / s, C2 / s, (ma, mb, mg)


def _adj(M):
    return np.array([np.cross(M[1], M[2]), np.cross(M[2], M[0]), np.cross(M[0], M[1])]).T


def _lines(D):
    """The two real lines of the degenerate conic D (rank <= 2), or [] when they are complex."""
    scale = np.abs(D).max()
    if not scale > 0:
        return []
    B = -_adj(D)
    i = int(np.argmax(np.abs(np.diag(B))))
    if abs(B[i, i]) <= 1e-14 * scale * scale:  # rank one: a double line
        r = int(np.argmax(np.abs(D).sum(1)))
        return [D[r], D[r]]
    if B[i, i] < 0:
        return []
    p = B[:, i] / np.sqrt(B[i, i])
    M = D + np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])
    r, c = np.unravel_index(int(np.argmax(np.abs(M))), (3, 3))
    return [M[r, :], M[:, c]]


def _line_conic(l, C):
    """Homogeneous points where the line l meets the conic C (a negative discriminant is taken as a
    tangency: the residual filter after the polish decides)."""
    k = int(np.argmax(np.abs(l)))
    e = np.eye(3)
    p0 = np.cross(l, e[(k + 1) % 3])
    d = np.cross(l, p0)
    A, Bq, Cq = d @ C @ d, p0 @ C @ d, p0 @ C @ p0
    out = []
    if abs(A) >= abs(Cq):
        if A == 0:
            return out
        s = np.sqrt(max(Bq * Bq - A * Cq, 0.0))
        for t in ((-Bq + s) / A, (-Bq - s) / A):
            out.append(p0 + t * d)
    else:
        s = np.sqrt(max(Bq * Bq - A * Cq, 0.0))
        for t in ((-Bq + s) / Cq, (-Bq - s) / Cq):
            out.append(t * p0 + d)
    return out


def _resid(C, x):
    size = np.abs(x) @ np.abs(C) @ np.abs(x)
    return abs(x @ C @ x) / size if size > 0 else 0.0


def _newton(C1, C2, u, v, steps=8):
    for _ in range(steps):
        x = np.array([u, v, 1.0])
        F = np.array([x @ C1 @ x, x @ C2 @ x])
        J = 2.0 * np.array([(C1 @ x)[:2], (C2 @ x)[:2]])
        det = J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]
        if not (np.isfinite(det) and det != 0):
            break
        du = (F[0] * J[1, 1] - F[1] * J[0, 1]) / det
        dv = (F[1] * J[0, 0] - F[0] * J[1, 0]) / det
        if not (np.isfinite(du) and np.isfinite(dv)):
            break
        u, v = u - du, v - dv
    return u, v


def ratios(P, f):
    """Every (x, y) = (u - 1, v - 1) with u, v > 0 on both conics: relative residual <= 1e-9,
    duplicates merged."""
    C1, C2, m = _conics(P, f)
    A1, A2 = _adj(C1), _adj(C2)
    cubic = [np.linalg.det(C2), np.trace(C1 @ A2), np.trace(A1 @ C2), np.linalg.det(C1)]
    cand = []
    for lam in np.roots(cubic):
        if abs(lam.imag) > 1e-6 * max(1.0, abs(lam.real)):
            continue
        for l in _lines(C1 + lam.real * C2):
            for C in (C1, C2):
                for p in _line_conic(l, C):
                    if abs(p[2]) > 1e-12 * np.abs(p).max():
                        cand.append((p[0] / p[2], p[1] / p[2]))
    out = []
    for x, y in cand:
        if not (np.isfinite(x) and np.isfinite(y)):
            continue
        x, y = _newton(C1, C2, x, y)
        if not (x > -1 and y > -1):
            continue
        p = np.array([x, y, 1.0])
        if not (_resid(C1, p) <= 1e-9 and _resid(C2, p) <= 1e-9):
            continue
        if any(abs(x - xo) + abs(y - yo) <= 1e-6 * (abs(x) + abs(y) + sum(m)) for xo, yo in out):
            continue
        out.append((x, y))
    return out


def _kabsch(P, Q):
    Pc, Qc = P.mean(0), Q.mean(0)
    U, _, Vt = np.linalg.svd((P - Pc).T @ (Q - Qc))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = Qc - R @ Pc
    return T


def solve(K, xyz, uv):
    """All world-in-camera poses (float64 4x4) that map the three points onto their pixels."""
    P = np.asarray(xyz, np.float64)
    f = bearings(K, uv)
    sides2 = np.sum((P[1] - P[2]) ** 2) + np.sum((P[0] - P[2]) ** 2) + np.sum((P[0] - P[1]) ** 2)
    ma, mb, mg = _conics(P, f)[2]
    out = []
    for x, y in ratios(P, f):
        u, v = 1 + x, 1 + y
        # the three squared sides at s1 = 1
        unit = (x * x + 2 * u * mg) + (y * y + 2 * v * mb) + ((x - y) ** 2 + 2 * u * v * ma)
        s1 = np.sqrt(sides2 / unit)
        T = _kabsch(P, np.array([s1, u * s1, v * s1])[:, None] * f)
        if np.all(np.isfinite(T)):
            out.append(T)
    return out


# ------------------------------------------------------------------------------------------------
# the metric
# ------------------------------------------------------------------------------------------------
def project(T, K, X):
    pc = X @ T[:3, :3].T + T[:3, 3]
    ph = pc @ np.asarray(K, np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        return ph[:, :2] / ph[:, 2:3]


def probe_px(Ta, Tb, K, probes):
    """The probe discrepancy: the largest pixel distance of the probes seen from Ta and from Tb."""
    d = np.linalg.norm(project(np.asarray(Ta, np.float64), K, probes) -
                       project(np.asarray(Tb, np.float64), K, probes), axis=1)
    return float(d.max()) if np.all(np.isfinite(d)) else float("inf")


def rounded(T):
    return np.asarray(T, np.float64).astype(np.float32).astype(np.float64)


class Case:
    """One triangle with its reference root set on the float32 inputs."""

    def __init__(self, K, xyz, uv, T_true, probes):
        self.K, self.xyz, self.uv, self.T_true, self.probes = K, xyz, uv, T_true, probes
        self.roots = solve(K, xyz, uv)
        self.floor = [probe_px(T, rounded(T), K, probes) for T in self.roots]
        self.tol = [ACCEPT_PX + TOL_FACTOR * fl for fl in self.floor]
        self.isolated = [all(probe_px(T, To, K, probes) > ISOLATED_PX for j, To in enumerate(self.roots) if j != i)
                         for i, T in enumerate(self.roots)]

    def compare(self, poses):
        """(spurious, lost, worst): poses with no reference root within its tol_r, isolated reference
        roots with no pose within tol_r, and the largest (d - ACCEPT_PX) / floor_r of the matches."""
        D = np.array([[probe_px(T, Tr, self.K, self.probes) for Tr in self.roots] for T in poses]).reshape(
            len(poses), len(self.roots))
        tol = np.array(self.tol)
        spurious = sum(1 for i in range(len(poses)) if not (D[i] <= tol).any())
        lost = sum(1 for j in range(len(self.roots)) if self.isolated[j] and not (D[:, j] <= tol[j]).any())
        worst = 0.0
        for i in range(len(poses)):
            if len(self.roots):
                j = int(np.argmin(D[i]))
                if D[i, j] <= tol[j] and self.floor[j] > 0:
                    worst = max(worst, (D[i, j] - ACCEPT_PX) / self.floor[j])
        return spurious, lost, worst


# ------------------------------------------------------------------------------------------------
# the families
# ------------------------------------------------------------------------------------------------
def _rot(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _min_angle(X):
    best = np.pi
    for i in range(3):
        a, b = X[(i + 1) % 3] - X[i], X[(i + 2) % 3] - X[i]
        best = min(best, np.arccos(np.clip(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1)))
    return best


def _ray(rng, K):
    """A camera-frame direction (z = 1) through a pixel of the 640 x 480 image, 40 px inside."""
    px = np.array([rng.uniform(40, 600), rng.uniform(40, 440), 1.0])
    return np.linalg.solve(np.asarray(K, np.float64), px)


def _well_shaped(cam, K):
    """Neither the triangle nor its image is a sliver (smallest angle >= 15 deg), all in the image."""
    uv = project(np.eye(4), K, cam)
    inside = (uv[:, 0] > 0).all() and (uv[:, 0] < 639).all() and (uv[:, 1] > 0).all() and (uv[:, 1] < 479).all()
    return bool(inside and (cam[:, 2] > 0.2).all() and _min_angle(cam) >= np.radians(15) and
                _min_angle(np.column_stack([uv, np.zeros(3)])) >= np.radians(15))


def _by_depth(rng, K, depths):
    while True:
        cam = np.array([_ray(rng, K) * z for z in depths(rng)])
        if _well_shaped(cam, K):
            return cam


def _small(rng, K, size, lo=1.0, hi=10.0):
    """A triangle of about `size` metres at lo-hi m, in a plane tilted from facing the camera by
    0-60 deg or, one draw in eight, by less than its own angular size: only there does a small
    triangle have more than two poses (two of them often within a pixel of each other)."""
    while True:
        centre = _ray(rng, K) * rng.uniform(lo, hi)
        n = centre / np.linalg.norm(centre)
        e1 = np.cross(n, rng.normal(size=3))
        e1 /= np.linalg.norm(e1)
        tilt = np.radians(rng.uniform(0, 60)) if rng.integers(8) else rng.uniform(0, 1) * size / np.linalg.norm(centre)
        e2 = np.cos(tilt) * np.cross(n, e1) + np.sin(tilt) * n
        xy = size * rng.uniform(-0.5, 0.5, (3, 2))
        cam = centre + xy[:, :1] * e1 + xy[:, 1:] * e2
        if _well_shaped(cam, K) and min(np.linalg.norm(cam[i] - cam[j]) for i, j in ((0, 1), (0, 2), (1, 2))) > 0.3 * size:
            return cam


def _equilateral(rng, K, eps):
    side, z, phi = rng.uniform(0.5, 2.0), rng.uniform(2.0, 6.0), rng.uniform(0, 2 * np.pi)
    r = side / np.sqrt(3.0)
    cam = np.array([[r * np.cos(phi + k * 2 * np.pi / 3), r * np.sin(phi + k * 2 * np.pi / 3), z] for k in range(3)])
    return cam + eps * rng.normal(size=(3, 3))


def _near_collinear(rng, K):
    cam = _by_depth(rng, K, lambda g: g.uniform(2, 10, 3))
    d = rng.normal(size=3)
    cam[2] = 0.5 * (cam[0] + cam[1]) + 1e-3 * rng.uniform(0.2, 1.0) * d / np.linalg.norm(d)
    return cam


def _equal(eps):
    def make(rng, K):
        cam = _by_depth(rng, K, lambda g: np.full(3, g.uniform(2, 10)))
        return cam + eps * rng.normal(size=(3, 3))
    return make


def _depth_ratio(g):
    d = g.uniform(0.5, 1.0)
    return np.array([d, d * np.exp(g.uniform(0, np.log(200.0))), 200.0 * d])[g.permutation(3)]


# name -> (K, camera-frame triangle maker, strict)
FAMILIES = {
    "generic": (K_PIN, lambda r, K: _by_depth(r, K, lambda g: g.uniform(2, 10, 3)), True),
    "skewed_K": (K_SKEW, lambda r, K: _by_depth(r, K, lambda g: g.uniform(2, 10, 3)), True),
    "far": (K_PIN, lambda r, K: _by_depth(r, K, lambda g: g.uniform(50, 200, 3)), True),
    "depth_ratio": (K_PIN, lambda r, K: _by_depth(r, K, _depth_ratio), True),
    "equal_depths_0": (K_PIN, _equal(0.0), True),
    "equal_depths_1e-4": (K_PIN, _equal(1e-4), True),
    "equilateral_0": (K_PIN, lambda r, K: _equilateral(r, K, 0.0), True),
    "equilateral_1e-6": (K_PIN, lambda r, K: _equilateral(r, K, 1e-6), True),
    "equilateral_1e-4": (K_PIN, lambda r, K: _equilateral(r, K, 1e-4), True),
    "equilateral_1e-2": (K_PIN, lambda r, K: _equilateral(r, K, 1e-2), True),
    "triangle_10cm": (K_PIN, lambda r, K: _small(r, K, 0.1), True),
    "triangle_1cm": (K_PIN, lambda r, K: _small(r, K, 0.01), False),
    "near_collinear": (K_PIN, _near_collinear, False),
}
STRICT = [k for k, v in FAMILIES.items() if v[2]]
REPORT_ONLY = [k for k, v in FAMILIES.items() if not v[2]]


def family(name, n=N_CASES, exact=False):
    """Seeded generator of n cases: (xyz (3, 3), uv (3, 2), T_true float64 4x4 world-in-camera).
    xyz and uv are float32 (the solver's inputs); with exact=True they are the float64 values they
    were rounded from, which T_true maps onto each other to double precision."""
    K, make, _ = FAMILIES[name]
    rng = np.random.default_rng([sorted(FAMILIES).index(name), 20240])
    for _ in range(n):
        cam = make(rng, K)
        T = np.eye(4)
        T[:3, :3] = _rot(rng)
        T[:3, 3] = rng.uniform(-5, 5, 3)
        xyz = (cam - T[:3, 3]) @ T[:3, :3]  # R^T (cam - t)
        uv = project(np.eye(4), K, cam)
        if exact:
            yield xyz, uv, T
        else:
            yield xyz.astype(np.float32), uv.astype(np.float32), T


def probes(name, i, T_true):
    """Five world points, fixed for case i of the family, in the true camera's frustum (x +-2 m,
    y +-1.5 m, z 2-10 m).  The vertices cannot serve: every P3P root maps them to the same pixels."""
    rng = np.random.default_rng([sorted(FAMILIES).index(name), i, 777])
    pc = np.column_stack([rng.uniform(-2, 2, N_PROBES), rng.uniform(-1.5, 1.5, N_PROBES), rng.uniform(2, 10, N_PROBES)])
    return (pc - T_true[:3, 3]) @ T_true[:3, :3]


_CACHE = {}


def cases(name):
    """The family's cases with their reference roots on the float32 inputs (computed once)."""
    if name not in _CACHE:
        K = FAMILIES[name][0]
        _CACHE[name] = [Case(K, xyz, uv, T, probes(name, i, T)) for i, (xyz, uv, T) in enumerate(family(name))]
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------
# the solver's source on the host (bin/p3p_check)
# ------------------------------------------------------------------------------------------------
def pose12(p):
    """12 floats (R column-major, then t), as the solver stores a pose -> float64 4x4."""
    T = np.eye(4)
    T[:3, :3] = np.asarray(p[:9], np.float64).reshape(3, 3).T
    T[:3, 3] = p[9:12]
    return T


def run_p3p_check(exe, path, triangles):
    """bin/p3p_check on (K, xyz (3, 3), uv (3, 2)) triangles -> per triangle the (n, 12) float32 poses."""
    import subprocess
    with open(path, "w") as f:
        for K, xyz, uv in triangles:
            vals = np.concatenate([np.asarray(K, np.float32).T.reshape(-1), np.asarray(xyz, np.float32).reshape(-1),
                                   np.asarray(uv, np.float32).reshape(-1)])
            f.write(" ".join(float(v).hex() for v in vals) + "\n")
    res = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    out = []
    for line in res.stdout.strip().splitlines():
        tok = line.split()
        out.append(np.array([float.fromhex(t) for t in tok[1:]], np.float32).reshape(int(tok[0]), 12))
    assert len(out) == len(triangles)
    return out
