"""Two-view DLT triangulation: the float64-SVD reference, its bounds and the input sets shared by
tests/test_triangulate_reference.py (CPU) and tests/test_gpu_triangulate.py (GPU).

The reference is independent of the oracle (oracle/picp_oracle.c or_triangulate, an eigensolver
of A^T A in long double) and of the kernel (triangulate_dlt, one-sided Jacobi in double): per
point the 4x4 DLT matrix A in float64 from the float32 P1, P2 and pixels -- the same products and
differences both of them form -- then numpy.linalg.svd, the last right singular vector converted
to float32 and dehomogenised in float32 with cv::convertPointsFromHomogeneous' rule (scale 1 when
|w| <= FLT_EPSILON).

Bounds (EPS32 = FLT_EPSILON = 2^-23; every result is the float32 image of the exact minimiser
through one conversion per component, one conversion of w, one reciprocal and one product: four
roundings of 2^-24 each, at most 2.5 EPS32 relative per component):

  (a) residual, whatever the conditioning: with xh = (xyz, 1) -- (xyz, 0) where the reference's
      float w is within FLT_EPSILON -- normalised in float64,
          |A xh| <= sigma4 + RES_C * EPS32 * sigma1,         RES_C = 4
      (|A xh| <= sigma4 + sigma1 |delta|, |delta| <= 2.5 EPS32; 4 adds margin);
  (b) direct, where kappa = sigma1 / (sigma3 - sigma4) <= KAPPA_MAX = 1e3:
          max|xyz - ref| <= DIRECT_C * EPS32 * max|ref|,      DIRECT_C = 4
      (kappa 2^-52 << 2^-24: any two double null vectors agree far below float precision; what
      remains is the same float roundings).
"""
import os

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)  # FLT_EPSILON
RES_C = 4.0
DIRECT_C = 4.0
KAPPA_MAX = 1e3
# the sets on which at least MIN_DIRECT_SHARE of the points must qualify for (b)
DIRECT_SETS = ("general", "noise", "large_focal", "offset_world", "rotated_pair", "forward", "golden")
MIN_DIRECT_SHARE = 0.9
N_PER_SET = 400

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picp_golden.npz")


def dlt_matrices(P1, P2, uv1, uv2):
    """(n, 4, 4) float64: rows u P[2] - P[0], v P[2] - P[1] of each view, as or_triangulate and
    triangulate_dlt form them (float32 inputs widened first)."""
    P1 = np.asarray(P1, np.float32).reshape(3, 4).astype(np.float64)
    P2 = np.asarray(P2, np.float32).reshape(3, 4).astype(np.float64)
    a = np.asarray(uv1, np.float32).reshape(-1, 2).astype(np.float64)
    b = np.asarray(uv2, np.float32).reshape(-1, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.stack([a[:, 0:1] * P1[2] - P1[0], a[:, 1:2] * P1[2] - P1[1],
                         b[:, 0:1] * P2[2] - P2[0], b[:, 1:2] * P2[2] - P2[1]], 1)


def dehomogenise(v):
    """float64 (n, 4) homogeneous -> (xyz float32 (n, 3), w float32 (n,)): points4D is float, then
    convertPointsFromHomogeneous in float."""
    v4 = np.asarray(v, np.float64).astype(np.float32)
    w = v4[:, 3]
    with np.errstate(all="ignore"):
        scale = np.where(np.abs(w) > np.float32(EPS32), np.float32(1.0) / w, np.float32(1.0)).astype(np.float32)
    return (v4[:, :3] * scale[:, None]).astype(np.float32), w


def reference(P1, P2, uv1, uv2):
    """dict(xyz float32, w float32, at_inf bool, A, sig (n, 4) descending, kappa, v float64)."""
    A = dlt_matrices(P1, P2, uv1, uv2)
    _, sig, vt = np.linalg.svd(A)
    v = vt[:, 3, :]
    xyz, w = dehomogenise(v)
    with np.errstate(divide="ignore"):
        kappa = sig[:, 0] / (sig[:, 2] - sig[:, 3])
    return {"xyz": xyz, "w": w, "at_inf": ~(np.abs(w) > np.float32(EPS32)), "A": A, "sig": sig, "kappa": kappa,
            "v": v}


def residual_ratio(ref, got):
    """(|A xh| - sigma4) / (EPS32 sigma1) per point: bound (a) is `<= RES_C`."""
    got = np.asarray(got, np.float64)
    xh = np.concatenate([got, np.where(ref["at_inf"], 0.0, 1.0)[:, None]], 1)
    xh = xh / np.linalg.norm(xh, axis=1, keepdims=True)
    r = np.linalg.norm(np.einsum("nij,nj->ni", ref["A"], xh), axis=1)
    return (r - ref["sig"][:, 3]) / (EPS32 * ref["sig"][:, 0])


def direct_ulps(ref_xyz, got):
    """max|got - ref| / (EPS32 max|ref|) per point: bound (b) is `<= DIRECT_C`."""
    ref_xyz = np.asarray(ref_xyz, np.float64)
    return np.abs(np.asarray(got, np.float64) - ref_xyz).max(1) / (EPS32 * np.abs(ref_xyz).max(1))


def check_bounds(ref, got, name, who):
    """Assert (a) on every point and (b) on every point with kappa <= KAPPA_MAX; returns the worst
    ratios (residual, direct or None)."""
    got = np.asarray(got)
    assert got.shape == ref["xyz"].shape and np.isfinite(got).all(), (name, who)
    res = residual_ratio(ref, got)
    k = int(np.argmax(res))
    assert res[k] <= RES_C, "%s/%s: residual ratio %.3g at point %d (kappa %.3g)" % (name, who, res[k], k,
                                                                                      ref["kappa"][k])
    ok = ref["kappa"] <= KAPPA_MAX
    if name in DIRECT_SETS:
        assert ok.mean() >= MIN_DIRECT_SHARE, "%s: only %.0f %% of the points have kappa <= %g" % (
            name, 100 * ok.mean(), KAPPA_MAX)
    worst_direct = None
    if name in DIRECT_SETS:
        d = direct_ulps(ref["xyz"][ok], got[ok])
        j = int(np.argmax(d))
        assert d[j] <= DIRECT_C, "%s/%s: direct error %.3g ulp at point %d" % (name, who, d[j],
                                                                               int(np.nonzero(ok)[0][j]))
        worst_direct = float(d[j])
    return float(res[k]), worst_direct


# ------------------------------------- input sets -------------------------------------
def _rodrigues(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0.0:
        return np.eye(3)
    k = r / th
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * kx + (1 - np.cos(th)) * kx @ kx


def _K(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])


def _project(P, X):
    """Exact (float64) projection through the float32 P, rounded to float32 pixels."""
    h = np.c_[X, np.ones(len(X))] @ P.astype(np.float64).T
    return (h[:, :2] / h[:, 2:]).astype(np.float32)


def _two_view(rng, n, K, R, C, depth, size, noise=0.0, Rw=None, offset=None, near_axis=0):
    """Camera 1 at the origin, camera 2 with rotation R (world-in-camera) and centre C; points at
    `depth` (lo, hi) seen by camera 1 inside `size` = (cols, rows).  Rw / offset move both cameras
    and the points rigidly in the world (world-in-camera-1 rotation Rw, camera-1 centre offset).
    The first `near_axis` points lie within a few pixels of the principal point."""
    uv = rng.uniform([0, 0], [size[0] - 1, size[1] - 1], (n, 2))
    if near_axis:
        uv[:near_axis] = K[:2, 2] + rng.uniform(-3, 3, (near_axis, 2))
    z = rng.uniform(depth[0], depth[1], n)
    Xc = np.c_[(uv - K[:2, 2]) / K[0, 0], np.ones(n)] * z[:, None]  # camera-1 coordinates
    Rw = np.eye(3) if Rw is None else Rw
    o = np.zeros(3) if offset is None else np.asarray(offset, np.float64)
    Xw = Xc @ Rw + o  # X_c = Rw (X_w - o)
    R1, t1 = Rw, -Rw @ o
    R2, t2 = R @ Rw, R @ t1 - R @ np.asarray(C, np.float64)
    P1 = (K @ np.c_[R1, t1]).astype(np.float32)
    P2 = (K @ np.c_[R2, t2]).astype(np.float32)
    uv1, uv2 = _project(P1, Xw), _project(P2, Xw)
    if noise:
        uv1 = (uv1 + rng.normal(0, noise, uv1.shape)).astype(np.float32)
        uv2 = (uv2 + rng.normal(0, noise, uv2.shape)).astype(np.float32)
    return {"P1": P1, "P2": P2, "uv1": uv1, "uv2": uv2, "K": K, "X": Xw}


R_GEN = (0.05, -0.1, 0.02)
C_GEN = (0.5, 0.1, 0.05)


def input_sets(n=N_PER_SET):
    """name -> dict(P1, P2 (3, 4) float32, uv1, uv2 (n, 2) float32, K); insertion-ordered."""
    K = _K(180.0, 320.0, 240.0)
    R = _rodrigues(R_GEN)
    sets = {}
    sets["general"] = _two_view(np.random.default_rng(101), n, K, R, C_GEN, (3, 10), (640, 480))
    sets["noise"] = _two_view(np.random.default_rng(102), n, K, R, C_GEN, (3, 10), (640, 480), noise=0.5)
    sets["large_focal"] = _two_view(np.random.default_rng(103), n, _K(1000.0, 960.0, 540.0), R, C_GEN, (3, 10),
                                    (1920, 1080))
    # both cameras away from the world origin.  kappa grows with the square of the offset (sigma1
    # with the translation column, 1 / sigma3 with |X|): at 1e3 it is 1e4 .. 2e5 and no point
    # qualifies for (b), so the 1e3 set gets (a) only and a second set, at the largest round offset
    # where the reference's kappa stays under KAPPA_MAX (max 522), gets (a) and (b)
    sets["offset_world"] = _two_view(np.random.default_rng(104), n, K, R, C_GEN, (3, 10), (640, 480),
                                     offset=(5.0, -5.0, 5.0))
    sets["offset_world_1e3"] = _two_view(np.random.default_rng(112), n, K, R, C_GEN, (3, 10), (640, 480),
                                         offset=(1e3, -1e3, 1e3))
    sets["rotated_pair"] = _two_view(np.random.default_rng(105), n, K, R, C_GEN, (3, 10), (640, 480),
                                     Rw=_rodrigues((0.0, 1.6, 0.0)))
    # forward motion: the epipole is the principal point; 40 points within 3 px of it
    sets["forward"] = _two_view(np.random.default_rng(106), n, K, np.eye(3), (0.0, 0.0, 0.5), (3, 10), (640, 480),
                                near_axis=40)
    sets["short_baseline_1e-2"] = _two_view(np.random.default_rng(107), n, K, R, (1e-2, 0.0, 0.0), (3, 10),
                                            (640, 480))
    sets["short_baseline_1e-3_noise"] = _two_view(np.random.default_rng(108), n, K, R, (1e-3, 0.0, 0.0), (3, 10),
                                                  (640, 480), noise=0.1)
    sets["far"] = _two_view(np.random.default_rng(109), n, K, R, (0.5, 0.0, 0.0), (1e3, 1e5), (640, 480))
    # tiny parallax: R = I, camera 2 moved 0.5 sideways, the second pixel 2e-5 .. 4e-4 px left of the
    # first (depths 2e5 .. 4.5e6): the float w of the solution straddles FLT_EPSILON
    rng = np.random.default_rng(110)
    s = _two_view(rng, n, K, np.eye(3), (0.5, 0.0, 0.0), (3, 10), (640, 480))
    # (half of the shifts in the lowest octave, where the threshold lies)
    shift = np.exp(np.r_[rng.uniform(np.log(2e-5), np.log(4e-5), n // 2),
                         rng.uniform(np.log(2e-5), np.log(4e-4), n - n // 2)])
    s["uv2"] = s["uv1"].copy()
    s["uv2"][:, 0] = (s["uv1"][:, 0].astype(np.float64) - shift).astype(np.float32)
    del s["X"]
    sets["tiny_parallax"] = s
    # points at infinity: the same pair, uv2 == uv1 bit for bit
    s = _two_view(np.random.default_rng(111), n, K, np.eye(3), (0.5, 0.0, 0.0), (3, 10), (640, 480))
    s["uv2"] = s["uv1"].copy()
    del s["X"]
    sets["infinity"] = s
    g = np.load(GOLDEN)
    sets["golden"] = {"P1": g["tri/P1"].reshape(3, 4).astype(np.float32),
                      "P2": g["tri/P2"].reshape(3, 4).astype(np.float32),
                      "uv1": g["tri/uv1"].reshape(-1, 2).astype(np.float32),
                      "uv2": g["tri/uv2"].reshape(-1, 2).astype(np.float32), "K": None}
    return sets


def infinity_directions(s):
    """Unit back-projections K^-1 (u, v, 1) of a set's first-view pixels (float64)."""
    K = s["K"]
    uv = s["uv1"].astype(np.float64)
    d = np.c_[(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(uv))]
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def check_infinity(s, got, who):
    """(c): each result is a unit vector equal to +- the back-projection to 4 EPS32."""
    d = infinity_directions(s)
    got = np.asarray(got, np.float64)
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= DIRECT_C * EPS32, who
    err = np.minimum(np.abs(got - d).max(1), np.abs(got + d).max(1))
    assert err.max() <= DIRECT_C * EPS32, (who, err.max() / EPS32)
    return float(err.max() / EPS32)
