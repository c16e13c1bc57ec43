"""Numpy restatement of the point refiner's semantics (include/picp_c.h picp_refine_*): the oracle
of tests/test_refine_cpu.py and tests/test_gpu_refine.py.

refine(..., dtype=np.float64) is the oracle.  dtype=np.float32 runs the same statements with every
operation rounded to float32 and every sum taken sequentially in track order; the distance between
the two results is the D the GPU tolerance is derived from (4 D, see test_gpu_refine.py).

Everything is vectorised over the observations of all points; the per-point sums loop over the
position inside the track, so a point's terms are added one at a time, in track order.
"""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)


def linearize_obs(K, rows, cols, R, t, X, uv, dt=np.float64):
    """Per observation: R (n, 3, 3), t (n, 3) world-in-camera, X (n, 3) the observed point, uv (n, 2).
    Returns dict(valid, e (n, 2), J (n, 2, 3), chi, proj (n, 2), pcz) in dtype dt, in the solver's
    operation order (projectPoint's rules: pc.z <= 0 rejects, then the image bounds)."""
    K = np.asarray(K, dt)
    R = np.asarray(R, dt)
    t = np.asarray(t, dt)
    X = np.asarray(X, dt)
    uv = np.asarray(uv, dt)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(all="ignore"):
        pc = [((R[:, i, 0] * x + R[:, i, 1] * y) + R[:, i, 2] * z) + t[:, i] for i in range(3)]
        ph = [(K[i, 0] * pc[0] + K[i, 1] * pc[1]) + K[i, 2] * pc[2] for i in range(3)]
        iz = dt(1.0) / ph[2]
        ix, iy = ph[0] * iz, ph[1] * iz
        valid = ~(pc[2] <= 0) & ~((ix < 0) | (ix > dt(cols - 1)) | (iy < 0) | (iy > dt(rows - 1)))
        e = np.stack([ix - uv[:, 0], iy - uv[:, 1]], 1)
        chi = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        # J = Jp K R, Jp = [iz 0 -ph0 iz^2; 0 iz -ph1 iz^2]
        iz2 = iz * iz
        jp = [-(ph[0] * iz2), -(ph[1] * iz2)]
        A = [[iz * K[r, c] + jp[r] * K[2, c] for c in range(3)] for r in range(2)]
        J = np.stack([np.stack([(A[r][0] * R[:, 0, c] + A[r][1] * R[:, 1, c]) + A[r][2] * R[:, 2, c]
                                for c in range(3)], 1) for r in range(2)], 1)
    assert J.dtype == dt and chi.dtype == dt
    return {"valid": valid, "e": e, "J": J, "chi": chi, "proj": np.stack([ix, iy], 1), "pcz": pc[2]}


def _ldl3(H, b, dt):
    """H (n, 6) upper triangle row-major (00 01 02 11 12 22), damped; solves H dx = -b by LDL^T
    without pivoting.  Returns dx (n, 3) and ok (positive definite and dx finite)."""
    with np.errstate(all="ignore"):
        d0 = H[:, 0]
        i0 = dt(1.0) / d0
        l10, l20 = H[:, 1] * i0, H[:, 2] * i0
        d1 = H[:, 3] - l10 * H[:, 1]
        i1 = dt(1.0) / d1
        l21 = (H[:, 4] - l20 * H[:, 1]) * i1
        d2 = H[:, 5] - l20 * H[:, 2] - l21 * (l21 * d1)
        i2 = dt(1.0) / d2
        y0 = -b[:, 0]
        y1 = -b[:, 1] - l10 * y0
        y2 = -b[:, 2] - l20 * y0 - l21 * y1
        x2 = y2 * i2
        x1 = y1 * i1 - l21 * x2
        x0 = y0 * i0 - l10 * x1 - l20 * x2
        dx = np.stack([x0, x1, x2], 1)
        ok = (d0 > 0) & (d1 > 0) & (d2 > 0) & np.isfinite(dx).all(1)
    return dx, ok


def refine(K, rows, cols, poses, track_off, obs_pose, obs_uv, xyz, threshold=3000.0, damping=1.0,
           min_inliers=2, keep_outliers=False, max_rounds=10, conv_eps=1e-5, dtype=np.float64):
    """-> (xyz (n, 3) in dtype, stats dict of arrays, borderline (n,) bool).

    borderline[i]: in some round one of point i's observations had |chi - threshold| <= 1e-3
    threshold, a projection within 1e-3 px of an image bound, or |pc.z| < 1e-6: a gate decision
    that may legitimately flip in float32."""
    dt = dtype
    poses = np.asarray(poses, np.float32).reshape(-1, 4, 4)
    off = np.asarray(track_off, np.int64)
    obs_pose = np.asarray(obs_pose, np.int64).reshape(-1)
    obs_uv = np.asarray(obs_uv, np.float32).reshape(-1, 2)
    n = len(off) - 1
    lens = np.diff(off)
    owner = np.repeat(np.arange(n), lens)
    X = np.array(xyz, dt).reshape(n, 3)
    K = np.asarray(K, np.float32)
    R = poses[obs_pose][:, :3, :3] if len(obs_pose) else np.zeros((0, 3, 3), np.float32)
    t = poses[obs_pose][:, :3, 3] if len(obs_pose) else np.zeros((0, 3), np.float32)
    thr = dt(np.float32(threshold))
    eps = dt(np.float32(conv_eps))
    st = {"chi_in": np.zeros(n, dt), "chi_out": np.zeros(n, dt), "n_in": np.zeros(n, np.int32),
          "n_projected": np.zeros(n, np.int32), "ok": np.zeros(n, np.int32), "rounds": np.zeros(n, np.int32),
          "converged": np.zeros(n, np.int32)}
    border = np.zeros(n, bool)
    active = np.ones(n, bool)
    prev = np.full(n, FLT_MAX, dt)
    maxlen = int(lens.max()) if n else 0
    for _ in range(int(max_rounds)):
        if not active.any():
            break
        L = linearize_obs(K, rows, cols, R, t, X[owner], obs_uv, dt)
        valid, chi, e, J = L["valid"], L["chi"], L["e"], L["J"]
        with np.errstate(all="ignore"):
            outl = valid & (chi > thr)  # strict gate
            inl = valid & ~outl
            use = inl | (valid & bool(keep_outliers))
            lam = np.where(outl, np.sqrt(thr / chi), dt(1.0)).astype(dt)
            # borderline decisions of this round
            px, py = L["proj"][:, 0], L["proj"][:, 1]
            near = (valid & (np.abs(chi - thr) <= dt(1e-3) * thr)) | (np.abs(L["pcz"]) < 1e-6)
            infront = L["pcz"] > 0
            for v, hi in ((px, cols - 1), (py, rows - 1)):
                near |= infront & ((np.abs(v) <= 1e-3) | (np.abs(v - hi) <= 1e-3))
        border |= np.bincount(owner[near & active[owner]], minlength=n) > 0
        # per-observation terms (zero where unused), then the sequential per-point sums
        w = np.where(use, lam, dt(0.0)).astype(dt)
        Jz = np.where(use[:, None, None], J, dt(0.0))
        ez = np.where(use[:, None], e, dt(0.0))
        terms = np.zeros((len(owner), 11), dt)
        k = 0
        for a in range(3):
            for b in range(a, 3):
                terms[:, k] = (w * Jz[:, 0, a]) * Jz[:, 0, b] + (w * Jz[:, 1, a]) * Jz[:, 1, b]
                k += 1
        for a in range(3):
            terms[:, 6 + a] = (w * Jz[:, 0, a]) * ez[:, 0] + (w * Jz[:, 1, a]) * ez[:, 1]
        terms[:, 9] = np.where(inl, chi, dt(0.0))
        terms[:, 10] = np.where(outl, chi, dt(0.0))
        acc = np.zeros((n, 11), dt)
        n_in = np.zeros(n, np.int32)
        n_proj = np.zeros(n, np.int32)
        for j in range(maxlen):
            pts = np.nonzero(lens > j)[0]
            idx = off[pts] + j
            acc[pts] = acc[pts] + terms[idx]
            n_in[pts] += inl[idx]
            n_proj[pts] += valid[idx]
        assert acc.dtype == dt
        # record: the stats of this linearisation, before the update
        for key, val in (("chi_in", acc[:, 9]), ("chi_out", acc[:, 10]), ("n_in", n_in), ("n_projected", n_proj)):
            st[key][active] = val[active]
        few = active & (n_in < int(min_inliers))
        st["ok"][few] = 0
        active = active & ~few
        H = acc[:, [0, 1, 2, 3, 4, 5]].copy()
        H[:, [0, 3, 5]] = H[:, [0, 3, 5]] + dt(np.float32(damping))
        dx, ok = _ldl3(H, acc[:, 6:9], dt)
        bad = active & ~ok
        st["ok"][bad] = 0
        active = active & ok
        X[active] = X[active] + dx[active]
        st["ok"][active] = 1
        st["rounds"][active] += 1
        cur = acc[:, 9]
        with np.errstate(all="ignore"):
            rel = np.where(prev > dt(1e-10), np.abs(prev - cur) / prev, dt(0.0))
        conv = active & (rel < eps)
        st["converged"][conv] = 1
        upd = active & ~conv
        prev[upd] = cur[upd]
        active = upd
    return X, st, border


# ------------------------------------------------------------------------------------------------
# the cases the CPU and GPU tests share
# ------------------------------------------------------------------------------------------------
TRACK_LENGTHS = (0, 1, 2, 15, 16, 17, 33, 100)  # mixed inside every wave of the synthetic cases


def data_case(vo, outlier_frac=0.0):
    """The known-answer inputs on the dataset: tracks with at least 6 observations, ground-truth
    poses, start = world.dat + N(0, 0.05 m) (seed 1); outlier_frac of the observations replaced
    by uniform pixels (seed 2)."""
    rows_kept, off, obs_pose, obs_uv = vo.tracks(min_obs=6)
    poses = np.stack([vo.T_wc(k) for k in range(vo.n_frames)]).astype(np.float32)
    truth = vo.world_xyz[rows_kept].astype(np.float32)
    start = (truth + np.random.default_rng(1).normal(0.0, 0.05, truth.shape)).astype(np.float32)
    uv = obs_uv.copy()
    if outlier_frac > 0:
        rng = np.random.default_rng(2)
        bad = rng.random(len(uv)) < outlier_frac
        uv[bad] = np.stack([rng.uniform(0, vo.cols - 1, bad.sum()), rng.uniform(0, vo.rows - 1, bad.sum())], 1)
    return {"K": vo.K.astype(np.float32), "rows": vo.rows, "cols": vo.cols, "poses": poses, "off": off,
            "obs_pose": obs_pose, "obs_uv": uv.astype(np.float32), "start": start, "truth": truth}


def synth_poses(n_poses):
    """A planar trajectory (picp_amd.synth.MOUNT): the robot drifts sideways and forward while its
    heading swings by +-69 degrees, so far-apart poses look in different directions."""
    from picp_amd import synth
    step = 0.02 if n_poses > 2 else 0.4
    out = []
    for k in range(n_poses):
        th = 1.2 * np.sin(2.0 * np.pi * k / 120.0)
        out.append(synth.world_in_camera((0.004 * k, step * k, th)))
    return np.stack(out).astype(np.float32)


def synth_case(n_points, n_poses, seed, K, rows=480, cols=640, pixel_noise=0.5, outlier_frac=0.1):
    """Synthetic tracks: lengths from TRACK_LENGTHS (longest first) in a shuffled cycle, depths 0.6 to 5 m in the
    track's middle camera, pixel noise 0.5 px, at least 2 degrees of parallax where the track has
    two poses to choose, every 37th point behind its cameras, 10 % uniform-pixel outliers.  Poses
    far from the middle one see the point outside the image or behind them."""
    rng = np.random.default_rng(seed)
    poses = synth_poses(n_poses)
    K64 = np.asarray(K, np.float64)
    Kinv = np.linalg.inv(K64)
    lens = np.array([TRACK_LENGTHS[::-1][i % len(TRACK_LENGTHS)] for i in range(n_points)], np.int64)
    for s in range(0, n_points, 8):  # shuffled inside every group of 8: all lengths in every wave
        rng.shuffle(lens[s:s + 8])
    off = np.zeros(n_points + 1, np.int64)
    off[1:] = np.cumsum(lens)
    obs_pose = np.zeros(off[-1], np.int32)
    obs_uv = np.zeros((off[-1], 2), np.float32)
    truth = np.zeros((n_points, 3), np.float32)
    for i in range(n_points):
        L = int(lens[i])
        if n_poses >= 121 and 2 <= L <= n_poses:
            while True:
                c = int(rng.integers(0, n_poses))
                lo = 0 if L > 60 else min(max(0, c - 30), n_poses - 61)  # a 61-pose window
                hi = n_poses if L > 60 else lo + 61
                idx = np.sort(rng.choice(np.arange(lo, hi), L, replace=False))
                if idx[-1] - idx[0] >= 20:  # 0.4 m of baseline: more than 2 degrees up to 5 m
                    break
        else:
            idx = np.arange(L) % n_poses
        mid = int(idx[len(idx) // 2]) if L else 0
        d = rng.uniform(0.6, 5.0) * (-1.0 if i % 37 == 36 else 1.0)
        pix = np.array([rng.uniform(100, cols - 100), rng.uniform(100, rows - 100), 1.0])
        Xc = d * (Kinv @ pix)
        T_cw = np.linalg.inv(poses[mid].astype(np.float64))
        Xw = T_cw[:3, :3] @ Xc + T_cw[:3, 3]
        truth[i] = Xw
        for j, k in enumerate(idx):
            T = poses[k].astype(np.float64)
            pc = T[:3, :3] @ Xw + T[:3, 3]
            if pc[2] > 1e-3 and rng.random() >= outlier_frac:
                ph = K64 @ pc
                z = ph[:2] / ph[2] + rng.normal(0.0, pixel_noise, 2)
            else:
                z = np.array([rng.uniform(0, cols - 1), rng.uniform(0, rows - 1)])
            obs_pose[off[i] + j] = k
            obs_uv[off[i] + j] = np.clip(z, -1e4, 1e4)
    start = (truth + rng.normal(0.0, 0.05, truth.shape)).astype(np.float32)
    return {"K": np.asarray(K, np.float32), "rows": rows, "cols": cols, "poses": poses, "off": off,
            "obs_pose": obs_pose, "obs_uv": obs_uv, "start": start, "truth": truth}


def run_case(case, dtype=np.float64, **params):
    return refine(case["K"], case["rows"], case["cols"], case["poses"], case["off"], case["obs_pose"],
                  case["obs_uv"], case["start"], dtype=dtype, **params)


def measure_d(case, **params):
    """D of a case: max |X_f32 - X_f64| over the points that are not borderline; also the
    borderline mask (of the float64 run) and the float64 result."""
    X64, st, border = run_case(case, np.float64, **params)
    X32, _, _ = run_case(case, np.float32, **params)
    diff = np.abs(X32.astype(np.float64) - X64).max(1) if len(X64) else np.zeros(0)
    keep = ~border
    return (float(diff[keep].max()) if keep.any() else 0.0), border, X64, st


# ------------------------------------------------------------------------------------------------
# the named cases: inputs, parameters and the float64 reference, computed once per process
# ------------------------------------------------------------------------------------------------
BASE = dict(threshold=3000.0, damping=1.0, min_inliers=2, keep_outliers=0, max_rounds=10, conv_eps=-1.0)
N_POINTS = (0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 4099)
SHAPES = [(n, 121) for n in N_POINTS] + [(65, 1), (65, 2), (257, 2)]
# seeds for which the oracle keeps at most 1 % of a case's points borderline (checked in
# tests/test_refine_cpu.py); 11 is the first seed tried
SEEDS = {s: 11 for s in SHAPES}
SEEDS[(17, 121)] = 12
# parameter variants, all on the 257-point, 121-pose synthetic case
VARIANTS = {"keep": dict(keep_outliers=1), "damp0": dict(damping=0.0), "rounds1": dict(max_rounds=1),
            "rounds5": dict(max_rounds=5), "conv": dict(conv_eps=1e-5)}
NAMES = (["data_clean", "data_outliers"] + ["synth_%d_%d" % s for s in SHAPES] + sorted(VARIANTS))

_cache = {}


def _vo():
    from picp_amd.vo_data import VOData
    if "vo" not in _cache:
        _cache["vo"] = VOData()
    return _cache["vo"]


def named_case(name):
    """-> (case, params) of a name in NAMES."""
    key = ("case", name)
    if key not in _cache:
        vo = _vo()
        if name.startswith("data_"):
            _cache[key] = (data_case(vo, 0.2 if name == "data_outliers" else 0.0), dict(BASE))
        elif name.startswith("synth_"):
            n, npz = (int(v) for v in name.split("_")[1:])
            _cache[key] = (synth_case(n, npz, SEEDS[(n, npz)], vo.K), dict(BASE))
        else:
            _cache[key] = (named_case("synth_257_121")[0], {**BASE, **VARIANTS[name]})
    return _cache[key]


def reference(name):
    """-> (case, params, X64, stats, borderline): the float64 oracle of a named case.  For "conv"
    the reference is the FIXED-round result (convergence disabled): the converged run must land
    within the tolerance of it."""
    key = ("ref", name)
    if key not in _cache:
        case, params = named_case(name)
        ref_params = {**params, "conv_eps": -1.0}
        X, st, border = run_case(case, np.float64, **ref_params)
        _cache[key] = (case, params, X, st, border)
    return _cache[key]


def measured_d(name):
    """D of a named case: max |X_f32 - X_f64| over its non-borderline points, X_f32 the float32
    restatement with the case's parameters, X_f64 the reference above."""
    case, params, X64, _, border = reference(name)
    X32, _, _ = run_case(case, np.float32, **params)
    keep = ~border
    if not keep.any():
        return 0.0
    return float(np.abs(X32.astype(np.float64) - X64)[keep].max())
