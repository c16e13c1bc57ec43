"""Reference of the alternating pose / point adjustment (include/picp_c.h picp_refine_run_poses,
picp_refine_adjust): the pose-major view of the tracks in numpy, and the alternation as
refine_oracle.refine (point step) followed, per movable pose, by the CPU oracle's solve (pose step).

Two arithmetic classes: "f64" = refine in float64 and oracle.solve in MODE_F64, the reference;
"f32" = refine in float32 and MODE_FAITHFUL.  The distance between the two runs gives the D_X
(points) and D_T (pose entries) the GPU tolerance is derived from, as in test_gpu_refine.py.  The
points are rounded to float32 between the steps in both classes, as the kernel stores them.

The half-step figures are those of the library's sweep records: the sums of the step's own
per-item stats (chi_in, n_in, ok), i.e. of every item's last linearisation.
"""
import numpy as np

import refine_oracle as RO

# the parameters of the shared cases: both steps gate at 3000, fixed round counts (a convergence
# stop may legitimately fall one round apart in float32 and float64)
POINTS = dict(threshold=3000.0, damping=1.0, min_inliers=2, keep_outliers=0, max_rounds=10, conv_eps=-1.0)
POSES = dict(threshold=3000.0, damping=1.0, min_inliers=0, keep_outliers=0, max_rounds=10, conv_eps=-1.0)
PERTURB_SEED = 5
SYNTH_SEED = 11


def pose_view(n_poses, track_off, obs_pose, obs_uv):
    """-> (pose_off (n_poses+1,) int64, obs_point int32, obs_uv float32 (n, 2)): pose k's entries in
    ascending position of the point-major arrays (a stable sort of the positions by pose)."""
    off = np.asarray(track_off, np.int64)
    obs_pose = np.asarray(obs_pose, np.int64).reshape(-1)
    uv = np.asarray(obs_uv, np.float32).reshape(-1, 2)
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.argsort(obs_pose, kind="stable")
    pose_off = np.zeros(n_poses + 1, np.int64)
    pose_off[1:] = np.cumsum(np.bincount(obs_pose, minlength=n_poses))
    return pose_off, owner[order].astype(np.int32), uv[order]


def movable_poses(case):
    """Ascending indices of the poses a pose step solves: not fixed, list not empty."""
    pose_off, _, _ = pose_view(len(case["poses"]), case["off"], case["obs_pose"], case["obs_uv"])
    fixed = np.asarray(case.get("fixed", np.zeros(len(case["poses"]), bool)), bool)
    return np.nonzero(~fixed & (np.diff(pose_off) > 0))[0]


def pose_step(oracle, case, poses, X32, mode, **prm):
    """One pose step at the float32 points X32 -> (poses (n, 4, 4) float32, stats dict of arrays)."""
    n = len(poses)
    pose_off, pt, uv = pose_view(n, case["off"], case["obs_pose"], case["obs_uv"])
    out = np.array(poses, np.float32)
    st = {"chi_in": np.zeros(n), "n_in": np.zeros(n, np.int64), "ok": np.zeros(n, np.int64),
          "rounds": np.zeros(n, np.int64)}
    for k in movable_poses(case):
        q = slice(pose_off[k], pose_off[k + 1])
        m = pose_off[k + 1] - pose_off[k]
        pairs = np.stack([np.arange(m), np.arange(m)], 1).astype(np.int32)
        T, s = oracle.solve(poses[k], case["K"], case["rows"], case["cols"], X32[pt[q]], uv[q], pairs,
                            prm["threshold"], damping=prm["damping"], min_inliers=prm["min_inliers"],
                            keep_outliers=bool(prm["keep_outliers"]), mode=mode, max_rounds=prm["max_rounds"],
                            conv_eps=prm["conv_eps"])
        if np.isfinite(T).all():
            out[k] = T
        for f in st:
            st[f][k] = s[f]
    return out, st


def alternate(oracle, case, sweeps, cls="f64", points=None, poses=None):
    """-> list, one entry per sweep: dict(X (n, 3) float32, poses (m, 4, 4) float32, border (n,) bool of
    this sweep's point step, pt = the point step's stats, ps = the pose step's stats)."""
    dt, mode = (np.float64, oracle.MODE_F64) if cls == "f64" else (np.float32, oracle.MODE_FAITHFUL)
    points = {**POINTS, **(points or {})}
    poses_prm = {**POSES, **(poses or {})}
    X = np.asarray(case["start"], np.float32)
    T = np.asarray(case["poses"], np.float32)
    out = []
    for _ in range(sweeps):
        Xn, pt, border = RO.refine(case["K"], case["rows"], case["cols"], T, case["off"], case["obs_pose"],
                                   case["obs_uv"], X, dtype=dt, **points)
        X = Xn.astype(np.float32)
        T, ps = pose_step(oracle, case, T, X, mode, **poses_prm)
        out.append({"X": X, "poses": T, "border": border, "pt": pt, "ps": ps})
    return out


def total_chi_in(case, poses, X, threshold=POINTS["threshold"]):
    """-> (chi, n): the inlier chi2 summed over ALL observations of the case at a state (float32
    poses and points, float64 arithmetic), and the inliers.  One set of observations for both kinds
    of step, unlike the steps' own stats: the point stats include the fixed poses' observations, the
    pose stats do not, and each holds its items' LAST linearisation, one update before the state."""
    owner = np.repeat(np.arange(len(case["off"]) - 1), np.diff(case["off"]))
    P = np.asarray(poses, np.float32)[np.asarray(case["obs_pose"], np.int64)]
    L = RO.linearize_obs(case["K"], case["rows"], case["cols"], P[:, :3, :3], P[:, :3, 3],
                         np.asarray(X, np.float32)[owner], case["obs_uv"])
    inl = L["valid"] & ~(L["chi"] > threshold)
    return float(L["chi"][inl].sum()), int(inl.sum())


def half_steps(case, run):
    """total_chi_in at the start and after every half-step of a run of alternate(), in order."""
    out = [total_chi_in(case, case["poses"], case["start"])[0]]
    T = case["poses"]
    for s in run:
        out += [total_chi_in(case, T, s["X"])[0], total_chi_in(case, s["poses"], s["X"])[0]]
        T = s["poses"]
    return out


def record_sums(run):
    """Per sweep the sums the library's sweep records hold: the steps' own per-item stats."""
    return [{"chi_in_points": float(np.sum(s["pt"]["chi_in"], dtype=np.float64)),
             "chi_in_poses": float(np.sum(s["ps"]["chi_in"], dtype=np.float64)),
             "n_in_points": int(s["pt"]["n_in"].sum()), "n_in_poses": int(s["ps"]["n_in"].sum()),
             "ok_points": int(s["pt"]["ok"].sum()), "ok_poses": int(s["ps"]["ok"].sum())} for s in run]


def distances(run32, run64):
    """Per sweep (D_X, D_T): max |X_f32 - X_f64| over the points not borderline in any point step of
    the float64 run so far, and max |T_f32 - T_f64| over the pose entries."""
    out = []
    border = np.zeros(len(run64[0]["X"]), bool)
    for a, b in zip(run32, run64):
        border = border | b["border"]
        keep = ~border
        dx = np.abs(a["X"].astype(np.float64) - b["X"].astype(np.float64)).max(1)
        out.append((float(dx[keep].max()) if keep.any() else 0.0,
                    float(np.abs(a["poses"].astype(np.float64) - b["poses"].astype(np.float64)).max())))
    return out


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
def perturb_poses(oracle, poses, seed=PERTURB_SEED):
    """Poses 1.. moved by N(0, 2 cm) and N(0, 0.01 rad) (v2t_euler(d) @ T); pose 0 stays."""
    rng = np.random.default_rng(seed)
    out = np.array(poses, np.float32)
    d = rng.normal(0.0, 1.0, (len(poses) - 1, 6)) * np.array([0.02] * 3 + [0.01] * 3)
    for k in range(1, len(poses)):
        out[k] = (oracle.v2t_euler(d[k - 1].astype(np.float32)).astype(np.float64) @ poses[k].astype(np.float64))
    return out


def _fixed0(n):
    f = np.zeros(n, bool)
    f[0] = True
    return f


def two_long_case(n, K, rows=480, cols=640, seed=3):
    """2 poses 0.4 m apart and n points seen by both (track = pose 0, pose 1), 0.5 px of noise; the
    poses are both movable and start 1 cm / 0.005 rad off."""
    rng = np.random.default_rng(seed)
    poses = RO.synth_poses(2)
    K64 = np.asarray(K, np.float64)
    Kinv = np.linalg.inv(K64)
    T0inv = np.linalg.inv(poses[0].astype(np.float64))
    pts, uvs = [], []
    while len(pts) < n:
        pix = np.array([rng.uniform(60, cols - 60), rng.uniform(60, rows - 60), 1.0])
        Xw = T0inv[:3, :3] @ (rng.uniform(1.5, 6.0) * (Kinv @ pix)) + T0inv[:3, 3]
        z = []
        for T in poses.astype(np.float64):
            pc = T[:3, :3] @ Xw + T[:3, 3]
            ph = K64 @ pc
            z.append(ph[:2] / ph[2] + rng.normal(0.0, 0.5, 2) if pc[2] > 0.1 else np.array([-1.0, -1.0]))
        z = np.array(z)
        if (z[:, 0] > 5).all() and (z[:, 0] < cols - 6).all() and (z[:, 1] > 5).all() and (z[:, 1] < rows - 6).all():
            pts.append(Xw)
            uvs.append(z)
    truth = np.array(pts, np.float32).reshape(n, 3)
    off = 2 * np.arange(n + 1, dtype=np.int64)
    obs_pose = np.tile(np.array([0, 1], np.int32), n)
    start = (truth + rng.normal(0.0, 0.02, truth.shape)).astype(np.float32)
    return {"K": np.asarray(K, np.float32), "rows": rows, "cols": cols, "poses": poses, "off": off,
            "obs_pose": obs_pose, "obs_uv": np.array(uvs, np.float32).reshape(2 * n, 2), "start": start,
            "truth": truth, "fixed": np.zeros(2, bool)}


def tiny_case(K, rows=480, cols=640):
    """3 points and 3 poses: pose 2 is in no track, point 1 has an empty track, point 2 is seen twice
    by pose 0."""
    C = two_long_case(3, K, rows, cols, seed=4)
    uv = C["obs_uv"].reshape(3, 2, 2)
    off = np.array([0, 2, 2, 5], np.int64)
    obs_pose = np.array([0, 1, 0, 1, 0], np.int32)
    obs_uv = np.concatenate([uv[0], uv[2], uv[2][:1] + np.float32(0.25)]).astype(np.float32)
    poses = np.concatenate([C["poses"], C["poses"][1:]])
    return {**C, "poses": poses, "off": off, "obs_pose": obs_pose, "obs_uv": obs_uv, "fixed": np.zeros(3, bool)}


def many_poses_case(n, K, rows=480, cols=640, seed=8):
    """n identity poses (the view build does not read them) and n // 2 + 2 points: point i is tracked
    by poses i and (7 i + 3) mod n and, every 64th point, by pose n - 1.  The poses from 0 up to the
    number of points are a run of non-empty lists (past one scan chunk of 1,024 poses for n = 2049),
    the rest are hit or not by the second rule, and the last pose's list is long."""
    m = n // 2 + 2
    rng = np.random.default_rng(seed)
    tracks = [[i, (7 * i + 3) % n] + ([n - 1] if i % 64 == 0 else []) for i in range(m)]
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([len(t) for t in tracks])
    obs_pose = np.concatenate(tracks).astype(np.int32)
    obs_uv = rng.uniform(5.0, min(rows, cols) - 6.0, (len(obs_pose), 2)).astype(np.float32)
    lens = np.bincount(obs_pose, minlength=n)
    assert (lens == 0).any() and lens[n - 1] > 8 and (lens[:m] > 0).all(), (n, lens.max())
    return {"K": np.asarray(K, np.float32), "rows": rows, "cols": cols,
            "poses": np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)), "off": off, "obs_pose": obs_pose,
            "obs_uv": obs_uv, "start": np.zeros((m, 3), np.float32), "fixed": np.zeros(n, bool)}


_cache = {}


def case(oracle, name):
    """data_perturbed | synth | two_long_<n> | tiny | many_poses_<n>"""
    if name in _cache:
        return _cache[name]
    K = RO._vo().K
    if name == "data_perturbed":
        C = dict(RO.data_case(RO._vo()))
        C["truth_poses"] = C["poses"]
        C["poses"] = perturb_poses(oracle, C["poses"])
        C["fixed"] = _fixed0(len(C["poses"]))
    elif name == "synth":
        C = dict(RO.synth_case(257, 121, SYNTH_SEED, K))
        C["truth_poses"] = C["poses"]
        C["poses"] = perturb_poses(oracle, C["poses"])
        C["fixed"] = _fixed0(len(C["poses"]))
    elif name.startswith("two_long_"):
        C = two_long_case(int(name.split("_")[2]), K)
        C["truth_poses"] = C["poses"]
        C["poses"] = perturb_poses(oracle, C["poses"], seed=6)
        d = np.array([0.01, -0.01, 0.005, 0.003, -0.002, 0.004], np.float32)
        C["poses"][0] = oracle.v2t_euler(d).astype(np.float64) @ C["truth_poses"][0].astype(np.float64)
    elif name == "tiny":
        C = tiny_case(K)
    elif name.startswith("many_poses_"):
        C = many_poses_case(int(name.split("_")[2]), K)
    else:
        raise KeyError(name)
    _cache[name] = C
    return C


def reference(oracle, name, sweeps, cls="f64"):
    """alternate() of a named case, computed once per process (a shorter run is a prefix of a longer)."""
    key = ("run", name, cls)
    if key not in _cache or len(_cache[key]) < sweeps:
        _cache[key] = alternate(oracle, case(oracle, name), sweeps, cls)
    return _cache[key][:sweeps]
