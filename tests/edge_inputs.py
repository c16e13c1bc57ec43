"""Extreme and NaN correspondences for the solve, classify and refine kernels (CPU only).

A problem is ordinary items sampled in the camera frame of a pose T0 (depth 1.5-9 m, inside the
image, 0.5 px noise, 20 % outliers) with a few *slots* spread through the index range.  In the
clean variant every slot holds an ordinary point 4-5 m behind the camera (skipped), in the
"clean_out" variant an ordinary projectable outlier (skipped with keep_outliers = 0); in an edge
variant the slots hold the items of one family, cycling through the family's list.

Two bases:

  * "depth": T0 is a signed permutation with a (minus) zero translation, so R p + t is exact in
    float32 and an item lands on its intended camera-frame depth bit for bit (depth_f32 restates
    the kernels' item_depth and make() asserts the bits).  With any translation along the optical
    axis the tiny depths could not be written at all: 1e-40 - 1.0 rounds to -1.0.  Its families
    are tied to T0: they are linearized at T0 and solved for one round from it.
  * "free": T0 is a general rotation with a short-mantissa translation.  Its families hold
    whatever the pose is (an overflowing coordinate or measurement), so they are also evaluated
    at a second nearby pose, T1, and solved for several rounds from it.

Families (what the oracle makes of them is asserted in test_edge_inputs_cpu.py):

  depth / skip      depth +0, -0, 1e-40 with zero and non-zero x, y; 2^-101, 2^-100, 9e-13, 1e-13
                    with non-zero x, y (the projection overflows the image); 3e38; -3e38;
                    x = +-3e38 at depth 1-5.  All skipped: everything bit-identical to clean.
  depth / out       valid outliers: depth 2^101 inside the image (x = z and x = 0); depth 2^-101,
                    2^-100, 9e-13, 1e-13 ON the optical axis (x = y = 0 projects to the principal
                    point whatever the depth) and 2^-101 (1, 0, 1); measurement (10, 10).
  depth / tiny_in   the same tiny depths measured where they project: valid INLIERS whose J^2
                    overflows float32 in the reference too -- gate only.
  free / skip       world x = +-3e38, y = -3e38, z = -3e38, z = -inf (the camera-frame depth is
                    negative or the projection infinite at any nearby pose).
  free / out        an ordinary projectable point measured at u = 1e20, 3e38, +inf, -inf.
  free / nan        world x = NaN; world z = +inf, x = +inf (a depth of +inf has 1/z = 0 and the
                    projection inf * 0, or K pc is inf - inf); u = NaN, v = NaN on a projectable
                    point.  NaN passes every comparison of the gate: each is an INLIER with NaN chi.
"""
import numpy as np

f32 = np.float32
ROWS, COLS = 480, 640
THR = 3000.0
K_PIN = np.array([[180, 0, 320], [0, 180, 240], [0, 0, 1]], f32)
K_SKEW = np.array([[180, 3.5, 320], [0, 181, 240], [0, 0, 1.0000001]], f32)

# camera = R world: pc0 = -y, pc1 = -z, pc2 = x; -0 translation so that a -0 depth survives the sum
T_PERM = np.array([[0, -1, 0, -0.0], [0, 0, -1, -0.0], [1, 0, 0, -0.0], [0, 0, 0, 1]], f32)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def _pose(R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(f32)


T_FREE = _pose(_rot(0.03, -0.05, 0.02), [0.125, -0.25, 0.5])


def nearby(T, seed):
    """A random pose a few centimetres and about a degree from T."""
    rng = np.random.default_rng(seed)
    D = _pose(_rot(*rng.uniform(-0.02, 0.02, 3)), rng.uniform(-0.04, 0.04, 3)).astype(np.float64)
    return (D @ T.astype(np.float64)).astype(f32)


def depth_f32(T, x, y, z):
    """item_depth of picp_item.h in float32: row 2 of R p + t, left to right, every operation
    rounded on its own (no contraction)."""
    T = np.asarray(T, f32)
    x, y, z = f32(x), f32(y), f32(z)
    with np.errstate(all="ignore"):
        return f32(f32(f32(f32(T[2, 0] * x) + f32(T[2, 1] * y)) + f32(T[2, 2] * z)) + T[2, 3])


def _bits(v):
    return np.asarray(v, f32).reshape(-1).view(np.uint32)


def _cam_perm(c0, c1, c2, u=10.0, v=10.0):
    """World point and measurement of the camera-frame point (c0, c1, c2) under T_PERM, with the
    depth asserted bit for bit."""
    item = np.array([c2, -f32(c0), -f32(c1), u, v], f32)
    assert _bits(depth_f32(T_PERM, *item[:3]))[0] == _bits(c2)[0], (c0, c1, c2)
    return item


NEG0 = f32(-0.0)
TINY = [f32(2.0) ** -101, f32(2.0) ** -100, f32(9e-13), f32(1e-13)]
HUGE = f32(2.0) ** 101


def _families():
    fam = {}
    skip = [_cam_perm(0.0, 0.0, 0.0), _cam_perm(0.0, 0.0, NEG0), _cam_perm(0.0, 0.0, 1e-40),
            _cam_perm(0.7, 0.4, 0.0), _cam_perm(0.7, 0.4, NEG0), _cam_perm(-0.7, 0.4, 1e-40),
            _cam_perm(0.7, -0.4, 1e-40)]
    for d in TINY:
        skip += [_cam_perm(0.7, 0.4, d), _cam_perm(-0.7, -0.4, d)]
    skip += [_cam_perm(1.0, -2.0, 3e38), _cam_perm(1.0, 2.0, -3e38), _cam_perm(3e38, 0.5, 2.0),
             _cam_perm(-3e38, 0.5, 4.5), _cam_perm(0.5, 3e38, 1.0), _cam_perm(0.5, -3e38, 5.0)]
    fam["depth", "skip"] = skip
    out = [_cam_perm(HUGE, 0.0, HUGE), _cam_perm(0.0, 0.0, HUGE)]
    out += [_cam_perm(0.0, 0.0, d) for d in TINY] + [_cam_perm(TINY[0], 0.0, TINY[0])]
    fam["depth", "out"] = out
    fam["depth", "tiny_in"] = ([_cam_perm(0.0, 0.0, d, 320.0, 240.0) for d in TINY] +
                               [_cam_perm(TINY[0], 0.0, TINY[0], 500.0, 240.0)])
    fam["free", "skip"] = [np.array(w + [10.0, 10.0], f32) for w in
                           ([3e38, 0.3, 4.0], [-3e38, 0.3, 4.0], [0.2, -3e38, 4.0], [0.2, 0.3, -3e38],
                            [0.2, 0.3, -np.inf])]
    # an ordinary point near the optical axis of T_FREE, 4 m out: projectable at any nearby pose
    p = (T_FREE[:3, :3].astype(np.float64).T @ (np.array([0.1, -0.1, 4.0]) - T_FREE[:3, 3])).astype(f32)
    fam["free", "out"] = [np.array([*p, u, 200.0], f32) for u in (1e20, 3e38, np.inf, -np.inf)]
    fam["free", "nan"] = [np.array([np.nan, 0.3, 4.0, 10.0, 10.0], f32),
                          np.array([0.2, 0.3, np.inf, 10.0, 10.0], f32),
                          np.array([np.inf, 0.3, 4.0, 10.0, 10.0], f32),
                          np.array([*p, np.nan, 200.0], f32), np.array([*p, 300.0, np.nan], f32)]
    return fam


FAMILIES = _families()
BASE_POSE = {"depth": T_PERM, "free": T_FREE}
# what the float32 gate makes of every item of a family: 0 skipped, 1 inlier, 2 outlier
EXPECTED_STATE = {("depth", "skip"): 0, ("depth", "out"): 2, ("depth", "tiny_in"): 1,
                  ("free", "skip"): 0, ("free", "out"): 2, ("free", "nan"): 1}


def slots(n):
    """Slot positions of a problem of n items: lane 0 and lane 63 of a wave (0, 63; 128, 191),
    the items 5 + {0, 256, 512, 1024} -- slots k and k + 1 of lane 5 whatever the block size of a
    multi-item layout, one (k, k + 1) pair, and each of the last three the lone slot of its wave
    -- about 40 positions spread through the range, and the last item n - 1."""
    fixed = [0, 63, 128, 191, 5, 5 + 256, 5 + 512, 5 + 1024]
    spread = np.unique((np.arange(40) * (n / 40.0) + 0.37 * n / 40.0).astype(np.int64)) if n > 2000 else []
    s = np.unique(np.array([k for k in list(fixed) + list(spread) + [n - 1] if 0 <= k < n], np.int64))
    return s


def _ordinary(rng, T0, n, outlier_frac=0.2, noise=0.5):
    """n ordinary items in the camera frame of T0 -> (n, 5) float32 rows x, y, z, u, v."""
    T = T0.astype(np.float64)
    d = rng.uniform(1.5, 9.0, n)
    px = rng.uniform(20.0, COLS - 21.0, n)
    py = rng.uniform(20.0, ROWS - 21.0, n)
    pc = np.stack([(px - 320.0) / 180.0 * d, (py - 240.0) / 180.0 * d, d], 1)
    w = ((pc - T[:3, 3]) @ T[:3, :3]).astype(f32)  # R^T (pc - t)
    pcw = w.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    uv = np.stack([180.0 * pcw[:, 0] / pcw[:, 2] + 320.0, 180.0 * pcw[:, 1] / pcw[:, 2] + 240.0], 1)
    uv += rng.normal(0.0, noise, uv.shape)
    bad = rng.random(n) < outlier_frac
    uv[bad] = np.stack([rng.uniform(0, COLS - 1, bad.sum()), rng.uniform(0, ROWS - 1, bad.sum())], 1)
    return np.concatenate([w, uv.astype(f32)], 1).astype(f32)


def _behind(rng, T0, m):
    T = T0.astype(np.float64)
    pc = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(-5.0, -4.0, m)], 1)
    w = ((pc - T[:3, 3]) @ T[:3, :3]).astype(f32)
    return np.concatenate([w, np.full((m, 2), 10.0, f32)], 1).astype(f32)


def _central_outliers(rng, T0, m):
    """Ordinary points 3-5 m out that project within 20 px of the principal point (at T0 and at
    any nearby pose), measured at (10, 10): projectable outliers with a finite chi."""
    T = T0.astype(np.float64)
    d = rng.uniform(3.0, 5.0, m)
    pc = np.stack([rng.uniform(-20, 20, m) / 180.0 * d, rng.uniform(-20, 20, m) / 180.0 * d, d], 1)
    w = ((pc - T[:3, 3]) @ T[:3, :3]).astype(f32)
    return np.concatenate([w, np.full((m, 2), 10.0, f32)], 1).astype(f32)


def make(base, n, seed=0, shift=0):
    """One problem of n items on `base` ("depth" / "free").  Returns a dict: T0, T1 (the nearby
    pose), slots, "clean", "clean_out" (the slots hold ordinary projectable outliers instead of
    points behind the camera: with keep_outliers = 0 they are skipped lanes on the iz-only side
    of accumulate_pinhole's zeroing vote, where a point behind the camera takes the all-eight
    side) and one entry per family of the base, each an (n, 5) float32 array of
    x, y, z, u, v rows.  Slot j of family f holds item (j + shift) % len(f) of FAMILIES[base, f]."""
    rng = np.random.default_rng(1000 * seed + n % 997 + (0 if base == "depth" else 500))
    T0 = BASE_POSE[base]
    s = slots(n)
    clean = _ordinary(rng, T0, n)
    clean[s] = _behind(rng, T0, len(s))
    out = {"base": base, "n": n, "T0": T0, "T1": nearby(T0, seed + 7), "slots": s, "clean": clean}
    out["clean_out"] = clean.copy()
    out["clean_out"][s] = _central_outliers(np.random.default_rng(77 + n % 997), T0, len(s))
    for (b, name), items in FAMILIES.items():
        if b != base:
            continue
        v = clean.copy()
        for j, k in enumerate(s):
            v[k] = items[(j + shift) % len(items)]
        if base == "depth":  # every item sits on its intended depth, bit for bit
            for j, k in enumerate(s):
                it = items[(j + shift) % len(items)]
                assert _bits(depth_f32(T0, *v[k, :3]))[0] == _bits(it[0])[0]
        out[name] = v
    return out


def make_batch(base, sizes, seed=0):
    """The frames of a batch: make() per frame (its own seed and shift, so the last item of one
    frame and the first of the next are both slots holding different items), concatenated.
    Returns dict(sizes, frames (the per-frame problems), and per variant the packed (N, 5) rows)."""
    frames = [make(base, int(n), seed=seed + 31 * i, shift=3 * i) for i, n in enumerate(sizes) if n > 0]
    it = iter(frames)
    frames = [next(it) if n > 0 else None for n in sizes]
    out = {"sizes": list(sizes), "frames": frames}
    names = ["clean", "clean_out"] + [name for (b, name) in FAMILIES if b == base]
    for name in names:
        rows = [fr[name] for fr in frames if fr is not None]
        out[name] = np.concatenate(rows) if rows else np.zeros((0, 5), f32)
    return out


def soa(rows):
    return tuple(np.ascontiguousarray(rows[:, i]) for i in range(5))


# ------------------------------------------------------------------------------------------------
# the point refiner
# ------------------------------------------------------------------------------------------------
REFINE_TIED = {"rounds": 1, "depths": (f32(0.0), NEG0, f32(1e-40))}


def _flip(T):
    """The pose looking the other way: every point in front of T is behind it."""
    return (np.diag([-1.0, 1.0, -1.0, 1.0]) @ T.astype(np.float64)).astype(f32)


def refine_case(seed=11):
    """A small refiner case of its own, from the construction of refine_oracle's synth_65_121.

    Six ordinary points with long tracks host replaced observations, at the track positions 0, 15,
    16 and the last (lane 0 and lane 15 of the point's 16-lane row, its second pass, the tail).  In
    the clean variant these observations come from a pose that looks away from the point (skipped
    in every round).  The edge variants point them at another pose:

      "tied"  hosts 0-2: a signed-permutation pose under which the START point has the depth +0, -0,
              1e-40 bit for bit (the host's x coordinate is moved to 0 by a shift of its own copy
              of the world -- points are refined independently -- and its start's x set to the
              depth).  Holds for the first round only.
      "free"  hosts 3-5: a pose whose translation puts every point at the depth 3e38; and two further
              points START at x = 3e38 and y = -3e38 (all their observations skipped: ok = 0, the
              point unchanged).  Holds in every round.
      "nan"   one further point starts at x = NaN.

    Returns dict(clean, tied, free, nan -> case dicts for refine_oracle.run_case, hosts,
    moved (the points whose own start a variant replaces))."""
    import refine_oracle as RO
    case = RO.synth_case(65, 121, seed, K_PIN)
    off, lens = case["off"], np.diff(case["off"])
    start = case["start"].copy()
    poses = [T for T in case["poses"]]
    obs_pose = case["obs_pose"].copy()
    obs_uv = case["obs_uv"].copy()
    ordinary = [i for i in range(65) if i % 37 != 36]
    hosts = [i for i in ordinary if lens[i] >= 17][:6]
    others = [i for i in ordinary if i not in hosts and lens[i] >= 2][:3]
    assert len(hosts) == 6 and len(others) == 3
    # hosts 0-2 get their own copy of the world, shifted along x so that the start's x is 0
    for h, d in zip(hosts[:3], REFINE_TIED["depths"]):
        sx = float(start[h, 0])
        for o in range(off[h], off[h + 1]):
            T = poses[obs_pose[o]].astype(np.float64)
            T[:3, 3] += T[:3, 0] * sx  # R (X' + s) + t = R X' + (t + R s), s = (sx, 0, 0)
            poses.append(T.astype(f32))
            obs_pose[o] = len(poses) - 1
        start[h, 0] = d
    variants = {k: obs_pose.copy() for k in ("clean", "tied", "free")}
    for j, h in enumerate(hosts):
        pos = sorted({0, 15, 16, int(lens[h]) - 1})
        mid = poses[obs_pose[off[h] + lens[h] // 2]]
        poses.append(_flip(mid))
        away = len(poses) - 1
        if j < 3:  # depth = ((1 * x + z1 * y) + z2 * z) + -0 with both products -0: exactly x
            y, z = start[h, 1], start[h, 2]
            P = T_PERM.copy()
            P[2, 1] = NEG0 if y > 0 else f32(0.0)
            P[2, 2] = NEG0 if z > 0 else f32(0.0)
            assert _bits(depth_f32(P, *start[h]))[0] == _bits(start[h, 0])[0]
            poses.append(P)
        else:
            P = mid.copy()
            P[2, 3] = f32(3e38)
            assert depth_f32(P, *start[h]) == f32(3e38)
            poses.append(P)
        edge = len(poses) - 1
        for q in pos:
            o = off[h] + q
            obs_uv[o] = (10.0, 10.0)
            variants["clean"][o] = away
            variants["tied"][o] = edge if j < 3 else away
            variants["free"][o] = edge if j >= 3 else away
    poses = np.stack(poses).astype(f32)
    base = {"K": K_PIN, "rows": ROWS, "cols": COLS, "poses": poses, "off": off, "obs_uv": obs_uv}
    out = {k: {**base, "obs_pose": v.astype(np.int32), "start": start.copy()} for k, v in variants.items()}
    out["free"]["start"][others[0], 0] = 3e38
    out["free"]["start"][others[1], 1] = -3e38
    out["nan"] = {**base, "obs_pose": variants["clean"].astype(np.int32), "start": start.copy()}
    out["nan"]["start"][others[2], 0] = np.nan
    out["hosts"] = hosts
    out["moved"] = {"tied": [], "free": others[:2], "nan": others[2:]}
    return out
