"""numpy float64 restatement of the device Sim(3) RANSAC (csrc/picp_sim3.hip), independent of its
code: the sampler (tests/pnp_ref.py: the same pure function), the closed form
(picp_amd.evaluate.umeyama: np.linalg.svd, nothing of the Jacobi), the float32 inlier test in the
order include/picp_c.h states, and the selection and refit rules.

The metric is §4.12's probe discrepancy, with the case's own points as the probes: both transforms
map the src points in double, and the discrepancy is the largest distance between the two images
relative to the dst cloud's extent (the diagonal of its bounding box).  `floor` is that
discrepancy between a reference transform and its own float32 rounding, and the bound for a float32
result is tol = 1e-6 + 4 floor (TOL_FACTOR: the float32 result sits at ratio <= 1 by definition).
"""
import os
import subprocess

import numpy as np

import pnp_ref
from picp_amd.evaluate import umeyama

N_CASES = 64
TOL_ABS, TOL_FACTOR = 1e-6, 4.0
RANK_EPS = 1e-10  # sigma_2 <= RANK_EPS sigma_1: no transform
# (n, seed) of the end-to-end cases (50 % outliers, 1 cm noise) the CPU and the GPU tests share
E2E_CASES = [(n, seed) for n in (64, 500) for seed in (100, 101, 102, 103)]
E2E_THRESHOLD = 0.01

samples = pnp_ref.samples


# ---------------------------------------------------------------------------------------------
# the closed form
# ---------------------------------------------------------------------------------------------
def closed(src, dst, with_scale=True):
    """Umeyama's 4x4 [[c R, t], [0, 1]] (float64) of the pairs, or None where they give no
    transform: fewer than 3, a non-finite coordinate, no source variance, covariance of rank < 2."""
    src = np.asarray(src, np.float64).reshape(-1, 3)
    dst = np.asarray(dst, np.float64).reshape(-1, 3)
    if len(src) < 3 or not (np.isfinite(src).all() and np.isfinite(dst).all()):
        return None
    xs, xd = src - src.mean(0), dst - dst.mean(0)
    if not (xs * xs).sum() > 0:
        return None
    sv = np.linalg.svd(xd.T @ xs, compute_uv=False)
    if not (sv[0] > 0 and sv[1] > RANK_EPS * sv[0]):
        return None
    S = umeyama(src, dst, with_scale)
    return S if np.isfinite(S).all() else None


def closed32(src, dst, with_scale=True):
    """closed() rounded to float32, as the device stores, scores and returns it; None as closed()."""
    S = closed(src, dst, with_scale)
    if S is None:
        return None
    S32 = S.astype(np.float32)
    return S32 if np.isfinite(S32).all() else None


def scale_of(S):
    """c of [[c R, t], [0, 1]] with det R = +1."""
    return float(np.cbrt(np.linalg.det(np.asarray(S, np.float64)[:3, :3])))


def apply(S, p):
    S = np.asarray(S, np.float64)
    return np.asarray(p, np.float64) @ S[:3, :3].T + S[:3, 3]


def extent(dst):
    d = np.asarray(dst, np.float64)
    return float(np.linalg.norm(d.max(0) - d.min(0)))


def discrepancy(Sa, Sb, src, dst):
    """Largest distance between the images of the case's src points under both, over dst's extent."""
    return float(np.linalg.norm(apply(Sa, src) - apply(Sb, src), axis=1).max() / extent(dst))


def floor(S, src, dst):
    return discrepancy(S, np.asarray(S, np.float64).astype(np.float32), src, dst)


def tol(S, src, dst):
    return TOL_ABS + TOL_FACTOR * floor(S, src, dst)


# ---------------------------------------------------------------------------------------------
# the float32 inlier test, the selection and the refits
# ---------------------------------------------------------------------------------------------
def d2_f32(S, src, dst):
    """(n,) float32 squared distances in the stated order: per row
    e_r = (((m_r0 x + m_r1 y) + m_r2 z) + t_r) - q_r, d2 = (e_0^2 + e_1^2) + e_2^2, every operation
    rounded to float32 (numpy float32 arithmetic does not contract)."""
    S = np.asarray(S, np.float32)
    p = np.asarray(src, np.float32).reshape(-1, 3)
    q = np.asarray(dst, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = [(((S[r, 0] * p[:, 0] + S[r, 1] * p[:, 1]) + S[r, 2] * p[:, 2]) + S[r, 3]) - q[:, r] for r in range(3)]
        return (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]


def inlier_mask(S, src, dst, thr):
    with np.errstate(invalid="ignore"):
        return d2_f32(S, src, dst) < np.float32(thr)  # strict: a NaN fails


def count(S, src, dst, thr):
    return int(inlier_mask(S, src, dst, thr).sum())


def hypotheses(src, dst, seed, i, H, with_scale=True):
    """Per hypothesis the float32 4x4 or None."""
    n = len(src)
    smp = samples(seed, i, H, n)
    return [closed32(src[smp[h]], dst[smp[h]], with_scale) if n >= 4 else None for h in range(H)]


def select(counts, valid):
    """The valid hypothesis with the largest count, then the lowest index; None when none is valid."""
    best = None
    for h in range(len(valid)):
        if valid[h] and (best is None or counts[h] > counts[best]):
            best = h
    return best


def refit_chain(S0, src, dst, thr, refits, with_scale=True):
    """[(S_r float32 or None, count_r or -1)] for r = 1..refits: S_r is the closed form of the
    inliers of S_(r-1); the chain ends at a refit without a transform."""
    out, cur = [], S0
    for _ in range(refits):
        if cur is not None:
            m = inlier_mask(cur, src, dst, thr)
            cur = closed32(src[m], dst[m], with_scale)
        out.append((cur, count(cur, src, dst, thr) if cur is not None else -1))
    return out


def choose(S0, count0, chain):
    """The candidate with the largest count among {winner, refit 1, ...}, the latest on a tie."""
    best, best_c = S0, count0
    for S, c in chain:
        if S is not None and c >= best_c:
            best, best_c = S, c
    return best, best_c


def finish(S0, count0, chain, src, dst, thr, min_inliers):
    """dict(S, scale, inliers, found, rms, mask) from the winner (None: no valid hypothesis) and its chain."""
    n = len(src)
    if S0 is None or n < 4:
        S, c = None, 0
    else:
        S, c = choose(S0, count0, chain)
    found = S is not None and c >= min_inliers
    if not found:
        return {"S": np.eye(4, dtype=np.float32), "scale": 1.0, "inliers": c, "found": False, "rms": 0.0,
                "mask": np.zeros(n, bool)}
    m = inlier_mask(S, src, dst, thr)
    rms = float(np.sqrt(d2_f32(S, src, dst)[m].astype(np.float64).sum() / c)) if c else 0.0
    return {"S": S, "scale": scale_of(S), "inliers": c, "found": True, "rms": rms, "mask": m}


def ransac(src, dst, thr=0.01, H=256, min_inliers=4, with_scale=True, refits=2, seed=0, i=0):
    """The whole reference pipeline."""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    dst = np.asarray(dst, np.float32).reshape(-1, 3)
    hyps = hypotheses(src, dst, seed, i, H, with_scale)
    valid = [S is not None for S in hyps]
    counts = [count(S, src, dst, thr) if S is not None else 0 for S in hyps]
    w = select(counts, valid)
    S0 = hyps[w] if w is not None else None
    chain = refit_chain(S0, src, dst, thr, refits, with_scale) if S0 is not None else []
    out = finish(S0, counts[w] if w is not None else 0, chain, src, dst, thr, min_inliers)
    out.update(hyps=hyps, counts=counts, winner=w, chain=chain)
    return out


# ---------------------------------------------------------------------------------------------
# constructed cases
# ---------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def similarity(c, R, t):
    S = np.eye(4)
    S[:3, :3] = c * R
    S[:3, 3] = t
    return S


def _draw(rng, c=None):
    c = float(rng.uniform(0.5, 2.0)) if c is None else c
    return c, random_rotation(rng), rng.uniform(-5, 5, 3)


def _family_case(name, rng):
    """(src, dst, with_scale) in float64, before the rounding to float32."""
    ws = True
    if name == "generic_triples":
        c, R, t = _draw(rng)
        src = rng.uniform(-5, 5, (3, 3))
    elif name == "clouds_500":
        c, R, t = _draw(rng)
        src = rng.uniform(-5, 5, (500, 3))
    elif name == "planar":
        c, R, t = _draw(rng)
        src = np.column_stack([rng.uniform(-5, 5, (50, 2)), np.zeros(50)]) @ random_rotation(rng).T + rng.uniform(-2, 2, 3)
    elif name == "mirrored":
        c, R, t = _draw(rng)
        src = rng.uniform(-5, 5, (20, 3))
        R = R @ np.diag([1.0, 1.0, -1.0])  # dst is a mirror image: no rotation maps src onto it
    elif name == "near_collinear":
        c, R, t = _draw(rng)
        a, d = rng.uniform(-5, 5, 3), random_rotation(rng)[:, 0]
        off = np.cross(d, random_rotation(rng)[:, 0])
        src = np.stack([a, a + 4 * d, a + 2 * d + 4e-4 * off / np.linalg.norm(off)])  # 1e-4 of the length off the line
    elif name == "scale_1e-3":
        c, R, t = _draw(rng, 1e-3)
        src = rng.uniform(-5, 5, (50, 3))
    elif name == "scale_1e3":
        c, R, t = _draw(rng, 1e3)
        src = rng.uniform(-5, 5, (50, 3))
    elif name == "far_1e4":
        c, R, t = _draw(rng, 1.0)
        src = rng.uniform(-0.5, 0.5, (50, 3))
        far = 1e4 * random_rotation(rng)[:, 0]
        dst = src @ R.T + far + rng.uniform(-5, 5, 3)  # both clouds of 1 m extent, 1e4 m from the origin
        return src + far, dst, ws
    elif name == "rigid":
        c, R, t = _draw(rng, 1.3)
        src = rng.uniform(-5, 5, (50, 3))
        ws = False
    else:
        raise KeyError(name)
    dst = c * src @ R.T + t
    if name in ("clouds_500", "rigid"):
        dst = dst + rng.normal(0, 0.01, dst.shape)  # a least-squares problem, not an exact one
    return src, dst, ws


FAMILIES = ["generic_triples", "clouds_500", "planar", "mirrored", "near_collinear", "scale_1e-3", "scale_1e3",
            "far_1e4", "rigid"]


def family(name, n_cases=N_CASES):
    """Seeded cases (src, dst, with_scale), inputs rounded to float32 as the device reads them."""
    rng = np.random.default_rng([FAMILIES.index(name), 2718])
    for _ in range(n_cases):
        src, dst, ws = _family_case(name, rng)
        yield src.astype(np.float32), dst.astype(np.float32), ws


def no_transform_cases():
    """name -> (src, dst) that give no transform."""
    rng = np.random.default_rng(31)
    p = rng.uniform(-5, 5, (3, 3)).astype(np.float32)
    q = rng.uniform(-5, 5, (3, 3)).astype(np.float32)
    line = np.array([[1, 2, 3], [2, 4, 4], [3, 6, 5]], np.float32)  # exact in float32
    out = {
        "coincident": (np.repeat(p[:1], 3, 0), np.repeat(q[:1], 3, 0)),
        "coincident_src": (np.repeat(p[:1], 3, 0), q),
        "collinear": (line, 2 * line + 1),
        "collinear_src": (line, q),
        "collinear_dst": (p, line),
        "two_pairs": (p[:2], q[:2]),
    }
    for name, bad in (("nan", np.nan), ("inf", np.inf), ("neg_inf", -np.inf)):
        for side in (0, 1):
            a, b = p.copy(), q.copy()
            (a, b)[side][1, 2] = bad
            out["%s_%s" % (name, "src" if side == 0 else "dst")] = (a, b)
    cloud = rng.uniform(-5, 5, (20, 3)).astype(np.float32)
    out["zero_variance_cloud"] = (np.repeat(p[:1], 20, 0), cloud)
    return out


def e2e_case(n, seed, outlier_frac=0.5, noise=0.01):
    """A robustness case: (src, dst, S_true, is_outlier).  n matches of a similarity with `noise` m
    of Gaussian noise on dst; the outliers' dst are uniform in the dst cloud's box."""
    rng = np.random.default_rng([seed, n])
    c, R, t = _draw(rng)
    src = rng.uniform(-5, 5, (n, 3))
    dst = c * src @ R.T + t
    lo, hi = dst.min(0), dst.max(0)
    dst = dst + rng.normal(0, noise, dst.shape)
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outlier_frac * n))]] = True
    dst[out] = rng.uniform(lo, hi, (int(out.sum()), 3))
    return src.astype(np.float32), dst.astype(np.float32), similarity(c, R, t), out


def self_check():
    """On float64-exact constructed similarities the closed form returns the constructed (c, R, t)."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for k in range(32):
        c, R, t = _draw(rng)
        if k % 2:
            src = rng.uniform(-5, 5, (3, 3))
        else:
            src = rng.uniform(-5, 5, (40, 3))
        S_true = similarity(c, R, t)
        S = closed(src, apply(S_true, src))
        assert S is not None
        assert abs(np.linalg.det(S[:3, :3] / scale_of(S)) - 1) < 1e-12
        worst = max(worst, np.abs(S - S_true).max(), abs(scale_of(S) - c))
    assert worst < 1e-9, worst
    # a mirror image has no rotation: det R stays +1 and the residual is that of the best rotation
    src = rng.uniform(-5, 5, (30, 3))
    S = closed(src, src * np.array([1.0, 1.0, -1.0]))
    assert abs(np.linalg.det(S[:3, :3] / scale_of(S)) - 1) < 1e-12
    return worst


# ---------------------------------------------------------------------------------------------
# the host build of csrc/picp_umeyama.h (bin/sim3_check, bin/sim3_check_plain)
# ---------------------------------------------------------------------------------------------
def run_check(exe, cases, tmp_path, name="cases"):
    """cases: [(src, dst, with_scale)] -> [float32 4x4 or None], [c or None] from the host build."""
    path = os.path.join(str(tmp_path), name + ".txt")
    with open(path, "w") as f:
        for src, dst, ws in cases:
            src = np.asarray(src, np.float32).reshape(-1, 3)
            dst = np.asarray(dst, np.float32).reshape(-1, 3)
            f.write("%d %d\n" % (1 if ws else 0, len(src)))
            for p, q in zip(src, dst):
                f.write(" ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in list(p) + list(q)) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(cases)
    Ss, cs = [], []
    for ln in lines:
        tok = ln.split()
        if tok[0] == "0":
            Ss.append(None)
            cs.append(None)
            continue
        v = np.array([float.fromhex(t) for t in tok[1:]], np.float32)
        assert len(v) == 13
        S = np.eye(4, dtype=np.float32)
        S[:3, :3] = v[:9].reshape(3, 3).T  # column-major
        S[:3, 3] = v[9:12]
        Ss.append(S)
        cs.append(v[12])
    return Ss, cs
