"""numpy float64 reference of the pose-graph solver (picp_pgo_batch, include/picp_c.h), independent
of csrc/picp_sim3_lie.h: closed-form Exp / Log / Ad on 4x4 matrices, the canonical form by
np.linalg.svd, central-difference Jacobians of the residual itself (node i and node j perturbed on
the right; nothing of the J_r^-1 Ad identity), dense normal equations, np.linalg.solve, and
Gauss-Newton until the gradient is below 1e-12 of its initial value or stalls.

self_check() holds it to scipy: Exp and Log against scipy.linalg.expm / logm on sampled elements,
Ad by S Exp(x) S^-1 = Exp(Ad x), and the optimum's cost against scipy.optimize.least_squares on
the same residual.

Also the test cases (make_ring), the metric (DESIGN.md §4.13's probe discrepancy: eight fixed probe
points through every node's S in double, the largest distance relative to the extent of the
reference's node positions; floor = the reference against its own float32 rounding;
tol = 1e-6 + 4 floor) and the batch file tests/pgo_check/pgo_main.cpp reads.
"""
import functools

import numpy as np

TOL_ABS, TOL_FACTOR = 1e-6, 4.0
FD_STEP = 1e-5
PROBES = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
OK, BAD_INPUT, BAD_EDGE, DISCONNECTED, NOT_PD, TOO_LARGE = range(6)


# ---------------------------------------------------------------------------------------------
# Sim(3): elements are (N, 4, 4) [[c R, t], [0, 1]], tangent vectors (N, 7) = (upsilon, omega, sigma)
# ---------------------------------------------------------------------------------------------
def hat(w):
    w = np.asarray(w, np.float64).reshape(-1, 3)
    W = np.zeros((len(w), 3, 3))
    W[:, 0, 1], W[:, 0, 2] = -w[:, 2], w[:, 1]
    W[:, 1, 0], W[:, 1, 2] = w[:, 2], -w[:, 0]
    W[:, 2, 0], W[:, 2, 1] = -w[:, 1], w[:, 0]
    return W


def _rodrigues(w):
    th = np.linalg.norm(w, axis=1)
    small = th < 1e-4
    ts = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ts) / ts)
    half = np.where(small, 0.5 - th * th / 48.0, np.sin(0.5 * ts) / ts)  # sin(th/2)/th
    b = 2.0 * half * half  # (1 - cos th) / th^2
    W = hat(w)
    return np.eye(3) + a[:, None, None] * W + b[:, None, None] * (W @ W)


def _V(w, sigma):
    """The integral of exp(s (omega^ + sigma I)) over [0, 1]: A I + B W + C W^2 in closed form; below
    theta = 1e-2, where C's numerator cancels, the power series sum M^k / (k + 1)!."""
    th = np.linalg.norm(w, axis=1)
    W = hat(w)
    s0 = sigma == 0.0
    sg = np.where(s0, 1.0, sigma)
    A = np.where(s0, 1.0, np.expm1(sg) / sg)
    small = th < 1e-2
    ts = np.where(small, 1.0, th)
    es, d = np.exp(sigma), sigma * sigma + ts * ts
    B = (es * (sigma * np.sin(ts) - ts * np.cos(ts)) + ts) / (d * ts)
    C = (A - (es * (sigma * np.cos(ts) + ts * np.sin(ts)) - sigma) / d) / (ts * ts)
    V = A[:, None, None] * np.eye(3) + B[:, None, None] * W + C[:, None, None] * (W @ W)
    if small.any():
        M = W[small] + sigma[small, None, None] * np.eye(3)
        term = np.broadcast_to(np.eye(3), M.shape).copy()
        acc = term.copy()
        for k in range(1, 60):
            term = term @ M / (k + 1)
            acc = acc + term
        V[small] = acc
    return V


def exp(x):
    x = np.asarray(x, np.float64).reshape(-1, 7)
    T = np.zeros((len(x), 4, 4))
    T[:, :3, :3] = np.exp(x[:, 6])[:, None, None] * _rodrigues(x[:, 3:6])
    T[:, :3, 3] = np.einsum("nij,nj->ni", _V(x[:, 3:6], x[:, 6]), x[:, :3])
    T[:, 3, 3] = 1.0
    return T


def log(T):
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    c = np.cbrt(np.linalg.det(T[:, :3, :3]))
    R = T[:, :3, :3] / c[:, None, None]
    s = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    sn = np.linalg.norm(s, axis=1)
    cs = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    assert (cs > -0.99).all(), "the reference does not take logarithms near pi"
    th = np.arctan2(sn, cs)
    f = np.where(sn < 1e-7, 1.0 + th * th / 6.0, th / np.where(sn < 1e-7, 1.0, sn))
    w = f[:, None] * s
    sigma = np.log(c)
    u = np.linalg.solve(_V(w, sigma), T[:, :3, 3][:, :, None])[:, :, 0]
    return np.concatenate([u, w, sigma[:, None]], 1)


def inv(T):
    return np.linalg.inv(np.asarray(T, np.float64))


def adjoint(T):
    """(7, 7) [[c R, t^ R, -t], [0, R, 0], [0, 0, 1]] of one element."""
    T = np.asarray(T, np.float64)
    c = np.cbrt(np.linalg.det(T[:3, :3]))
    R, t = T[:3, :3] / c, T[:3, 3]
    A = np.zeros((7, 7))
    A[:3, :3], A[:3, 3:6], A[:3, 6] = c * R, hat(t)[0] @ R, -t
    A[3:6, 3:6] = R
    A[6, 6] = 1.0
    return A


def canonical(M, with_scale=True):
    """The nearest similarity of a float32 4x4 in double, by the SVD; None where the input fails."""
    M = np.asarray(M, np.float32).astype(np.float64)
    if not np.isfinite(M).all():
        return None
    det = np.linalg.det(M[:3, :3])
    if not (det > 0 and np.isfinite(det)):
        return None
    c = np.cbrt(det)
    U, _, Vt = np.linalg.svd(M[:3, :3] / c)
    T = np.eye(4)
    T[:3, :3] = (c if with_scale else 1.0) * (U @ Vt)
    T[:3, 3] = M[:3, 3]
    return T


# ---------------------------------------------------------------------------------------------
# the problem and its solution
# ---------------------------------------------------------------------------------------------
def residuals(S, idx, Zinv, dim=7):
    """(m, dim): Log(Z^-1 S_i^-1 S_j)."""
    if len(idx) == 0:
        return np.zeros((0, dim))
    E = Zinv @ inv(S[idx[:, 0]]) @ S[idx[:, 1]]
    return log(E)[:, :dim]


def cost(S, idx, Zinv, w, dim=7):
    r = residuals(S, idx, Zinv, dim)
    return 0.5 * float((w * (r * r).sum(1)).sum())


def _pad(d, dim):
    out = np.zeros((len(d), 7))
    out[:, :dim] = d
    return out


def solve(S, fixed, edges, Z, weight=None, with_scale=True, max_steps=60):
    """The stationary point Gauss-Newton reaches from S.  S (n, 4, 4), fixed (n,), edges (m, 2),
    Z (m, 4, 4), float32 values as the device gets them.  Returns dict(S float64 (n, 4, 4),
    cost_initial, cost_final, grad_initial, grad_final, steps)."""
    dim = 7 if with_scale else 6
    S = np.stack([canonical(s, with_scale) for s in np.asarray(S, np.float32)]) if len(S) else np.zeros((0, 4, 4))
    idx = np.asarray(edges, np.int64).reshape(-1, 2)
    m = len(idx)
    Zinv = inv(np.stack([canonical(z, with_scale) for z in np.asarray(Z, np.float32)])) if m else np.zeros((0, 4, 4))
    w = np.ones(m) if weight is None else np.asarray(weight, np.float32).astype(np.float64)
    free = np.flatnonzero(~np.asarray(fixed, bool))
    col = -np.ones(len(S), np.int64)
    col[free] = np.arange(len(free))
    nu = dim * len(free)

    def linearise(S):
        r = residuals(S, idx, Zinv, dim)
        J = np.zeros((2, m, dim, dim))
        for side in range(2):
            for c in range(dim):
                d = np.zeros((m, 7))
                d[:, c] = FD_STEP
                P = [S[idx[:, 0]], S[idx[:, 1]]]  # every edge's own copy of its two nodes
                Pp, Pm = list(P), list(P)
                Pp[side] = P[side] @ exp(d)
                Pm[side] = P[side] @ exp(-d)
                rp = log(Zinv @ inv(Pp[0]) @ Pp[1])[:, :dim]
                rm = log(Zinv @ inv(Pm[0]) @ Pm[1])[:, :dim]
                J[side, :, :, c] = (rp - rm) / (2 * FD_STEP)
        H, g = np.zeros((nu, nu)), np.zeros(nu)
        for e in range(m):
            blocks = [(col[idx[e, s]], J[s, e]) for s in range(2) if col[idx[e, s]] >= 0]
            for a, Ja in blocks:
                g[dim * a:dim * a + dim] += w[e] * Ja.T @ r[e]
                for b, Jb in blocks:
                    H[dim * a:dim * a + dim, dim * b:dim * b + dim] += w[e] * Ja.T @ Jb
        return 0.5 * float((w * (r * r).sum(1)).sum()), H, g

    c0, H, g = linearise(S)
    g0 = float(np.linalg.norm(g))
    c, gn, steps, stall = c0, g0, 0, 0
    while nu and m and steps < max_steps and gn > 1e-12 * g0 and stall < 2:
        d = np.linalg.solve(H, -g).reshape(-1, dim)
        S = S.copy()
        S[free] = S[free] @ exp(_pad(d, dim))
        steps += 1
        c, H, g = linearise(S)
        new = float(np.linalg.norm(g))
        stall = stall + 1 if new >= 0.5 * gn else 0
        gn = new
    return {"S": S, "cost_initial": c0, "cost_final": c, "grad_initial": g0, "grad_final": gn, "steps": steps}


# ---------------------------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------------------------
def extent(S):
    t = np.asarray(S, np.float64)[:, :3, 3]
    return float(np.linalg.norm(t.max(0) - t.min(0)))


def _probe(S):
    S = np.asarray(S, np.float64)
    return np.einsum("nij,pj->npi", S[:, :3, :3], PROBES) + S[:, None, :3, 3]


def discrepancy(S, S_ref):
    """Largest distance between the probes' images under both, over the extent of S_ref's positions."""
    return float(np.linalg.norm(_probe(S) - _probe(S_ref), axis=2).max() / extent(S_ref))


def floor(S_ref):
    return discrepancy(np.asarray(S_ref, np.float64).astype(np.float32), S_ref)


def tol(S_ref):
    return TOL_ABS + TOL_FACTOR * floor(S_ref)


# ---------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------
def make_ring(n, noise, loops, seed, sigma_step=0.2, with_scale=True):
    """Ground-truth nodes by composing random steps (translation about 0.2, rotation about 0.1 rad,
    log-scale N(0, sigma_step)); chain edges (k, k + 1) and the loop edges; each Z the true relative
    similarity times Exp(noise N(0, I_7)), rounded to float32; weights U(0.5, 2); the initial nodes
    the chain product of the rounded Z; node 0 fixed.  Returns a graph dict (S, fixed, edges, Z,
    weight) of float32 / uint8 / int32 arrays."""
    rng = np.random.default_rng(seed)
    dim = 7 if with_scale else 6
    step = np.zeros((n - 1, 7))
    step[:, :3] = rng.normal(0, 0.05, (n - 1, 3)) + np.array([0.2, 0.0, 0.0])
    step[:, 3:6] = rng.normal(0, 0.1, (n - 1, 3))
    if with_scale and sigma_step:
        step[:, 6] = rng.normal(0, sigma_step, n - 1)
    truth = [np.eye(4)]
    for T in exp(step):
        truth.append(truth[-1] @ T)
    truth = np.stack(truth)
    edges = [(k, k + 1) for k in range(n - 1)] + [tuple(l) for l in loops]
    idx = np.asarray(edges, np.int32).reshape(-1, 2)
    eps = np.zeros((len(idx), 7))
    eps[:, :dim] = noise * rng.normal(0, 1, (len(idx), dim))
    Z = (inv(truth[idx[:, 0]]) @ truth[idx[:, 1]] @ exp(eps)).astype(np.float32)
    weight = rng.uniform(0.5, 2.0, len(idx)).astype(np.float32)
    S = [np.eye(4)]
    for k in range(n - 1):
        S.append(S[-1] @ Z[k].astype(np.float64))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return {"S": np.stack(S).astype(np.float32), "fixed": fixed, "edges": idx, "Z": Z, "weight": weight}


def permuted(g, seed):
    """The same graph with its nodes renumbered by a random permutation (long envelope rows)."""
    n = len(g["S"])
    perm = np.random.default_rng(seed).permutation(n)  # new index of old node k
    where = np.argsort(perm)
    out = dict(g)
    out["S"], out["fixed"] = g["S"][where], g["fixed"][where]
    out["edges"] = perm[g["edges"]].astype(np.int32)
    return out


CASES = {
    "a": dict(n=12, noise=0.1, loops=[(11, 0), (3, 9)], seed=1),
    "b": dict(n=40, noise=0.05, loops=[(39, 0), (5, 25), (10, 30)], seed=2),
    "c": dict(n=150, noise=0.03, loops=[(149, 0), (20, 100)], seed=3),
    "d": dict(n=12, noise=0.0, loops=[(11, 0)], seed=4),
}


def case(name):
    return make_ring(**CASES[name])


@functools.lru_cache(maxsize=None)
def variants():
    """name -> (graph, with_scale): the four table cases and the ones the device is first checked on."""
    a = case("a")
    out = {k: (case(k), True) for k in CASES}
    two = make_ring(2, 0.1, [], 5)
    two["S"][1] = np.eye(4)  # not at the optimum: the result is S_0 Z
    out["two"] = (two, True)
    tri = make_ring(3, 0.0, [(2, 0)], 6)
    tri["Z"][2] = (tri["Z"][2].astype(np.float64) @ exp([[0.2, -0.1, 0.1, 0.1, 0.05, -0.1, 0.15]])[0]).astype(np.float32)
    out["triangle"] = (tri, True)
    out["ring65"] = (make_ring(65, 0.02, [(64, 0), (10, 40)], 7), True)
    out["ring300"] = (make_ring(300, 0.01, [(299, 0), (50, 200)], 8, sigma_step=0.05), True)
    out["a_permuted"] = (permuted(a, 9), True)
    f5 = dict(a)
    f5["fixed"] = a["fixed"].copy()
    f5["fixed"][5] = 1
    out["a_fixed5"] = (f5, True)
    dup = dict(a)
    dup["edges"] = np.concatenate([a["edges"], a["edges"][4:5]])
    again = a["Z"][4].astype(np.float64) @ exp([[0.05, 0.0, -0.05, 0.02, 0.0, 0.01, 0.03]])[0]
    dup["Z"] = np.concatenate([a["Z"], again[None].astype(np.float32)])  # a second measurement of (4, 5)
    dup["weight"] = np.concatenate([a["weight"], a["weight"][:1]])
    out["a_duplicate"] = (dup, True)
    zw = dict(a)
    zw["weight"] = a["weight"].copy()
    zw["weight"][12] = 0.0  # the (3, 9) loop takes no part
    out["a_zero_weight"] = (zw, True)
    out["a_rigid"] = (make_ring(with_scale=False, **CASES["a"]), False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """solve() of variant `name`, computed once per process; treat it as read-only."""
    g, with_scale = variants()[name]
    return solve(g["S"], g["fixed"], g["edges"], g["Z"], g["weight"], with_scale)


def check_against(name, got_S, got_cost, label=""):
    """The two conditions on a solver's result for variant `name`; prints the figures first."""
    ref = reference(name)
    d, fl, t = discrepancy(got_S, ref["S"]), floor(ref["S"]), tol(ref["S"])
    print("%s%s: discrepancy %.3e, floor %.3e, tol %.3e; cost %.12g, reference %.12g"
          % (label, name, d, fl, t, got_cost, ref["cost_final"]))
    assert d <= t, (name, d, t)
    assert got_cost <= ref["cost_final"] * (1 + 1e-6), (name, got_cost, ref["cost_final"])


# ---------------------------------------------------------------------------------------------
# the batch file of tests/pgo_check/pgo_main.cpp and tests/pgo_facade/pgo_main.cpp
# ---------------------------------------------------------------------------------------------
def write_batch(path, graphs, with_scale=True, iterations=10, damping=0.0, eps=0.0):
    with open(path, "w") as f:
        f.write("%d %d %s %s %d\n" % (1 if with_scale else 0, iterations, float(damping).hex(), float(eps).hex(),
                                      len(graphs)))
        for g in graphs:
            S = np.asarray(g["S"], np.float32).reshape(-1, 4, 4)
            idx = np.asarray(g["edges"], np.int64).reshape(-1, 2)
            Z = np.asarray(g["Z"], np.float32).reshape(-1, 4, 4)
            w = g.get("weight")
            f.write("%d %d %d\n" % (len(S), len(idx), 0 if w is None else 1))
            fl = lambda M: " ".join(_hex(v) for v in M.T.reshape(16))  # column-major
            for k in range(len(S)):
                f.write("%d %s\n" % (int(g["fixed"][k]), fl(S[k])))
            for e in range(len(idx)):
                ws = "" if w is None else _hex(np.float32(w[e])) + " "
                f.write("%d %d %s%s\n" % (idx[e, 0], idx[e, 1], ws, fl(Z[e])))


def _hex(v):
    v = float(v)
    return "nan" if v != v else ("inf" if v == np.inf else "-inf" if v == -np.inf else v.hex())


# ---------------------------------------------------------------------------------------------
# the reference's own checks
# ---------------------------------------------------------------------------------------------
def self_check(seed=0):
    """Returns the figures; asserts each."""
    import scipy.linalg
    import scipy.optimize
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (40, 7)) * rng.choice([1e-9, 1e-5, 1e-3, 0.1, 0.7], (40, 1))
    x[:5, 6] = 0.0
    x[5:10, 3:6] *= 1e-6
    x[:, 6] *= rng.choice([1.0, 1e-6], 40)
    T = exp(x)
    e_exp = e_log = e_ad = 0.0
    for k in range(len(x)):
        A = np.zeros((4, 4))
        A[:3, :3] = hat(x[k, 3:6])[0] + x[k, 6] * np.eye(3)
        A[:3, 3] = x[k, :3]
        e_exp = max(e_exp, np.abs(scipy.linalg.expm(A) - T[k]).max())
        if np.abs(x[k]).max() > 1e-4:  # logm itself loses digits next to the identity
            L = np.real(scipy.linalg.logm(T[k]))
            mine = log(T[k:k + 1])[0]
            back = np.concatenate([L[:3, 3], [L[2, 1], L[0, 2], L[1, 0]], [L[0, 0]]])
            e_log = max(e_log, np.abs(back - mine).max())
        e_log = max(e_log, np.abs(log(T[k:k + 1])[0] - x[k]).max())
        Sx = exp(rng.normal(0, 0.5, (1, 7)))[0]
        e_ad = max(e_ad, np.abs(Sx @ T[k] @ inv(Sx) - exp(adjoint(Sx) @ x[k])[0]).max())
    assert e_exp < 1e-13 and e_log < 1e-11 and e_ad < 1e-12, (e_exp, e_log, e_ad)
    g = case("a")
    ref = solve(g["S"], g["fixed"], g["edges"], g["Z"], g["weight"])
    S0 = np.stack([canonical(s) for s in g["S"]])
    Zinv = inv(np.stack([canonical(z) for z in g["Z"]]))
    w = g["weight"].astype(np.float64)
    free = np.flatnonzero(g["fixed"] == 0)

    def fun(d):
        S = S0.copy()
        S[free] = S[free] @ exp(d.reshape(-1, 7))
        return (np.sqrt(w)[:, None] * residuals(S, g["edges"].astype(np.int64), Zinv)).ravel()

    ls = scipy.optimize.least_squares(fun, np.zeros(7 * len(free)), xtol=1e-15, ftol=1e-15, gtol=1e-15)
    rel = abs(ls.cost - ref["cost_final"]) / ref["cost_final"]
    assert rel < 1e-6, (ls.cost, ref["cost_final"])
    assert ref["grad_final"] < 1e-9 * ref["grad_initial"]
    return {"exp": e_exp, "log": e_log, "ad": e_ad, "cost_rel": rel, "grad": ref["grad_final"] / ref["grad_initial"]}
