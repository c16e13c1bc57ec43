"""Frame-size schedules for the VO step: packed synthetic sequences whose frames have EXACT
observation counts, chosen so that the driver takes every code path it selects from the largest
frame (picp_vo_runtime.cpp picp_vo_set_segments: npt; picp_block.hip picp_vo_block_fusable,
block_lds_bytes; picp_vo.hip and picp_vo_device.h: the `frames > 4096 obs` loops) and so that
empty and near-empty steps occur.

A schedule keeps, of frame k of picp_amd.vo_synth.VOSequence(n, obs_per_frame, seed=SEED,
pixel_noise=NOISE), the
first sizes[k] observations: each frame is a seeded shuffle, so that is a random subset with
consistent descriptors.  A frame may instead name a pick rule for its few observations:
  "old": the first observations whose landmark two consecutive earlier kept frames both hold
         (such a landmark is in the map, so the observation matches the map);
  "new": the first observations whose landmark no earlier kept frame holds (not in the map);
  "next": the first observations whose landmark the next source frame sees too;
  "far":  the observations of mapped landmarks that moved the most pixels (at least FAR_PX = 80)
          since the last non-empty kept frame, whose pose the step starts from: they match the
          map and lie outside the solver's inlier gate of sqrt(3000) = 54.8 px;
  "prev": the first observations whose landmark the previous kept frame holds.  A "next" frame
          followed by a "prev" frame of the same size gives a step whose correspondences are
          (nearly) the whole query frame: the only way to more than 11,776 items in one problem
          at max_obs 12,000, where a plain prefix matches 89 % of its observations.
What each schedule then contains -- which step has no correspondence, which appends nothing --
is proven on the CPU oracle by tests/test_vo_shapes_cpu.py; tests/test_gpu_vo_shapes.py runs the
same schedules on the GPU.

  name          max_obs  npt  block launch
  npt_<M>       M        1 (1023), 2 (1024, 2047), 4 (2048, 4095)   fused gather
  fused8        4096     8    fused gather, eight register slots, no LDS stage
  tail1         4097     8    vo_gather_kernel + plain launch, an LDS stage of one item (sized by
                              max_obs; no step of it has more than 4,096 correspondences)
  tails         5000     8    unfused; gather tail chunks (256) and append tail chunks (512) at
                              their edges and ragged; also as overlapping segments (tails_seg)
  streamed      12000    8    unfused; 7,680 items staged, the rest (n_corr - 11,776 > 0 at step 0)
                              streamed every round
"""
import functools

import numpy as np

SEED = 11
# Pixel noise keeps every step's round count a property of the data.  The PICP loop stops when
# chi_in changes by less than 1e-5 of itself.  On noise-free observations chi_in falls to its
# rounding floor, where that relative change is rounding noise and the round count differs even
# between the oracle's own float32 and float64 accumulation (22 against 50 rounds on one step of
# these sizes); with half a pixel of noise chi_in settles at ~0.5 per correspondence and the loop
# stops after 4-9 rounds in both.  A step whose inliers the pose can fit exactly -- ONE inlier
# correspondence: two equations, six unknowns -- has no such level whatever the noise: its chi_in
# falls to (one ulp of a pixel coordinate)^2 = 9.3e-10 and the loop stops when that value repeats
# or drops below the rule's 1e-10, which the last bit of the map point decides.  So the
# one-correspondence step is built with its correspondence outside the inlier gate ("far"):
# n_in = 0, no update, two rounds.  test_vo_shapes_cpu.py holds every step of every schedule to
# both conditions (equal rounds in the oracle's two modes; n_in = 0 or chi_in >= 1e-4 per inlier,
# five orders above the floor).
NOISE = 0.5
THR = 3000.0
ROWS, COLS = 480, 640

OLD, NEW, NXT, PRV, FAR = "old", "new", "next", "prev", "far"
FAR_PX = 80.0  # sqrt(THR) = 54.8 px is the inlier gate

# name -> (obs_per_frame, [size or (size, pick rule)], max_obs, npt, fused, segment length or None)
SCHEDULES = {
    "npt_1023": (2200, [1023, 1022, 512, 1023, 1022], 1023, 1, True, None),
    "npt_1024": (2200, [1024, 1023, 512, 1024, 1023], 1024, 2, True, None),
    "npt_2047": (2200, [2047, 2046, 512, 2047, 2046], 2047, 2, True, None),
    "npt_2048": (2200, [2048, 2047, 512, 2048, 2047], 2048, 4, True, None),
    "npt_4095": (4300, [4095, 4094, 512, 4095, 4094], 4095, 4, True, None),
    "fused8": (4300, [4096, 4095, 3585, 4096, 0, (1, FAR), 4096, 0, (2, NEW), 4096], 4096, 8, True, None),
    "tail1": (4300, [4097, 64, 4097, 4096, 4097], 4097, 8, False, None),
    "tails": (5400, [4096, 4097, 4608, 4095, 4353, 4609, 0, 513, 4352, 4700, (1, NEW), 512, 5000, 257, (64, PRV)],
              5000, 8, False, None),
    "streamed": (14200, [(12000, NXT), (12000, PRV), 11777, 300], 12000, 8, False, None),
}
SCHEDULES["tails_seg"] = SCHEDULES["tails"][:5] + (4,)
NAMES = list(SCHEDULES)


def _size(e):
    return e if isinstance(e, int) else e[0]


def sizes(name):
    return [_size(e) for e in SCHEDULES[name][1]]


@functools.lru_cache(maxsize=None)
def _source(obs, n):
    from picp_amd.vo_synth import VOSequence
    s = VOSequence(n, obs_per_frame=obs, seed=SEED, pixel_noise=NOISE)
    return s, [s.frame(k) for k in range(n)]


def _pick(frames, kept_ids, kept_uv, k, z, rule):
    ids = frames[k]["id_real"]
    if rule == OLD:
        pool = set()
        for j in range(k - 1):
            pool |= set(kept_ids[j].tolist()) & set(kept_ids[j + 1].tolist())
        ok = np.array([i in pool for i in ids.tolist()])
    elif rule == NEW:
        pool = set()
        for j in range(k):
            pool |= set(kept_ids[j].tolist())
        ok = np.array([i not in pool for i in ids.tolist()])
    elif rule == NXT:
        ok = np.isin(ids, frames[k + 1]["id_real"])
    elif rule == FAR:
        j = max(q for q in range(k) if len(kept_ids[q]))  # the frame whose pose the step starts from
        pool = np.intersect1d(kept_ids[j - 1], kept_ids[j])
        prev = dict(zip(kept_ids[j].tolist(), kept_uv[j]))
        move = np.array([np.linalg.norm(frames[k]["uv"][i] - prev[l]) if l in pool else -1.0
                         for i, l in enumerate(ids.tolist())])
        idx = np.argsort(-move, kind="stable")[:z]
        assert move[idx].min() >= FAR_PX, "frame %d: largest pixel move %.1f" % (k, move[idx].min())
        return np.sort(idx)
    else:
        ok = np.isin(ids, kept_ids[k - 1])
    idx = np.nonzero(ok)[0][:z]
    assert len(idx) == z, "frame %d: only %d observations fit the pick rule %r" % (k, len(idx), rule)
    return idx


@functools.lru_cache(maxsize=None)
def build(name):
    """-> dict(name, K, frame_off, uv, desc, id_real, T_cw, sizes, first, steps, boot, max_obs, npt, fused)."""
    from picp_amd.vo_synth import segments
    obs, entries, max_obs, npt, fused, seg_len = SCHEDULES[name]
    n = len(entries)
    s, frames = _source(obs, n)
    uv, desc, kept_ids = [], [], []
    for k, e in enumerate(entries):
        z = _size(e)
        have = len(frames[k]["uv"])
        assert have >= z, "%s: source frame %d has %d observations, the schedule needs %d" % (name, k, have, z)
        idx = np.arange(z) if isinstance(e, int) else _pick(frames, kept_ids, uv, k, z, e[1])
        uv.append(frames[k]["uv"][idx])
        desc.append(frames[k]["desc"][idx])
        kept_ids.append(frames[k]["id_real"][idx])
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(u) for u in uv])
    T_cw = np.stack([s.T_cw(k) for k in range(n)]).astype(np.float32)
    if seg_len is None:
        first, steps = np.array([0], np.int64), np.array([n - 1], np.int32)
    else:
        first, steps = segments(n, seg_len)
    boot = np.stack([[T_cw[f], T_cw[f + 1]] for f in first])
    out = {"name": name, "K": s.K, "frame_off": off, "uv": np.ascontiguousarray(np.concatenate(uv), np.float32),
           "desc": np.ascontiguousarray(np.concatenate(desc), np.float32), "id_real": np.concatenate(kept_ids),
           "T_cw": T_cw, "sizes": [_size(e) for e in entries], "first": first, "steps": steps, "boot": boot,
           "max_obs": max_obs, "npt": npt, "fused": fused}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(name, mode=None):
    import oracle
    S = build(name)
    refs = []
    for k, (f0, st) in enumerate(zip(S["first"], S["steps"])):
        r = oracle.vo_segment(S["K"], ROWS, COLS, S["frame_off"], S["uv"], S["desc"], int(f0), int(st),
                              S["boot"][k][0], S["boot"][k][1], threshold=THR,
                              mode=oracle.MODE_F64 if mode is None else mode)
        for v in r.values():
            v.setflags(write=False)
        refs.append(r)
    return refs


def reference(name, mode=None):
    """The free-running oracle (oracle.vo_segment; mode: its accumulation, float64 by default) of
    every segment of the schedule, computed once."""
    return _reference(name, mode)


def frame(S, f):
    o = S["frame_off"]
    return S["uv"][o[f]:o[f + 1]], S["desc"][o[f]:o[f + 1]]


@functools.lru_cache(maxsize=None)
def _steps(name):
    import oracle
    S = build(name)
    out = []
    for k, (f0, st) in enumerate(zip(S["first"], S["steps"])):
        r = reference(name)[k]
        m = int(r["n_new"][0])
        rows = []
        for t in range(int(st)):
            cf, nf = int(f0) + t, int(f0) + t + 1
            (_, dc), (_, dn) = frame(S, cf), frame(S, nf)
            wm = oracle.match_points(dn, r["map_desc"][:m])
            pm = oracle.match_points(dc, dn)
            sel = pm["accepted"].copy()
            sel[sel] &= ~wm["accepted"][pm["best_idx"][sel]]
            pairs = np.stack([np.nonzero(wm["accepted"])[0], wm["best_idx"][wm["accepted"]]], 1).astype(np.int32)
            _, st_ = oracle.solve(oracle.iso_inverse(r["poses"][t]), S["K"], ROWS, COLS, r["map_xyz"][:m],
                                  frame(S, nf)[0], pairs, THR)
            assert st_["n_in"] == r["n_in"][t] and st_["rounds"] == r["rounds"][t]
            pa, pb = r["poses"][t].astype(np.float64), r["poses"][t + 1].astype(np.float64)
            rows.append({"seg": k, "t": t, "cf": cf, "nf": nf, "nc": len(dc), "nq": len(dn),
                         "n_corr": int(r["n_corr"][t]), "n_new": int(r["n_new"][t + 1]),
                         "n_in": int(st_["n_in"]), "rounds": int(st_["rounds"]), "chi_in": float(st_["chi_in"]),
                         "pairs_accepted": int(pm["accepted"].sum()), "wm": wm, "pm": pm, "map_n": m,
                         "corr_idx_max": int(np.nonzero(wm["accepted"])[0].max()) if wm["accepted"].any() else -1,
                         "new_idx_max": int(np.nonzero(sel)[0].max()) if sel.any() else -1,
                         "baseline": float(np.linalg.norm(pb[:3, 3] - pa[:3, 3])),
                         "same_pose": bool(np.array_equal(r["poses"][t].view(np.uint32),
                                                          r["poses"][t + 1].view(np.uint32)))})
            assert int(wm["accepted"].sum()) == rows[-1]["n_corr"] and int(sel.sum()) == rows[-1]["n_new"]
            m += rows[-1]["n_new"]
        out.append(rows)
    return out


def oracle_steps(name):
    """Per segment, per step of the free-running oracle: frame sizes, counts, the largest
    observation index among the world matches and the selected pairs, the pose's move."""
    return _steps(name)
