"""The canonical observation tracks of a VO segment, rebuilt in numpy by teacher forcing (as
test_gpu_vo_track.py rebuilds the counters): the map is append-only, so the segment's FINAL map
descriptors and its step records' n_new give every step's map, and descriptor matching alone
(oracle.match_points) decides every track.  Everything is integers: a GPU result is compared with
exact equality.

The track of map point j (include/picp_c.h picp_vo_set_track_log): the point was created from the
pair (x in frame f0+c, y in frame f0+c+1) -- c = 0 for a bootstrap point, c = t for a point step t
appended -- and its track holds x, y and every accepted frame->map match of the segment whose best
index is j, except the match whose observation is y itself; ascending by global observation index.
"""
import numpy as np


def reference_tracks(oracle, frame_off, desc, f0, steps, map_desc, n_new, wm_of=None, pm_of=None):
    """frame_off, desc: the packed sequence; f0, steps: the segment; map_desc: its final map
    descriptors; n_new: its step records' n_new (steps + 1 entries, [0] = the bootstrap).
    wm_of(t) / pm_of(c): matches computed elsewhere (frame f0+t+1 against the map before step t's
    append / frame f0+c against frame f0+c+1) instead of a call of oracle.match_points.
    -> dict(track_off int64 (n+1), obs_slot int32, obs_index int64, own_y bool (n): the point's own
    y matched it (and is not counted twice), wm: per step (accepted, best_idx) of the frame->map match)."""
    off = np.asarray(frame_off, np.int64)
    f0, steps = int(f0), int(steps)
    n = len(map_desc)

    def frame(f):
        return desc[off[f]:off[f + 1]]

    def pairs(c):
        pm = pm_of(c) if pm_of is not None else oracle.match_points(frame(f0 + c), frame(f0 + c + 1))
        acc = np.nonzero(np.asarray(pm["accepted"]).astype(bool))[0]
        return acc, np.asarray(pm["best_idx"])[acc].astype(np.int64)

    cre_x, cre_y, cre_c = [], [], []

    def create(c, has_map_match):
        """the kept pairs of (f0+c, f0+c+1) in pair order: the k-th created map point m_before + k"""
        x, y = pairs(c)
        if has_map_match is not None:
            keep = ~has_map_match[y]
            x, y = x[keep], y[keep]
        cre_x.extend((off[f0 + c] + x).tolist())
        cre_y.extend((off[f0 + c + 1] + y).tolist())
        cre_c.extend([c] * len(x))
        return len(x)

    m = create(0, None)
    assert m == int(n_new[0]), (m, int(n_new[0]))
    match_pt, match_obs, match_slot, wms = [], [], [], []
    own_y = np.zeros(n, bool)
    for t in range(steps):
        nf = f0 + t + 1
        wm = wm_of(t) if wm_of is not None else oracle.match_points(frame(nf), map_desc[:m])
        acc = np.asarray(wm["accepted"]).astype(bool)
        bi = np.asarray(wm["best_idx"]).astype(np.int64)
        wms.append((acc.copy(), bi.copy()))
        i = np.nonzero(acc)[0]
        j, g = bi[i], off[nf] + i
        assert (j < m).all()
        own = g == np.asarray(cre_y, np.int64)[j] if len(i) else np.zeros(0, bool)
        own_y[j[own]] = True
        match_pt.extend(j[~own].tolist())
        match_obs.extend(g[~own].tolist())
        match_slot.extend([t + 1] * int((~own).sum()))
        k = create(t, acc)
        assert k == int(n_new[t + 1]), (t, k, int(n_new[t + 1]))
        m += k
    assert m == n, (m, n)
    # assemble: x, y and the matches of every point, ascending by global observation index
    cx, cy, cc = (np.asarray(v, np.int64) for v in (cre_x, cre_y, cre_c))
    pt = np.concatenate([np.arange(n), np.arange(n), np.asarray(match_pt, np.int64)]).astype(np.int64)
    ob = np.concatenate([cx, cy, np.asarray(match_obs, np.int64)]).astype(np.int64)
    sl = np.concatenate([cc, cc + 1, np.asarray(match_slot, np.int64)]).astype(np.int64)
    order = np.lexsort((ob, pt))
    track_off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(pt, minlength=n), out=track_off[1:])
    return {"track_off": track_off, "obs_slot": sl[order].astype(np.int32), "obs_index": ob[order],
            "own_y": own_y, "wm": wms}
