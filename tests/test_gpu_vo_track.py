"""GPU tests of the VO sequence's per-map-point track counters (picp_vo_set_track_stats /
picp_vo_get_map_stats, vo_track_kernel in csrc/picp_classify.hip).

Teacher forcing as in test_gpu_vo.py: the map is append-only, so the GPU's final map prefix and
its poses are the inputs of every step.
  * n_matched is EXACT: it follows from descriptor matching alone (oracle.match_points).
  * n_inlier: every accepted match classified in float64 at inv(poses[t+1]).  The test has only
    that inverted camera-in-world pose, not the kernel's own world-in-camera floats, so a map
    point's n_inlier may differ by the number of its AMBIGUOUS matches (|chi2 - thr| <= 1e-3 thr,
    a projected coordinate within 1e-2 px of an image bound, or |z| < 1e-4), and such matches
    must be rare (<= 0.1 % of all matches; the oracle has none on these shapes).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 3000.0
ROWS, COLS = 480, 640
SHAPES = [(25, 600, 8, 0.0), (19, 1500, 6, 0.5)]


def _sequence(n_frames, obs, seg_len, noise):
    from picp_amd.vo_synth import VOSequence, segments
    s = VOSequence(n_frames, obs_per_frame=obs, seed=11, pixel_noise=noise)
    F = s.frames(0, n_frames)
    first, steps = segments(n_frames, seg_len)
    boot = np.stack([[F["T_cw"][f], F["T_cw"][f + 1]] for f in first])
    return s, F, first, steps, boot


def _run(native, s, F, first, steps, boot, track, runs=1, toggle=None):
    seq = native.VOSequence(F["frame_off"], F["uv"], F["desc"], K=s.K)
    seq.set_segments(first, steps, boot, threshold=THR)
    if track:
        seq.track_stats(True)
    outs = []
    for r in range(runs):
        if toggle is not None:
            seq.track_stats(toggle[r])
        seq.run()
        on = toggle[r] if toggle is not None else track
        outs.append({"poses": seq.poses(), "rec": seq.step_records(), "map": [seq.map(k) for k in range(len(first))],
                     "stats": [seq.map_stats(k) for k in range(len(first))] if on else None})
    seq.close()
    return outs


def _assert_same_results(a, b, what):
    for x, y in zip(a["poses"], b["poses"]):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32), err_msg=what)
    for x, y in zip(a["rec"], b["rec"]):
        for f in x:
            np.testing.assert_array_equal(np.asarray(x[f]), np.asarray(y[f]), err_msg=what + " " + f)
    for (xa, da), (xb, db) in zip(a["map"], b["map"]):
        np.testing.assert_array_equal(xa.view(np.uint32), xb.view(np.uint32), err_msg=what + " map")
        np.testing.assert_array_equal(da, db, err_msg=what + " map descriptors")


def _assert_same_stats(a, b, what):
    for (ma, ia), (mb, ib) in zip(a["stats"], b["stats"]):
        np.testing.assert_array_equal(ma, mb, err_msg=what + " n_matched")
        np.testing.assert_array_equal(ia, ib, err_msg=what + " n_inlier")


def _classify64(K, T_cw, xyz, uv):
    """float64 state of every match at inv(T_cw) and whether it is ambiguous."""
    T = np.linalg.inv(np.asarray(T_cw, np.float64))
    K = np.asarray(K, np.float64)
    pc = xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        ph = pc @ K.T
        ix, iy = ph[:, 0] / ph[:, 2], ph[:, 1] / ph[:, 2]
        valid = ~(z <= 0) & ~((ix < 0) | (ix > COLS - 1) | (iy < 0) | (iy > ROWS - 1))
        chi = (ix - uv[:, 0]) ** 2 + (iy - uv[:, 1]) ** 2
        near_bound = (np.minimum(np.abs(ix), np.abs(ix - (COLS - 1))) <= 1e-2) | \
                     (np.minimum(np.abs(iy), np.abs(iy - (ROWS - 1))) <= 1e-2)
        amb = (np.abs(z) < 1e-4) | (~(z <= 0) & near_bound) | (valid & (np.abs(chi - THR) <= 1e-3 * THR))
    return valid & ~(chi > THR), valid, amb


def _reference_counts(oracle, K, off, uv, desc, f0, poses, rec, map_xyz, map_desc):
    n = len(map_xyz)
    n_matched = np.zeros(n, np.int64)
    n_inlier = np.zeros(n, np.int64)
    n_amb = np.zeros(n, np.int64)
    m = int(rec["n_new"][0])
    tot = {"matches": 0, "skipped": 0, "outlier": 0}
    for t in range(len(poses) - 1):
        nf = f0 + t + 1
        wm = oracle.match_points(desc[off[nf]:off[nf + 1]], map_desc[:m])
        acc = np.nonzero(wm["accepted"])[0]
        j = wm["best_idx"][acc]
        assert len(acc) == rec["n_corr"][t + 1]
        np.add.at(n_matched, j, 1)
        inl, valid, amb = _classify64(K, poses[t + 1], map_xyz[j], uv[off[nf]:off[nf + 1]][acc])
        np.add.at(n_inlier, j, inl.astype(np.int64))
        np.add.at(n_amb, j, amb.astype(np.int64))
        tot["matches"] += len(acc)
        tot["skipped"] += int((~valid).sum())
        tot["outlier"] += int((valid & ~inl).sum())
        m += int(rec["n_new"][t + 1])
    assert m == n
    return n_matched, n_inlier, n_amb, tot


@pytest.mark.parametrize("n_frames,obs,seg_len,noise", SHAPES)
def test_track_counters_against_oracle(native, oracle, n_frames, obs, seg_len, noise):
    s, F, first, steps, boot = _sequence(n_frames, obs, seg_len, noise)
    off = _run(native, s, F, first, steps, boot, track=False)[0]
    on = _run(native, s, F, first, steps, boot, track=True)[0]
    _assert_same_results(off, on, "tracking on vs off")  # read-only: poses, records and maps keep their bits
    matches = amb_total = 0
    less = False
    for k, f0 in enumerate(first):
        mx, md = on["map"][k]
        nm, ni = on["stats"][k]
        assert len(nm) == len(mx) and len(ni) == len(mx)
        ref_m, ref_i, ref_amb, tot = _reference_counts(oracle, s.K, F["frame_off"], F["uv"], F["desc"], int(f0),
                                                       on["poses"][k], on["rec"][k], mx, md)
        np.testing.assert_array_equal(nm, ref_m)
        assert nm.sum() == on["rec"][k]["n_corr"][1:].sum()
        assert (ni >= 0).all() and (ni <= nm).all()
        diff = np.abs(ni.astype(np.int64) - ref_i)
        assert (diff <= ref_amb).all(), (int(diff.max()), int(ref_amb.max()))
        matches += tot["matches"]
        amb_total += int(ref_amb.sum())
        less |= bool((ni < nm).any())
    assert matches > 0 and amb_total <= 1e-3 * matches, (amb_total, matches)
    if noise > 0:
        assert less  # some matches are skipped or outliers at the final pose


def test_track_counters_across_schedules(native, monkeypatch):
    """The counters do not depend on the schedule (integer adds), are zeroed per run, and the
    switch takes effect after a captured graph has run."""
    s, F, first, steps, boot = _sequence(*SHAPES[0])
    serial = {"PICP_VO_OVERLAP": "0", "PICP_VO_CHAINS": "1"}
    envs = [dict(serial, PICP_VO_GRAPH="1"), dict(serial, PICP_VO_GRAPH="0"), dict(serial, PICP_VO_FUSE="0"),
            {"PICP_VO_CHAINS": "2"}, {"PICP_VO_CHAINS": "1"}, {"PICP_VO_CHAINS": "2", "PICP_VO_FUSE": "0"}, {}]
    ref = None
    for env in envs:
        for k in ("PICP_VO_OVERLAP", "PICP_VO_CHAINS", "PICP_VO_GRAPH", "PICP_VO_FUSE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        outs = _run(native, s, F, first, steps, boot, track=True, runs=2)  # the second run replays
        if ref is None:
            ref = outs[0]
            assert sum(int(m.sum()) for m, _ in ref["stats"]) == sum(int(r["n_corr"][1:].sum()) for r in ref["rec"])
        for o in outs:
            _assert_same_results(ref, o, str(env))
            _assert_same_stats(ref, o, str(env))
    # toggling after a graph run: off -> on -> off -> on on one handle in the captured serial order
    for k in ("PICP_VO_OVERLAP", "PICP_VO_CHAINS", "PICP_VO_GRAPH", "PICP_VO_FUSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(serial, PICP_VO_GRAPH="1").items():
        monkeypatch.setenv(k, v)
    outs = _run(native, s, F, first, steps, boot, track=False, runs=4, toggle=[False, True, False, True])
    for o in outs:
        _assert_same_results(ref, o, "toggle")
    assert outs[0]["stats"] is None and outs[2]["stats"] is None
    _assert_same_stats(ref, outs[1], "toggle on")
    _assert_same_stats(ref, outs[3], "toggle on again")


def test_map_stats_needs_tracking(native):
    s, F, first, steps, boot = _sequence(8, 300, 8, 0.0)
    seq = native.VOSequence(F["frame_off"], F["uv"], F["desc"], K=s.K)
    seq.set_segments(first, steps, boot, threshold=THR)
    seq.run()
    with pytest.raises(native.PicpError) as e:
        seq.map_stats(0)
    assert e.value.code == native.ERR_STATE
    seq.track_stats(True)
    seq.track_stats(False)
    with pytest.raises(native.PicpError):
        seq.map_stats(0)
    seq.close()
