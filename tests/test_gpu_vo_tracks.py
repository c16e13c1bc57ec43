"""GPU tests of the VO sequence's observation tracks and map refinement (picp_vo_set_track_log,
picp_vo_get_tracks, picp_vo_get_poses_wc, picp_vo_refine_map; csrc/picp_vo_tracks.hip).

The tracks are integers and follow from descriptor matching alone, so they are compared with the
numpy reference (tests/vo_tracks_ref.py, teacher-forced from the GPU's final map descriptors and
step records) by exact equality.  The refinement is the standalone refiner's kernel on the same
tracks, poses and points, so it is compared with PointRefiner bit for bit (PointRefiner itself is
held to the float64 oracle by test_gpu_refine.py).
"""
import ctypes
import functools

import numpy as np
import pytest

import vo_shapes as VS
import vo_tracks_ref

pytestmark = pytest.mark.gpu

THR = 3000.0
ENV_KEYS = ("PICP_VO_FUSE", "PICP_VO_OVERLAP", "PICP_VO_CHAINS", "PICP_VO_SPLIT", "PICP_VO_GRAPH", "PICP_VO_GUARD",
            "PICP_VO_PHASE", "PICP_VO_MATCH_FULL")
SERIAL = {"PICP_VO_OVERLAP": "0", "PICP_VO_CHAINS": "1"}
# test_track_counters_across_schedules' list: serial graph, enqueued, unfused, two chains, one chain, default
ENVS = [dict(SERIAL, PICP_VO_GRAPH="1"), dict(SERIAL, PICP_VO_GRAPH="0"), dict(SERIAL, PICP_VO_FUSE="0"),
        {"PICP_VO_CHAINS": "2"}, {"PICP_VO_CHAINS": "1"}, {"PICP_VO_CHAINS": "2", "PICP_VO_FUSE": "0"}, {}]


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


def _setenv(monkeypatch, env):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _synth(n_frames, obs, seg_len, noise, first=None, steps=None, dup=0):
    from picp_amd.vo_synth import VOSequence, segments
    s = VOSequence(n_frames, obs_per_frame=obs, seed=11, pixel_noise=noise)
    F = s.frames(0, n_frames)
    if first is None:
        first, steps = segments(n_frames, seg_len)
    first, steps = np.asarray(first, np.int64), np.asarray(steps, np.int32)
    off, uv, desc, ids = F["frame_off"], F["uv"], F["desc"], F["id_real"]
    if dup:
        # `dup` observations of each segment's last frame once more (the same descriptor, the pixel
        # moved by half a pixel), appended to the frame.  They are chosen among landmarks the two
        # frames before hold too (so they are in the map and match it) and the frame after does
        # not (so no frame->next pair starts from a duplicated descriptor).
        fr = lambda f: slice(off[f], off[f + 1])
        last = set(int(f + st) for f, st in zip(first, steps))
        parts = []
        for f in range(n_frames):
            u, d, i = uv[fr(f)], desc[fr(f)], ids[fr(f)]
            if f in last:
                ok = np.isin(i, ids[fr(f - 1)]) & np.isin(i, ids[fr(f - 2)])
                if f + 1 < n_frames:
                    ok &= ~np.isin(i, ids[fr(f + 1)])
                k = np.nonzero(ok)[0][:dup]
                assert len(k) == dup
                u, d, i = np.concatenate([u, u[k] + 0.5]), np.concatenate([d, d[k]]), np.concatenate([i, i[k]])
            parts.append((u, d, i))
        off = np.zeros(n_frames + 1, np.int64)
        off[1:] = np.cumsum([len(p[0]) for p in parts])
        uv, desc, ids = (np.ascontiguousarray(np.concatenate([p[q] for p in parts])) for q in range(3))
    boot = np.stack([[F["T_cw"][f], F["T_cw"][f + 1]] for f in first])
    return {"K": s.K, "frame_off": off, "uv": uv.astype(np.float32), "desc": desc.astype(np.float32),
            "first": first, "steps": steps, "boot": boot, "shape": None}


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "seg8":
        return _synth(25, 600, 8, 0.0)
    if name == "noise":
        return _synth(19, 1500, 6, 0.5)  # the second shape of test_gpu_vo_track.py
    if name == "deep":  # frames are queried by different segments at different steps
        return _synth(25, 600, 8, 0.0, first=[0, 2, 4], steps=[6, 6, 6])
    if name == "dup":
        return _synth(25, 600, 8, 0.0, dup=3)
    S = VS.build(name)
    return {"K": S["K"], "frame_off": S["frame_off"], "uv": S["uv"], "desc": S["desc"], "first": S["first"],
            "steps": S["steps"], "boot": S["boot"], "shape": name}


def _open(native, C, log=True, stats=False):
    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    if log:
        seq.track_log(True)
    if stats:
        seq.track_stats(True)
    return seq


def _results(seq, n):
    return {"poses": seq.poses(), "rec": seq.step_records(), "map": [seq.map(k) for k in range(n)]}


def _debug_matches(native, seq, n_obs):
    out = []
    for which in (2, 3):
        dst = np.zeros(max(int(n_obs), 1), np.int32)
        assert native.lib().picp_vo_debug_matches(seq._h, which, dst.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
        out.append(dst)
    return out


_RUNS = {}


def _gpu(native, name):
    """The default schedule's run of a case with the log and the counters on, shared by the tests."""
    if name not in _RUNS:
        C = _case(name)
        n = len(C["first"])
        seq = _open(native, C, stats=True)
        seq.run()
        out = _results(seq, n)
        out["tracks"] = [seq.tracks(k) for k in range(n)]
        out["stats"] = [seq.map_stats(k) for k in range(n)]
        out["wm"] = _debug_matches(native, seq, C["frame_off"][-1])
        seq.close()
        _RUNS[name] = out
    return _RUNS[name]


_REFS = {}


def _ref(oracle, native, name):
    """The reference tracks of every segment of a case, from the shared run's map and records."""
    if name not in _REFS:
        C, out = _case(name), _gpu(native, name)
        refs = []
        for k, (f0, st) in enumerate(zip(C["first"], C["steps"])):
            kw = {}
            if C["shape"]:
                # the schedule's matches were computed once for test_gpu_vo_shapes.py (the oracle's
                # own map): they are this segment's when the GPU's map descriptors equal the oracle's
                rows, r = VS.oracle_steps(C["shape"])[k], VS.reference(C["shape"])[k]
                np.testing.assert_array_equal(out["map"][k][1], r["map_desc"])
                kw = {"wm_of": lambda t, rows=rows: rows[t]["wm"], "pm_of": lambda c, rows=rows: rows[c]["pm"]}
            refs.append(vo_tracks_ref.reference_tracks(oracle, C["frame_off"], C["desc"], f0, st, out["map"][k][1],
                                                       out["rec"][k]["n_new"], **kw))
        _REFS[name] = refs
    return _REFS[name]


def _assert_tracks_equal(got, ref, what):
    off, slot, idx = got
    assert off.dtype == np.int64 and slot.dtype == np.int32 and idx.dtype == np.int64
    np.testing.assert_array_equal(off, ref["track_off"], err_msg=what + " track_off")
    np.testing.assert_array_equal(idx, ref["obs_index"], err_msg=what + " obs_index")
    np.testing.assert_array_equal(slot, ref["obs_slot"], err_msg=what + " obs_slot")


def _assert_same_tracks(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for p, q in zip(x, y):
            np.testing.assert_array_equal(p, q, err_msg=what)


def _assert_same_results(a, b, what):
    for x, y in zip(a["poses"], b["poses"]):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32), err_msg=what)
    for x, y in zip(a["rec"], b["rec"]):
        for f in x:
            np.testing.assert_array_equal(np.asarray(x[f]).view(np.uint32), np.asarray(y[f]).view(np.uint32),
                                          err_msg=what + " " + f)
    for (xa, da), (xb, db) in zip(a["map"], b["map"]):
        np.testing.assert_array_equal(xa.view(np.uint32), xb.view(np.uint32), err_msg=what + " map")
        np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32), err_msg=what + " map descriptors")


# ---- 1. the tracks equal the reference exactly

@pytest.mark.parametrize("name", ["seg8", "noise", "tails", "tails_seg", "deep"])
def test_tracks_equal_the_reference(native, oracle, name):
    C, out, refs = _case(name), _gpu(native, name), _ref(oracle, native, name)
    if name == "deep":
        # What a rebuild from wm_* after the run would read: a shared frame's rows are those of the
        # segment that queried it LAST.  Segment s queries frame f at step f - first[s] - 1, so in
        # this layout that is segment 0, and every other segment's matches of the frame are gone:
        # segment 1's reference matches of frame 3 (its step 0; segment 0's step 2) differ from
        # the rows the run left, which are segment 0's.
        off = C["frame_off"]
        wm_bi, wm_acc = out["wm"]
        for f, s_last, s_lost in ((3, 0, 1), (5, 0, 2), (7, 1, 2)):
            q = slice(off[f], off[f + 1])
            acc, bi = refs[s_lost]["wm"][f - int(C["first"][s_lost]) - 1]
            left = np.where(wm_acc[q] != 0, wm_bi[q], -1)
            assert not np.array_equal(left, np.where(acc, bi, -1)), "frame %d: nothing was overwritten" % f
            if s_last == 0:
                acc0, bi0 = refs[0]["wm"][f - 1]
                np.testing.assert_array_equal(left, np.where(acc0, bi0, -1))
    if name == "tails_seg":
        # the scan of the track lengths runs per segment in chunks of 1,024 points: among the named
        # cases this one has a segment of more than two chunks and one of less than a chunk
        n_map = [len(out["map"][k][0]) for k in range(len(C["first"]))]
        assert max(n_map) > 2048 and min(n_map) < 1024, n_map
    total = 0
    for k in range(len(C["first"])):
        _assert_tracks_equal(out["tracks"][k], refs[k], "%s segment %d" % (name, k))
        assert len(out["tracks"][k][0]) == len(out["map"][k][0]) + 1
        total += len(out["tracks"][k][2])
    assert total > 0


# ---- 2. several observations of one frame on one point

def test_repeated_observations_of_one_frame_stay(native, oracle):
    C, out, refs = _case("dup"), _gpu(native, "dup"), _ref(oracle, native, "dup")
    repeated = 0
    for k, r in enumerate(refs):
        off, slot = r["track_off"], r["obs_slot"]
        for j in range(len(off) - 1):
            s = slot[off[j]:off[j + 1]]
            repeated += int((s[1:] == s[:-1]).any())
        _assert_tracks_equal(out["tracks"][k], r, "dup segment %d" % k)
    assert repeated >= 1


# ---- 3. consistency with the track counters

@pytest.mark.parametrize("name", ["seg8", "noise", "dup"])
def test_track_lengths_fit_the_counters(native, oracle, name):
    out, refs = _gpu(native, name), _ref(oracle, native, name)
    for k, r in enumerate(refs):
        off = out["tracks"][k][0]
        n_matched = out["stats"][k][0]
        own = r["own_y"].astype(np.int64)
        np.testing.assert_array_equal(np.diff(off) - 2, n_matched - own)
        assert int((np.diff(off) - 2).sum()) + int(own.sum()) == int(out["rec"][k]["n_corr"][1:].sum())
    assert sum(int(r["own_y"].sum()) for r in refs) > 0


# ---- 4. read-only and schedule-independent

def test_log_is_read_only_and_schedule_independent(native, monkeypatch):
    C = _case("seg8")
    n = len(C["first"])
    ref = _gpu(native, "seg8")
    seq = _open(native, C, log=False)
    seq.run()
    _assert_same_results(ref, _results(seq, n), "log off vs on")
    seq.close()
    for env in ENVS:
        _setenv(monkeypatch, env)
        seq = _open(native, C)
        for r in range(2):  # the second run replays
            seq.run()
            _assert_same_results(ref, _results(seq, n), "%s run %d" % (env, r))
            _assert_same_tracks(ref["tracks"], [seq.tracks(k) for k in range(n)], "%s run %d" % (env, r))
        seq.close()
    # off -> on -> off -> on on one handle, after a run of the captured serial order
    _setenv(monkeypatch, dict(SERIAL, PICP_VO_GRAPH="1"))
    seq = _open(native, C, log=False)
    for on in (False, True, False, True):
        seq.track_log(on)
        seq.run()
        _assert_same_results(ref, _results(seq, n), "toggle")
        if on:
            _assert_same_tracks(ref["tracks"], [seq.tracks(k) for k in range(n)], "toggle on")
        else:
            with pytest.raises(native.PicpError) as e:
                seq.tracks(0)
            assert e.value.code == native.ERR_STATE
    seq.close()


# ---- 5. the refinement is the refine kernel

def _standalone(native, C, seq, segs, **prm):
    """PointRefiner on the tracks, poses and map of the segments `segs` of an open handle."""
    slot0 = np.concatenate([[0], np.cumsum(C["steps"].astype(np.int64) + 1)])
    offs, poses, uvs, xyz, base = [np.zeros(1, np.int64)], [], [], [], 0
    for k in segs:
        off, slot, idx = seq.tracks(k)
        offs.append(base + off[1:])
        base += int(off[-1])
        poses.append(slot0[k] + slot)
        uvs.append(C["uv"][idx].reshape(-1, 2))
        xyz.append(seq.map(k)[0])
    R = native.PointRefiner(K=C["K"])
    R.set_poses(np.concatenate(seq.poses_wc()))
    R.set_tracks(np.concatenate(offs), np.concatenate(poses).astype(np.int32), np.concatenate(uvs))
    R.set_points(np.concatenate(xyz))
    out = R.run(**prm)
    R.close()
    return out


def _assert_refined_equal(got, want, what):
    (gx, gs), (wx, ws) = got, want
    np.testing.assert_array_equal(gx.view(np.uint32), wx.view(np.uint32), err_msg=what + " points")
    for f in ws:
        np.testing.assert_array_equal(gs[f].view(np.uint32), ws[f].view(np.uint32), err_msg=what + " " + f)


@pytest.mark.parametrize("name", ["seg8", "tails_seg"])
def test_refined_map_equals_the_standalone_refiner(native, oracle, name):
    C = _case(name)
    n = len(C["first"])
    seq = _open(native, C)
    seq.run()
    for k, inv in enumerate(seq.poses_wc()):  # the table is the float32 rigid inverse of poses()
        want = np.stack([oracle.iso_inverse(T) for T in seq.poses()[k]])
        np.testing.assert_array_equal(inv.view(np.uint32), want.view(np.uint32))
    moved = False
    for prm in ({}, {"keep_outliers": 1}, {"max_rounds": 1}):
        seq.refine_map(**prm)
        got = [seq.refined_map(k) for k in range(n)]
        for k in range(n):
            _assert_refined_equal(got[k], _standalone(native, C, seq, [k], **prm), "%s %s segment %d" % (name, prm, k))
            moved |= bool((got[k][0].view(np.uint32) != seq.map(k)[0].view(np.uint32)).any())
        allx, alls = _standalone(native, C, seq, range(n), **prm)
        np.testing.assert_array_equal(np.concatenate([g[0] for g in got]).view(np.uint32), allx.view(np.uint32))
        for f in alls:
            np.testing.assert_array_equal(np.concatenate([g[1][f] for g in got]).view(np.uint32), alls[f].view(np.uint32))
    assert moved  # the refinement did something
    seq.close()


# ---- 6. the refinement changes nothing else

def test_refinement_leaves_the_run_alone(native):
    C = _case("seg8")
    n = len(C["first"])
    ref = _gpu(native, "seg8")
    seq = _open(native, C)
    seq.run()
    seq.refine_map()
    first = [seq.refined_map(k) for k in range(n)]
    _assert_same_results(ref, _results(seq, n), "after refine_map")
    seq.refine_map()
    for k in range(n):
        _assert_refined_equal(seq.refined_map(k), first[k], "second refine_map, segment %d" % k)
    b_us, r_us = seq.refine_time(2)
    assert b_us > 0 and r_us > 0
    for k in range(n):
        _assert_refined_equal(seq.refined_map(k), first[k], "after refine_time, segment %d" % k)
    _assert_same_tracks(ref["tracks"], [seq.tracks(k) for k in range(n)], "after refine_time")
    seq.run()
    _assert_same_results(ref, _results(seq, n), "a run after refine_map")
    _assert_same_tracks(ref["tracks"], [seq.tracks(k) for k in range(n)], "a run after refine_map")
    seq.close()


# ---- 7. errors

def test_errors_and_recovery(native):
    C = _case("seg8")
    n = len(C["first"])
    ref = _gpu(native, "seg8")

    def raises(code, fn, *a, **kw):
        with pytest.raises(native.PicpError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    def works(seq):
        seq.run()
        _assert_same_tracks(ref["tracks"], [seq.tracks(k) for k in range(n)], "after an error")

    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    seq.run()
    raises(native.ERR_STATE, seq.tracks, 0)      # the log is off
    raises(native.ERR_STATE, seq.refine_map)
    raises(native.ERR_STATE, seq.poses_wc)
    seq.track_log(True)
    raises(native.ERR_STATE, seq.tracks, 0)      # no run since it was switched on
    raises(native.ERR_STATE, seq.refine_map)
    raises(native.ERR_STATE, seq.refine_time, 1)
    works(seq)
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)
    raises(native.ERR_STATE, seq.tracks, 0)      # no run since set_segments
    raises(native.ERR_STATE, seq.refine_map)
    works(seq)
    raises(native.ERR_STATE, seq.refined_map, 0)  # before any refine_map
    works(seq)
    raises(native.ERR_ARG, seq.tracks, n)        # segment out of range
    raises(native.ERR_ARG, seq.tracks, -1)
    seq.refine_map()
    raises(native.ERR_ARG, seq.refined_map, n)
    raises(native.ERR_ARG, seq.refine_time, 0)
    works(seq)
    raises(native.ERR_STATE, seq.refined_map, 0)  # the run made the last refinement stale
    seq.refine_map()
    assert len(seq.refined_map(0)[0]) == len(ref["map"][0][0])
    seq.close()


# ---- 8. the guard pads

@pytest.mark.parametrize("name", ["seg8", "tails_seg"])
def test_guard_pads_intact(native, monkeypatch, name):
    monkeypatch.setenv("PICP_VO_GUARD", "1")
    C = _case(name)
    seq = _open(native, C, log=False)
    monkeypatch.delenv("PICP_VO_GUARD")
    seq.track_log(True)
    seq.run()
    for k in range(len(C["first"])):
        seq.tracks(k)
    seq.refine_map()
    seq.refine_time(1)
    bad, buf = ctypes.c_int64(-1), ctypes.c_int(0)
    assert native.lib().picp_vo_debug_guard(seq._h, ctypes.byref(bad), ctypes.byref(buf)) == 0
    assert (bad.value, buf.value) == (0, -1)
    _assert_same_tracks(_gpu(native, name)["tracks"], [seq.tracks(k) for k in range(len(C["first"]))], "guarded")
    seq.close()
