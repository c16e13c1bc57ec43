"""GPU tests of picp_vo_adjust: the alternating adjustment on a VO run's own tracks, poses and maps.

It is the standalone refiner's adjustment on the same inputs (PointRefiner.adjust is held to the
float64 reference by test_gpu_adjust.py), so it is compared with it bit for bit; everything else
checks that it leaves the run, the tracks and picp_vo_refine_map alone.
"""
import ctypes

import numpy as np
import pytest

import adjust_ref as AR
from test_gpu_vo_tracks import (THR, _assert_refined_equal, _assert_same_results, _assert_same_tracks, _case,
                                _clean_env, _open, _results)

pytestmark = pytest.mark.gpu

PRM = dict(sweeps=2, points=AR.POINTS, poses=AR.POSES)


def _standalone_adjust(native, C, seq, **prm):
    """PointRefiner.adjust on the tracks, poses_wc and maps of all segments of an open handle, slot 0
    of every segment fixed (the pattern of test_gpu_vo_tracks._standalone)."""
    n = len(C["first"])
    slot0 = np.concatenate([[0], np.cumsum(C["steps"].astype(np.int64) + 1)])
    offs, poses, uvs, xyz, base = [np.zeros(1, np.int64)], [], [], [], 0
    for k in range(n):
        off, slot, idx = seq.tracks(k)
        offs.append(base + off[1:])
        base += int(off[-1])
        poses.append(slot0[k] + slot)
        uvs.append(C["uv"][idx].reshape(-1, 2))
        xyz.append(seq.map(k)[0])
    fixed = np.zeros(int(slot0[-1]), bool)
    fixed[slot0[:-1]] = True
    R = native.PointRefiner(K=C["K"])
    R.set_poses(np.concatenate(seq.poses_wc()))
    R.set_tracks(np.concatenate(offs), np.concatenate(poses).astype(np.int32), np.concatenate(uvs))
    R.set_points(np.concatenate(xyz))
    R.set_fixed_poses(fixed)
    R.adjust(**prm)
    out = R.points(), R.stats(), R.poses()
    R.close()
    return out


def _adjusted(seq, n):
    return [seq.adjusted_map(k) for k in range(n)], seq.adjusted_poses_wc()


@pytest.mark.parametrize("name", ["seg8", "tails_seg"])
def test_vo_adjust_equals_the_standalone_adjustment(native, name):
    C = _case(name)
    n = len(C["first"])
    seq = _open(native, C)
    seq.run()
    before = _results(seq, n)
    tracks = [seq.tracks(k) for k in range(n)]
    seq.refine_map()
    refined = [seq.refined_map(k) for k in range(n)]
    start_wc = seq.poses_wc()
    seq.adjust(**PRM)
    maps, poses = _adjusted(seq, n)
    X, st, T = _standalone_adjust(native, C, seq, **PRM)
    np.testing.assert_array_equal(np.concatenate([m[0] for m in maps]).view(np.uint32), X.view(np.uint32))
    for f in st:
        np.testing.assert_array_equal(np.concatenate([m[1][f] for m in maps]).view(np.uint32), st[f].view(np.uint32))
    np.testing.assert_array_equal(np.concatenate(poses).view(np.uint32), T.view(np.uint32))
    moved = False
    for k in range(n):  # slot 0 is the segment's world frame; later slots move
        np.testing.assert_array_equal(poses[k][0].view(np.uint32), start_wc[k][0].view(np.uint32))
        moved |= bool((poses[k][1:].view(np.uint32) != start_wc[k][1:].view(np.uint32)).any())
    assert moved
    # the run, its tracks and a fresh refine_map keep their bits
    _assert_same_results(before, _results(seq, n), "after adjust")
    _assert_same_tracks(tracks, [seq.tracks(k) for k in range(n)], "after adjust")
    for k in range(n):
        np.testing.assert_array_equal(seq.poses_wc()[k].view(np.uint32), start_wc[k].view(np.uint32))
    seq.refine_map()
    for k in range(n):
        _assert_refined_equal(seq.refined_map(k), refined[k], "refine_map after adjust, segment %d" % k)
    # a second adjust repeats the first
    seq.adjust(**PRM)
    maps2, poses2 = _adjusted(seq, n)
    for k in range(n):
        _assert_refined_equal(maps2[k], maps[k], "second adjust, segment %d" % k)
        np.testing.assert_array_equal(poses2[k].view(np.uint32), poses[k].view(np.uint32))
    # and a later run is the same run
    seq.run()
    _assert_same_results(before, _results(seq, n), "a run after adjust")
    with pytest.raises(native.PicpError) as e:
        seq.adjusted_map(0)  # the run made the adjustment stale
    assert e.value.code == native.ERR_STATE
    seq.close()


def test_state_errors(native):
    C = _case("seg8")
    seq = native.VOSequence(C["frame_off"], C["uv"], C["desc"], K=C["K"])
    seq.set_segments(C["first"], C["steps"], C["boot"], threshold=THR)

    def raises(code, fn, *a, **kw):
        with pytest.raises(native.PicpError) as e:
            fn(*a, **kw)
        assert e.value.code == code, (e.value.code, code)

    raises(native.ERR_STATE, seq.adjust)           # the log is off, no run
    seq.run()
    raises(native.ERR_STATE, seq.adjust)           # the log is off
    seq.track_log(True)
    raises(native.ERR_STATE, seq.adjust)           # no run since it was switched on
    raises(native.ERR_STATE, seq.adjusted_poses_wc)
    seq.run()
    raises(native.ERR_STATE, seq.adjusted_map, 0)  # before any adjust
    raises(native.ERR_ARG, seq.adjust, sweeps=-1)
    seq.adjust(sweeps=1)
    raises(native.ERR_ARG, seq.adjusted_map, len(C["first"]))
    assert len(seq.adjusted_map(0)[0]) == len(seq.map(0)[0])
    seq.close()


@pytest.mark.parametrize("name", ["seg8", "tails_seg"])
def test_guard_pads_intact(native, monkeypatch, name):
    monkeypatch.setenv("PICP_VO_GUARD", "1")
    C = _case(name)
    seq = _open(native, C, log=False)
    monkeypatch.delenv("PICP_VO_GUARD")
    seq.track_log(True)
    seq.run()
    seq.adjust(**PRM)
    seq.refine_map()
    seq.adjust(sweeps=1)
    bad, buf = ctypes.c_int64(-1), ctypes.c_int(0)
    assert native.lib().picp_vo_debug_guard(seq._h, ctypes.byref(bad), ctypes.byref(buf)) == 0
    assert (bad.value, buf.value) == (0, -1)
    seq.close()
