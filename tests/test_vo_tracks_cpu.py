"""CPU tests of the VO sequence's observation tracks: the numpy reference (tests/vo_tracks_ref.py)
on an example small enough to write its answer out, and the new entry points' behaviour without a
device."""
import ctypes

import numpy as np
import pytest

import vo_tracks_ref


def _example():
    """Three frames, one segment of two steps, descriptors (value, 10 * group): squared distances
    inside a group decide, the groups are 100 apart.

      frame 0: A0 = 0, P0 = .62                    observations 0, 1
      frame 1: P1 = .7, A1 = .3, Q1 = 0 (group 1)  observations 2, 3, 4
      frame 2: P2a = .63, Q2 = .1 (group 1), P2b = .61   observations 5, 6, 7

    bootstrap (0 -> 1): A0 -> A1 (.09; second P1 .49) and P0 -> P1 (.0064; second A1 .1024): points
      0 = (x 0, y 3) and 1 = (x 1, y 2).
    step 0, frame 1 against {A0, P0}: P1 -> point 1 (.0064 / .49): the point's own y, not counted
      twice; A1 is rejected (A0 .09 / P0 .1024 = .88 > .8); Q1 is 100 away.  The pairs of (0 -> 1)
      whose frame-1 observation has no map match: (A0, A1) again -> point 2 = (x 0, y 3), c = 0.
    step 1, frame 2 against {A0, P0, A0}: P2a -> point 1 and P2b -> point 1 (.0001 each): one point
      matched twice from one frame; Q2 is 100 away.  The pairs of (1 -> 2): P1 -> P2a (.0049 /
      .0081 = .6; P2a has a map match: dropped), A1 rejected (P2b .0961 / P2a .1089 = .88),
      Q1 -> Q2 (.01; no map match) -> point 3 = (x 4, y 6), c = 1."""
    d = lambda v, g=0: [v, 10.0 * g]
    frames = [[d(0.0), d(0.62)], [d(0.7), d(0.3), d(0.0, 1)], [d(0.63), d(0.1, 1), d(0.61)]]
    desc = np.array([r for f in frames for r in f], np.float32)
    off = np.array([0, 2, 5, 8], np.int64)
    map_desc = desc[[0, 1, 0, 4]]
    n_new = [2, 1, 1]
    return off, desc, map_desc, n_new


def test_reference_tracks_on_a_written_out_example(oracle):
    off, desc, map_desc, n_new = _example()
    r = vo_tracks_ref.reference_tracks(oracle, off, desc, 0, 2, map_desc, n_new)
    np.testing.assert_array_equal(r["track_off"], [0, 2, 6, 8, 10])
    np.testing.assert_array_equal(r["obs_index"], [0, 3, 1, 2, 5, 7, 0, 3, 4, 6])
    np.testing.assert_array_equal(r["obs_slot"], [0, 1, 0, 1, 2, 2, 0, 1, 1, 2])
    np.testing.assert_array_equal(r["own_y"], [False, True, False, False])
    assert r["track_off"].dtype == np.int64 and r["obs_index"].dtype == np.int64 and r["obs_slot"].dtype == np.int32
    # the step's matches as the helper saw them: step 0 accepts only P1, step 1 both P2a and P2b
    np.testing.assert_array_equal(r["wm"][0][0], [True, False, False])
    np.testing.assert_array_equal(r["wm"][1][0], [True, False, True])
    assert r["wm"][0][1][0] == 1 and r["wm"][1][1][0] == 1 and r["wm"][1][1][2] == 1


def test_reference_tracks_checks_the_step_records(oracle):
    off, desc, map_desc, _ = _example()
    with pytest.raises(AssertionError):
        vo_tracks_ref.reference_tracks(oracle, off, desc, 0, 2, map_desc, [2, 0, 2])


def test_null_handles_are_rejected_without_device():
    import picp_amd
    L = picp_amd.lib()
    n, m = ctypes.c_int64(0), ctypes.c_int64(0)
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    T = (ctypes.c_float * 16)()
    assert L.picp_vo_set_track_log(None, 1) == picp_amd.ERR_ARG
    assert L.picp_vo_get_tracks(None, 0, None, None, None, ctypes.byref(n), ctypes.byref(m)) == picp_amd.ERR_ARG
    assert L.picp_vo_get_poses_wc(None, T) == picp_amd.ERR_ARG
    assert L.picp_vo_refine_map(None, None) == picp_amd.ERR_ARG
    assert L.picp_vo_get_refined_map(None, 0, 0, None, None, ctypes.byref(n)) == picp_amd.ERR_ARG
    assert L.picp_vo_refine_time(None, None, 1, ctypes.byref(a), ctypes.byref(b)) == picp_amd.ERR_ARG
    assert L.picp_last_error()


def test_python_wrappers_exist():
    import picp_amd
    for name in ("track_log", "tracks", "poses_wc", "refine_map", "refined_map", "refine_time"):
        assert callable(getattr(picp_amd.VOSequence, name)), name
    assert picp_amd.lib().picp_abi_version() == 3  # new symbols only
