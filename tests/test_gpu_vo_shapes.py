"""The device-resident VO step at the frame sizes where the driver changes its code path, and on
empty and near-empty steps, against the CPU oracle.

The schedules are tests/vo_shapes.py's (its table: max_obs, npt, fused or not);
tests/test_vo_shapes_cpu.py proves on the oracle which sizes and which cases each one holds (a
step with an empty query frame, with no or one correspondence, with nothing to append, with
world matches and selected pairs past observation 4096, with more items than the block kernel's
registers and LDS stage).  The step checks and their bounds are tests/test_gpu_vo.py's
(_check_segment: pose < 1e-4, triangulation quantiles, residual constant 8).  On top of them:
  * counts, map size, map descriptors and the accept flags of both matches in EVERY step equal
    the free-running oracle's (matching only; the flags tie a count mismatch to the matcher or
    to the compaction);
  * n_in and rounds of every step equal the teacher-forced oracle solve's;
  * a step with no inlier (no correspondence, or none inside the inlier gate) leaves the pose as the reference's loop leaves it:
    inverse(inverse(previous pose)) in float32, bit for bit (the rotation keeps its bits, the
    translation may move by an ulp; test_vo_shapes_cpu.py shows the oracle does exactly this);
  * seq.info()["npt"] is the table's value;
  * poses, step records and maps keep their bits under the separate gather (PICP_VO_FUSE=0), the
    fused one where it applies (above 4,096 observations PICP_VO_FUSE=1 runs the separate
    kernels), the default concurrent schedule, two step chains and the world match split by map
    age (a zero-reference late part after a step that appended nothing, a zero-query part
    before an empty frame), and with the track counters on;
  * the library's own guard pads (PICP_VO_GUARD=1) are intact after a run.
"""
import ctypes

import numpy as np
import pytest

import vo_shapes as VS
from test_gpu_vo import THR, _assert_same_bits, _check_segment
from test_gpu_vo_track import _reference_counts

pytestmark = pytest.mark.gpu

ENV_KEYS = ("PICP_VO_FUSE", "PICP_VO_OVERLAP", "PICP_VO_CHAINS", "PICP_VO_SPLIT", "PICP_VO_GRAPH", "PICP_VO_GUARD",
            "PICP_VO_PHASE", "PICP_VO_MATCH_FULL")
SERIAL = {"PICP_VO_FUSE": "0", "PICP_VO_OVERLAP": "0", "PICP_VO_CHAINS": "1"}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)


def _run(native, name, track=False, guard=False, matches=False):
    S = VS.build(name)
    seq = native.VOSequence(S["frame_off"], S["uv"], S["desc"], K=S["K"])
    seq.set_segments(S["first"], S["steps"], S["boot"], threshold=THR)
    if track:
        seq.track_stats(True)
    seq.run()
    n = len(S["first"])
    out = {"poses": seq.poses(), "rec": seq.step_records(), "map": [seq.map(k) for k in range(n)],
           "npt": seq.info()["npt"]}
    if track:
        out["stats"] = [seq.map_stats(k) for k in range(n)]
    if matches:
        L = native.lib()
        out["matches"] = []
        for which in range(4):  # pm_bi, pm_acc, wm_bi, wm_acc, one row per observation
            dst = np.zeros(max(int(S["frame_off"][-1]), 1), np.int32)
            assert L.picp_vo_debug_matches(seq._h, which, dst.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
            out["matches"].append(dst)
    if guard:
        L = native.lib()
        bad, buf = ctypes.c_int64(-1), ctypes.c_int(0)
        assert L.picp_vo_debug_guard(seq._h, ctypes.byref(bad), ctypes.byref(buf)) == 0
        out["guard"] = (bad.value, buf.value)
    seq.close()
    return out


def _bits(o):
    return (o["poses"], o["rec"], o["map"])


_DEFAULT = {}


def _default(native, name):
    """The library default's run of a schedule, shared by the tests of this module."""
    if name not in _DEFAULT:
        _DEFAULT[name] = _run(native, name, matches=True)
    return _DEFAULT[name]


@pytest.mark.parametrize("name", VS.NAMES)
def test_counts_path_and_matches(native, name):
    S, refs, steps = VS.build(name), VS.reference(name), VS.oracle_steps(name)
    out = _default(native, name)
    assert out["npt"] == S["npt"]
    off = S["frame_off"]
    for k, ref in enumerate(refs):
        rec = out["rec"][k]
        what = "%s segment %d" % (name, k)
        np.testing.assert_array_equal(rec["n_corr"][1:], ref["n_corr"], err_msg=what)
        np.testing.assert_array_equal(rec["n_new"], ref["n_new"], err_msg=what)
        mx, md = out["map"][k]
        assert len(mx) == len(ref["map_xyz"]) == int(ref["n_new"].sum())
        np.testing.assert_array_equal(md, ref["map_desc"], err_msg=what)
    if len(refs) > 1:
        return  # overlapping segments rewrite each other's match rows
    pm_bi, pm_acc, wm_bi, wm_acc = out["matches"]
    for r in steps[0]:
        what = "%s step %d" % (name, r["t"])
        q, c = slice(off[r["nf"]], off[r["nf"] + 1]), slice(off[r["cf"]], off[r["cf"] + 1])
        acc = r["wm"]["accepted"]
        np.testing.assert_array_equal(wm_acc[q] != 0, acc, err_msg=what + " world match flags")
        np.testing.assert_array_equal(wm_bi[q][acc], r["wm"]["best_idx"][acc], err_msg=what + " world match index")
        if r["nq"] == 0:
            continue  # no frame->next problem is launched against an empty frame; nothing reads these rows
        acc = r["pm"]["accepted"]
        np.testing.assert_array_equal(pm_acc[c] != 0, acc, err_msg=what + " frame match flags")
        np.testing.assert_array_equal(pm_bi[c][acc], r["pm"]["best_idx"][acc], err_msg=what + " frame match index")


_FORCED = {}


def _forced(native, oracle, name):
    """Every segment of the default run through test_gpu_vo._check_segment (which asserts its
    bounds), once per schedule: -> per segment the oracle solve's n_in and rounds per step, the
    worst pose distance and the worst residual ratio."""
    if name not in _FORCED:
        S = VS.build(name)
        out = _default(native, name)
        res = []
        for k, (f0, st) in enumerate(zip(S["first"], S["steps"])):
            poses, rec = out["poses"][k], out["rec"][k]
            mx, md = out["map"][k]
            assert len(poses) == st + 1 and np.isfinite(poses).all() and np.isfinite(mx).all()
            stats = {}
            _check_segment(oracle, S["K"], S["frame_off"], S["uv"], S["desc"], int(f0), S["boot"][k][0],
                           S["boot"][k][1], poses, rec, mx, md, stats)
            res.append(stats)
        _FORCED[name] = res
    return _FORCED[name]


@pytest.mark.parametrize("name", VS.NAMES)
def test_every_step_teacher_forced(native, oracle, name):
    S = VS.build(name)
    out = _default(native, name)
    forced = _forced(native, oracle, name)
    for k in range(len(S["first"])):
        poses, rec = out["poses"][k], out["rec"][k]
        assert (rec["n_in"][1:][rec["n_corr"][1:] == 0] == 0).all()
        for t in np.nonzero(rec["n_in"][1:] == 0)[0]:  # no correspondence, or none inside the inlier gate
            twice = oracle.iso_inverse(oracle.iso_inverse(poses[t]))
            np.testing.assert_array_equal(poses[t + 1].view(np.uint32), twice.view(np.uint32),
                                          err_msg="%s segment %d step %d: no inlier" % (name, k, t))
            np.testing.assert_array_equal(poses[t + 1][:3, :3].view(np.uint32), poses[t][:3, :3].view(np.uint32))
    print("VO_SHAPE %s: max_obs %d npt %d %s, worst teacher-forced pose distance %.3g, worst residual ratio %.3g" % (
        name, S["max_obs"], out["npt"], "fused" if S["fused"] else "unfused", max(f["pose"] for f in forced),
        max(f["res"] for f in forced)))


@pytest.mark.parametrize("name", VS.NAMES)
def test_n_in_and_rounds_equal_the_oracle_solve(native, oracle, name):
    """Every step's inlier count and round count equal the teacher-forced oracle solve's, which
    starts from the device's own initial state (oracle.iso_inverse of the previous pose).

    The loop stops when chi_in changes by less than 1e-5 of itself (or the previous chi_in is
    below 1e-10).  The schedules keep that decision off the rounding floor of chi_in
    (vo_shapes.NOISE; test_vo_shapes_cpu.py test_round_counts_are_a_property_of_the_data): every
    step either has no inlier -- no update, two rounds -- or a noise level of chi_in five orders
    above the floor.  A step with ONE INLIER correspondence cannot be in them: its chi_in falls to
    9.3e-10, (an ulp of a pixel coordinate)^2, and the round at which that value repeats turns on
    the last bit of the map point (measured on an MI355X with such a step in fused8: GPU 5 rounds,
    oracle 6; from a float64-inverted start 5 and 5).  fused8's one-correspondence step therefore
    has its correspondence outside the inlier gate."""
    out = _default(native, name)
    forced = _forced(native, oracle, name)
    for k, f in enumerate(forced):
        rec = out["rec"][k]
        print("VO_SHAPE %s segment %d: n_corr %s; n_in gpu %s oracle %s; rounds gpu %s oracle %s" % (
            name, k, rec["n_corr"][1:].tolist(), rec["n_in"][1:].tolist(), f["n_in"], rec["rounds"][1:].tolist(),
            f["rounds"]))
    for k, f in enumerate(forced):
        np.testing.assert_array_equal(out["rec"][k]["n_in"][1:], f["n_in"], err_msg="%s segment %d n_in" % (name, k))
    for k, f in enumerate(forced):
        np.testing.assert_array_equal(out["rec"][k]["rounds"][1:], f["rounds"],
                                      err_msg="%s segment %d rounds" % (name, k))


@pytest.mark.parametrize("name", VS.NAMES)
def test_bit_identical_across_schedules(native, monkeypatch, name):
    """The serial order with the separate gather is the base; every other way of running the step
    gives its bits."""
    S = VS.build(name)
    envs = [dict(SERIAL), dict(SERIAL, PICP_VO_FUSE="1"), {}, dict(SERIAL, PICP_VO_SPLIT="1"), {"PICP_VO_SPLIT": "1"}]
    if len(S["first"]) > 1:
        envs += [dict(SERIAL, PICP_VO_CHAINS="2"), {"PICP_VO_CHAINS": "2", "PICP_VO_FUSE": "0"},
                 {"PICP_VO_CHAINS": "2", "PICP_VO_SPLIT": "1"}]
    base = None
    for env in envs:
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = _default(native, name) if not env else _run(native, name)
        assert out["npt"] == S["npt"]
        if base is None:
            base = out
        _assert_same_bits(_bits(base), _bits(out), "%s %s" % (name, env))


@pytest.mark.parametrize("name", VS.NAMES)
def test_guard_pads_intact(native, monkeypatch, name):
    """PICP_VO_GUARD=1 (read at create): every device buffer of the handle between two
    pattern-filled pads; no kernel of the run stored into one, and the results keep their bits."""
    monkeypatch.setenv("PICP_VO_GUARD", "1")
    out = _run(native, name, guard=True, track=name in ("tails", "fused8"))
    assert out["guard"] == (0, -1), "%s: %d pad bytes overwritten, first at pad %d" % ((name,) + out["guard"])
    monkeypatch.delenv("PICP_VO_GUARD")
    _assert_same_bits(_bits(_default(native, name)), _bits(out), name + " guarded")


@pytest.mark.parametrize("name", ["tails", "fused8", "tails_seg"])
def test_track_counters(native, oracle, name):
    """vo_track_kernel with nq > 4096, with empty problems and beside finished segments: the
    counters as tests/test_gpu_vo_track.py checks them, results unchanged."""
    S = VS.build(name)
    on = _run(native, name, track=True)
    _assert_same_bits(_bits(_default(native, name)), _bits(on), name + " tracking on")
    matches = amb_total = 0
    for k, f0 in enumerate(S["first"]):
        mx, md = on["map"][k]
        nm, ni = on["stats"][k]
        rec = on["rec"][k]
        assert len(nm) == len(mx) and len(ni) == len(mx)
        ref_m, ref_i, ref_amb, tot = _reference_counts(oracle, S["K"], S["frame_off"], S["uv"], S["desc"], int(f0),
                                                       on["poses"][k], rec, mx, md)
        np.testing.assert_array_equal(nm, ref_m)
        assert nm.sum() == rec["n_corr"][1:].sum()
        assert (ni >= 0).all() and (ni <= nm).all()
        diff = np.abs(ni.astype(np.int64) - ref_i)
        assert (diff <= ref_amb).all(), (int(diff.max()), int(ref_amb.max()))
        matches += tot["matches"]
        amb_total += int(ref_amb.sum())
    assert matches > 0 and amb_total <= 1e-3 * matches, (amb_total, matches)
