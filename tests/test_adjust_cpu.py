"""CPU tests of the reference of the alternating adjustment (tests/adjust_ref.py): it converges, its
gate decisions are not borderline, and the float32 / float64 distances the GPU tolerance is derived
from (tests/test_gpu_adjust.py D_X, D_T) are the recorded ones.  No GPU.
"""
import numpy as np
import pytest

import adjust_ref as AR
import test_gpu_adjust as G

CASES = ("data_perturbed", "synth")


@pytest.mark.parametrize("name", CASES)
def test_inlier_chi2_falls_at_every_half_step(oracle, name):
    C = AR.case(oracle, name)
    h = AR.half_steps(C, AR.reference(oracle, name, 3))
    print(name, ["%.6g" % v for v in h])
    assert len(h) == 7
    for a, b in zip(h, h[1:]):
        assert b < a, h
    assert h[-1] < 0.05 * h[0]


def test_data_case_is_the_measured_one(oracle):
    """396 points, 121 poses, 9,640 observations; the summed inlier chi2 starts at 707,922 and six
    sweeps bring it to 161, the worst camera centre from 7.3 cm to 1.2 cm off the ground truth, the
    median point to 7.0 mm."""
    C = AR.case(oracle, "data_perturbed")
    assert (len(C["start"]), len(C["poses"]), len(C["obs_pose"])) == (396, 121, 9640)
    run = AR.reference(oracle, "data_perturbed", 6)
    h = AR.half_steps(C, run)
    assert abs(h[0] - 707922) < 1 and abs(h[-1] - 161) < 1, (h[0], h[-1])

    def worst(P):
        c = lambda T: np.linalg.inv(np.asarray(T, np.float64))[:3, 3]
        return max(np.linalg.norm(c(a) - c(b)) for a, b in zip(P, C["truth_poses"]))

    assert 0.07 < worst(C["poses"]) < 0.08 and worst(run[-1]["poses"]) < 0.013
    assert np.median(np.linalg.norm(run[-1]["X"] - C["truth"], axis=1)) < 0.008


@pytest.mark.parametrize("name", CASES)
def test_borderline_points_are_rare(oracle, name):
    for s in AR.reference(oracle, name, 3):
        assert s["border"].sum() <= G.BORDERLINE_CAP * len(s["X"]), s["border"].sum()


@pytest.mark.parametrize("name", CASES)
def test_recorded_distances_are_the_measured_ones(oracle, name):
    d = AR.distances(AR.reference(oracle, name, 3, "f32"), AR.reference(oracle, name, 3, "f64"))
    for sweeps in (1, 3):
        dx, dt = d[sweeps - 1]
        print("%s sweeps=%d D_X=%.3g D_T=%.3g" % (name, sweeps, dx, dt))
        assert abs(dx - G.D_X[name][sweeps]) <= 0.1 * G.D_X[name][sweeps], (dx, G.D_X[name][sweeps])
        assert abs(dt - G.D_T[name][sweeps]) <= 0.1 * G.D_T[name][sweeps], (dt, G.D_T[name][sweeps])


@pytest.mark.parametrize("name", CASES)
def test_inlier_counts_agree_between_the_classes(oracle, name):
    a, b = AR.record_sums(AR.reference(oracle, name, 3, "f32")), AR.record_sums(AR.reference(oracle, name, 3, "f64"))
    for x, y in zip(a, b):
        assert (x["n_in_points"], x["n_in_poses"]) == (y["n_in_points"], y["n_in_poses"])
    if name == "data_perturbed":
        assert (b[0]["n_in_points"], b[0]["n_in_poses"]) == (9561, 9491)
        assert (b[2]["n_in_points"], b[2]["n_in_poses"]) == (9626, 9514)


def test_view_reference_on_the_tiny_case(oracle):
    C = AR.case(oracle, "tiny")
    off, pt, uv = AR.pose_view(3, C["off"], C["obs_pose"], C["obs_uv"])
    np.testing.assert_array_equal(off, [0, 3, 5, 5])
    np.testing.assert_array_equal(pt, [0, 2, 2, 0, 2])  # pose 0 sees point 2 twice, in track order
    np.testing.assert_array_equal(uv[[1, 2]], C["obs_uv"][[2, 4]])
    np.testing.assert_array_equal(AR.movable_poses(C), [0, 1])
