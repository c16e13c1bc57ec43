"""Small VO sequences run on the device against the build before the segment layout became a plan.

The cases and how one is run are in tools/vo_plan_golden.py, which also writes the golden file:
three segments of unequal steps, two of them overlapping; the same with an empty frame inside a
segment; frames of a little over 1,024 observations (npt 2, steps whose correspondences past
2 * 512 take the block kernel's streamed remainder); and a single segment.  Each runs under the
default schedule, the serial order (PICP_VO_OVERLAP=0 PICP_VO_CHAINS=1) and with the world match
split by map age (PICP_VO_SPLIT=1), the track log and the guard pads (PICP_VO_GUARD=1) on.

Every run is held, bit for bit, to tests/golden/vo_plan/parent.npz, written with the build before
csrc/picp_vo_plan.cpp (the plan changes no kernel, no kernel argument and no device byte):
picp_vo_info's four numbers, the poses and step records, every segment's map (count, xyz,
descriptors), its tracks, the world-in-camera pose table, the picp_vo_refine_map result (points
and stats), and no bad guard byte.  The recording holds the default schedule's arrays; writing it
asserted that the other two schedules of that build gave the same bits.

The picp_vo_adjust outputs go through an internal batch whose layout scales with the device's CU
count (tests/test_gpu_layout.py's rule), so they are compared where the CU count equals the
recorded one; tests/test_gpu_vo_adjust.py holds them on any device.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "vo_plan", "parent.npz")

_spec = importlib.util.spec_from_file_location("vo_plan_golden", os.path.join(ROOT, "tools", "vo_plan_golden.py"))
VG = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(VG)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN_FILE) as g:
        return {k: g[k] for k in g.files}


@pytest.mark.parametrize("schedule", list(VG.SCHEDULES))
@pytest.mark.parametrize("name", list(VG.CASES))
def test_vo_case_matches_the_build_before_the_plan(native, golden, name, schedule):
    got = VG.run_case(native, name, schedule)
    n_seg = len(VG.CASES[name][2])
    print(name, schedule, "info", got["info"].tolist(), "n_corr", got["steps"][:, 0].tolist(), "map",
          [len(got["map_xyz/%d" % k]) for k in range(n_seg)], "guard", got["guard"].tolist())
    assert got["guard"].tolist() == [0, -1]  # no bad pad byte, no bad pad
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert set(want) == set(got), sorted(set(want) ^ set(got))
    same_cus = int(golden["num_cu"]) == VG.num_cu()
    VG.assert_same(got, want, "%s %s" % (name, schedule), skip=() if same_cus else ("adj_",))
