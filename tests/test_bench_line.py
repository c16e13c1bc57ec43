"""The bench line's shape (CPU, no device): the driver keeps only the tail of stdout (about 2,000
characters), so the one JSON line must carry every sub-result's numbers in well under that, with
the contract's keys first; the C5 rounds-sync figure's arithmetic; --dump-outputs; and (GPU) a
plain run of the benchmark end to end."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as B
    return B


def test_compact_line_fits_the_driver_tail(bench):
    detail = os.path.join(ROOT, "profiles", "r06", "final", "bench_detail_a.json")
    out = json.load(open(detail))
    line = json.dumps(bench.compact_line(out, "gpurun_out/bench_detail_c2_n1.json"), separators=(",", ":"))
    assert len(line) < 1950, len(line)
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert list(d)[:2] == ["metric", "value"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    # every config's numbers: C3, C4 with its projections, C5 led by the 8e partition with its side figures
    assert {"c3", "c4", "c5", "stream16m"} <= set(d)
    assert {"n2", "n4", "n8"} <= set(d["c4"]["proj_eff"])
    assert {"essential_boot", "gt_anchored_250", "rounds_sync", "per_rank_n8", "proj_eff_n8"} <= set(d["c5"])


def test_dump_outputs_writes_float_arrays(bench, tmp_path):
    import argparse

    import numpy as np
    d = tmp_path / "dump"
    args = argparse.Namespace(dump_outputs=str(d))
    stats = [{"chi_in": 1.5, "chi_out": 0.0, "n_in": 99, "ok": 1, "rounds": 50, "converged": 0, "n_projected": 100}]
    bench.dump_outputs(args, bench._Solo(), {"poses": np.eye(4, dtype=np.float32)[None],
                                             "stats": bench._stats_rows(stats), "counts": np.arange(3)})
    poses, st, counts = (np.load(d / (n + ".npy")) for n in ("poses", "stats", "counts"))
    assert poses.dtype == np.float32 and poses.shape == (1, 4, 4)
    assert st.dtype == np.float64 and st.tolist() == [[1.5, 0.0, 99.0, 1.0, 50.0, 0.0, 100.0]]
    assert counts.dtype == np.float32 and counts.tolist() == [0.0, 1.0, 2.0]
    # no directory given: nothing is written; more than the limit: an error, not a silent cut
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), bench._Solo(), {"x": np.zeros(1)})
    assert sorted(p.name for p in d.iterdir()) == ["counts.npy", "poses.npy", "stats.npy"]
    with pytest.raises(ValueError):
        bench.dump_outputs(args, bench._Solo(), {"big": np.zeros(bench.DUMP_LIMIT // 8 + 1)})


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_solve(tmp_path):
    """A plain run: exactly --steps timed steps in one region, the contract's keys, none of the
    --full legs, no side file; --dump-outputs holds the timed frame's pose and statistics."""
    import subprocess

    import numpy as np
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup",
                        "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["detail"] is None
    assert line["metric"] == "PICP iterations/sec @ 100000 correspondences" and line["unit"] == "iterations/s"
    # value and ms_per_step describe the same region: 50 rounds per step
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 50.0 - 1.0) < 1e-3
    assert not {"cpu_baseline", "c3", "c4", "c5", "stream16m", "with_conv_its"} & set(line)
    poses, st = np.load(d / "poses.npy"), np.load(d / "stats.npy")
    assert poses.dtype == np.float32 and poses.shape == (1, 4, 4) and st.shape == (1, 7)
    assert np.array_equal(poses[0, 3], [0, 0, 0, 1]) and np.isfinite(poses).all()
    assert st[0, 3] == 1 and st[0, 4] == 50  # ok, 50 rounds run
    # the dumped pose is the seeded frame's solution: 0.5 px noise at focal 180 over 1e5 points puts
    # the estimate within ~1e-5..1e-4 of the ground truth (SE(3) log); any other frame is > 1e-2 away
    sys.path.insert(0, os.path.join(ROOT, "02-visualodometry_amd"))
    from picp_amd import synth
    p = synth.make_problem(100000, seed=42, outlier_frac=0.0, pixel_noise=0.5, shuffle=False)
    assert synth.se3_log_norm(poses[0], p["T_gt"]) < 1e-3


def test_rounds_sync(bench):
    # two chains of two segments; chain 0's per-step maxima: 5 + 9 = 14, chain 1's: 7 + 3 = 10; the
    # slowest segment alone: 2 + 9 = 11 (segment 1) -> ratio 14 / 11
    r = bench._rounds_sync([[5, 1], [2, 9], [7, 2], [3, 3]])
    assert r["sum_t_max_s"] == 14 and r["max_s_sum_t"] == 11 and r["chains"] == 2
    assert abs(r["ratio"] - round(14 / 11, 4)) < 1e-12
    r1 = bench._rounds_sync([[50, 50, 10]])  # one segment: no synchronisation cost
    assert r1["ratio"] == 1.0 and r1["steps_at_50_any"] == 2
