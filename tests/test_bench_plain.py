"""bench.py without --full runs the headline alone (no sequential check pass, no legs, no roofline objects that need a run of
their own, no CPU baseline); --full adds them and leaves the headline's steps and outputs as they are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_legs_need_full():
    import bench
    a = bench.parse_args([])
    assert not a.full and a.legs == "auto"
    assert not bench.parse_args(["--legs", "none"]).full
    assert bench.parse_args(["--full", "--legs", "c2,c4"]).legs == "c2,c4"
    with pytest.raises(SystemExit):
        bench.parse_args(["--legs", "c2,c4"])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_full_keeps_it(tmp_path):
    """A plain run and a --full run without legs at a small size: the plain line carries the headline and none of what moved behind
    --full, and both runs dump the same arrays."""
    common = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--windows", "4096"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    lines = []
    for extra, d in (([], "plain"), (["--full", "--legs", "none", "--no-cpu-baseline"], "full")):
        p = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path / d)] + common + extra, env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    plain, full = lines
    for j in lines:
        assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
        assert j["unit"] == "frames/s" and j["higher_is_better"] is True and j["dtype"] == "f64" and j["legs"] == {}
    assert not {"roofline", "roofline_fused", "cpu_baseline"} & plain.keys()
    assert not {"stage_ms_one_step_alone", "results_identical_to_a_sequential_pass"} & plain["config"].keys()
    assert full["config"]["results_identical_to_a_sequential_pass"] and full["roofline"]["on_headline_path"]
    for k in ("frames_through_list_decoder", "frames_with_crc_ok", "windows_with_a_top5_peak_within_2_samples_of_the_true_offset"):
        assert plain["config"][k] == full["config"][k], k
    a, b = (sorted(os.listdir(tmp_path / d)) for d in ("plain", "full"))
    assert a == b and "payload.npy" in a
    assert all(np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)) for f in a)
