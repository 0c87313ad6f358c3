"""bench.py --dump-outputs: the arrays the headline's last timed step returned, as float32 / float64 .npy files under 64 MB, the same
files from run to run so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _load_dir(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writer_samples_within_the_cap(tmp_path):
    """Stand-in results of 131 072 records at list size 16 (more than the cap holds in full; every row carries its own index):
    only float32 / float64 files, under 64 MB together, the kept rows are the source rows named by records.npy / records_wide.npy,
    and the same results give the same files."""
    import torch
    import bench
    B, L = 131072, 16
    idx = torch.arange(B)
    sy = types.SimpleNamespace(y=idx.double()[:, None].expand(B, 2048), thr=idx.double() / 7, peaks=(idx % 2048).int()[:, None].expand(B, 32),
                               npeaks=(idx | (1 << 30)).int(), flags=(idx % 2).to(torch.uint8))
    scl = types.SimpleNamespace(hard_info=(idx % 256).to(torch.uint8)[:, None].expand(B, 55), hard_ok=(idx % 2).to(torch.uint8),
                                cand_info=(idx % 256).to(torch.uint8)[:, None, None].expand(B, L, 55), cand_metric=idx.double()[:, None].expand(B, L),
                                cand_ok=(idx % 2).to(torch.uint8)[:, None].expand(B, L), ncand=(idx % 9).int())
    scl.selected = ((idx % 256).to(torch.uint8)[:, None].expand(B, 55), (idx % 4 - 2).to(torch.int8), (idx % 8).int())
    llr = idx.float()[:, None].expand(B, 1024)
    bench.dump_outputs(str(tmp_path / "a"), sy, llr, scl)
    bench.dump_outputs(str(tmp_path / "b"), sy, llr, scl)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) <= 64 * 10 ** 6
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a.keys() == b.keys() and all(np.array_equal(a[f], b[f]) for f in a)
    rows, wide = a["records.npy"].astype(np.int64), a["records_wide.npy"].astype(np.int64)
    assert 0 < rows.size < B and np.all(np.diff(rows) > 0) and np.all(np.diff(wide) > 0)
    assert np.array_equal(a["sync_npeaks.npy"], (rows | (1 << 30)).astype(np.float64))
    assert np.array_equal(a["payload.npy"], np.repeat((rows % 256)[:, None], 55, axis=1).astype(np.float32))
    assert np.array_equal(a["scl_cand_metric.npy"][:, 0], rows.astype(np.float64))
    assert np.array_equal(a["sync_y.npy"][:, 0], wide.astype(np.float64)) and np.array_equal(a["llr.npy"][:, -1], wide.astype(np.float32))
    assert a["scl_cand_info.npy"].shape == (wide.size, L, 55)


@pytest.mark.gpu
def test_dumped_outputs_repeat_across_runs_and_step_counts(tmp_path):
    """Two runs at a small size with different --steps decode the same windows: identical files, every record kept, and the dump
    agrees with the JSON line (frames with CRC ok)."""
    common = ["--gpus", "1", "--warmup", "1", "--windows", "4096", "--legs", "none", "--no-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    lines = []
    for steps, d in ((2, "a"), (4, "b")):
        p = subprocess.run([sys.executable, BENCH, "--steps", str(steps), "--dump-outputs", str(tmp_path / d)] + common, env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert [j["steps"] for j in lines] == [2, 4] and all(j["ms_per_step"] > 0 for j in lines)
    a, b = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert a.keys() == b.keys() and {"payload.npy", "ok.npy", "llr.npy", "sync_peaks.npy", "scl_cand_info.npy"} <= a.keys()
    assert all(x.dtype in (np.float32, np.float64) and x.dtype == b[f].dtype and np.array_equal(x, b[f]) for f, x in a.items())
    assert np.array_equal(a["records.npy"], np.arange(4096, dtype=np.float64))
    assert int((a["ok.npy"] == 1).sum()) == lines[0]["config"]["frames_with_crc_ok"]
