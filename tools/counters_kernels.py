"""The two kernels of counter origins alone, at the size of a live identification tick: 16 keys, 64 streams (256 band rows),
5 s windows (hop rows of 600 counters).  es_hop_window_batch, RxEngine.plan through es_plan_at_batch (its four small uploads included) and,
for scale, through es_plan_ragged_batch; every call between two events, medians of 20 with min and max.

    python tools/counters_kernels.py [--out profiles/counters_kernels.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoseal_amd.engine import RxEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
out = ap.parse_args().out
eng = RxEngine(0, fs=48_000)
rng = np.random.default_rng(0)
N, S, W = 16, 64, 240_000
C = -(-W // 1215) + 402
ring = eng.keyring([rng.bytes(32) for _ in range(N)])
bases = (70_000 + 1000 * np.arange(S) + 5000).astype(np.int64)
rows = 4 * S
peaks = np.sort(rng.integers(0, W - 1215, (rows, 32)), axis=1).astype(np.int32)
npeaks = np.full(rows, 25, np.int32)
P = rows * 25
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
pk, npk = d(peaks), d(npeaks)
hok, hlo = torch.zeros((N, P), dtype=torch.uint8, device=eng.device), torch.zeros((N, P), dtype=torch.int32, device=eng.device)
base = (25 * np.arange(rows)).astype(np.int32)
rowband = np.tile(np.arange(4, dtype=np.uint8), S)
pos0 = np.repeat(np.full(S, 1216 * 5000, np.int64), 4); ctr0 = np.repeat(70_000 + 1000 * np.arange(S), 4)
hb = np.maximum(0, 70_000 + 1000 * np.arange(S) + (2 * 1216 * 5000 + 1215) // 2430 - 200)
def timed(fn, reps=20):
    out = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); out.append(a.elapsed_time(b))
    out = out[3:]
    return r, {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}
hop, t_hop = timed(lambda: eng.hop_window(ring, hb, C))
_, t_plan = timed(lambda: eng.plan(pk, npk, rowband, base, np.full(rows, W, np.int32), hok, hlo, hop, pos0=pos0, ctr0=ctr0, hop_row=np.repeat(np.arange(S), 4), hop_base=hb))
hop0 = hop[:, 0].contiguous()
_, t_rag = timed(lambda: eng.plan(pk, npk, rowband, base, np.full(rows, W, np.int32), hok, hlo, hop0))
row = {"keys": N, "streams": S, "C": C, "hop_window_entries": N * S * C, "hop_window": t_hop, "plan_at_with_uploads": t_plan, "plan_ragged_with_uploads": t_rag}
print(json.dumps(row))
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(json.dumps(row) + "\n")
