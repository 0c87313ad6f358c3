"""What acquisition costs.  The two planner calls alone at 8 records x the full 32-bit span, each between two device events
(medians of 20 with min and max); then, on a 5 s noise clip with frames embedded from counter 70 000, WatermarkDetector.acquire over the
full span at list size 8 and at list size 256 and, for scale, verify(..., ctr0=70 000) on the same clip -- host clock around calls that end
in a download, every repeat listed.  Also how often the header decode says ok on noise, which decides what an unmarked clip costs.

    python tools/acquire_time.py [--out profiles/acquire.json] [--budget-s 240]

The list-256 run at the default max_records is made only if the run at max_records = 1 predicts it inside the budget.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from echoseal_amd.acquire import FULL_SPAN  # noqa: E402
from echoseal_amd.detector import WatermarkDetector  # noqa: E402
from echoseal_amd.engine import RxEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--budget-s", type=float, default=240.0)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("acquire_time.py measures on the GPU: none found")
eng = RxEngine(0, list_size_max=256, fs=48_000)
KEY, ORIGIN = b"\x5C" * 32, 70_000
rng = np.random.default_rng(0)


def events(fn, reps=20):
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
    ms = ms[3:]
    return r, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def clocked(fn, reps):
    fn()                                                                    # warm-up of every shape the timed calls use
    s = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); s.append(time.perf_counter() - t)
    return r, {"median_s": statistics.median(s), "all_s": [round(v, 4) for v in s]}


# ---- the two planner calls alone: 8 records x 65 536 high halves
ring = eng.keyring([KEY])
P = 8
d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
key, ok = d(np.zeros(P, np.int32)), d(np.ones(P, np.uint8))
lo16, band = d(rng.integers(0, 65_536, P).astype(np.int32)), d(rng.integers(0, 4, P).astype(np.uint8))
(mask, count), t_mask = events(lambda: eng.acquire_mask(ring, key, ok, lo16, band, FULL_SPAN))
cnt = count.cpu().numpy().astype(np.int64)
base, total = d(np.cumsum(cnt) - cnt), int(cnt.sum())
_, t_list = events(lambda: eng.acquire_list(mask, lo16, FULL_SPAN, base, total))
row = {"records": P, "span": list(FULL_SPAN), "candidates": total, "acquire_mask": t_mask, "acquire_list": t_list}

# ---- the calls on a 5 s clip
host = (0.05 * rng.standard_normal((1, 240_000))).astype(np.float32)
clip = eng.embed(KEY, host, ctr0=ORIGIN, seed=1).audio[0].cpu().numpy()


def acquire_run(list_size, max_records, reps, audio=clip):
    det = WatermarkDetector(KEY, list_size=list_size, engine=eng)

    def call():
        det.session_nonce, det._trace = None, []
        return det.acquire(audio, 48_000, max_records=max_records)
    acq, t = clocked(call, reps)
    t.update(list_size=list_size, max_records=max_records, found=acq is not None, tried=len(det._trace),
             records=None if acq is None else acq.records, ctr0=None if acq is None else acq.ctr0)
    return t


def verify_run(list_size, reps):
    det = WatermarkDetector(KEY, list_size=list_size, engine=eng)

    def call():
        det.session_nonce, det._trace = None, []
        return det.verify(clip, 48_000, ctr0=ORIGIN)
    okv, t = clocked(call, reps)
    t.update(list_size=list_size, verified=bool(okv), tried=len(det._trace))
    return t


row["verify_known_origin"] = [verify_run(8, 5), verify_run(256, 3)]
row["acquire_marked"] = [acquire_run(8, 8, 3), acquire_run(256, 1, 2)]
one = row["acquire_marked"][-1]
if one["median_s"] * 8 * 2 <= args.budget_s:                                # a warm-up and one timed call at 8 records
    row["acquire_marked"].append(acquire_run(256, 8, 1))
else:
    row["acquire_marked_256_default"] = f"not measured: {one['median_s']:.1f} s at one record predicts more than the budget of {args.budget_s:.0f} s"
row["acquire_noise"] = [acquire_run(8, 8, 2, audio=host[0])]

# ---- how often the header decode says ok on noise: 16 clips of 5 s
det = WatermarkDetector(KEY, list_size=8, engine=eng)
order = det._band_order()
n_ok = n_all = 0
per_clip = []
for s in range(16):
    z = (0.05 * np.random.default_rng(100 + s).standard_normal(240_000)).astype(np.float32)
    sc = det._scan_prepare([z], order)[0]
    per_clip.append(int(sc.hdr[0][sc.sel].sum()))
    n_ok += per_clip[-1]; n_all += int(sc.sel.size)
row["noise_headers"] = {"clips": 16, "fitting_peaks": n_all, "ok": n_ok, "ok_per_clip": per_clip}
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
