"""What a presence test costs.  On a 5 s clip marked on the device, under 33 keys (the detector's and 32 decoys): the fold, the
hop window and the score call, each between two device events (medians of 20 with min and max), and WatermarkDetector.presence as a whole by
the host clock around the call (it ends in a download), for
    span 4096 with 8 phases,   span 2^17 with 8 phases,   span 4096 with 1215 phases.

    python tools/presence_time.py [--out profiles/presence.json]
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
from echoseal_amd import presence as pr  # noqa: E402
from echoseal_amd.detector import WatermarkDetector  # noqa: E402
from echoseal_amd.engine import RxEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("presence_time.py measures on the GPU: none found")
eng = RxEngine(0, list_size_max=0, fs=48_000)
KEY, DECOYS, FL = b"\x5C" * 32, 32, 1215


def events(fn, reps=20):
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
    ms = ms[3:]
    return r, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def clocked(fn, reps=20):
    fn()                                                                    # warm-up of every shape the timed calls use
    s = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); s.append(time.perf_counter() - t)
    return r, {"median_ms": 1e3 * statistics.median(s), "min_ms": 1e3 * min(s), "max_ms": 1e3 * max(s)}


host = (0.005 * np.random.default_rng(0).standard_normal((1, 240_000))).astype(np.float32)
clip = eng.embed(KEY, host, ctr0=0, seed=1).audio[0].cpu().numpy()[777:]
det = WatermarkDetector(KEY, list_size=8, engine=eng)
ring = det._presence_ring(DECOYS)

# the rows presence() reads: four band rows of the clip
bid = torch.arange(4, dtype=torch.uint8, device=eng.device)
x = torch.from_numpy(np.repeat(clip[None], 4, axis=0)).to(eng.device)
(corr), t_front = events(lambda: eng.xcorr(eng.bpf(x, bid), bid))
nlag = [clip.size - 62]
J = nlag[0] // FL
fold, t_fold = events(lambda: eng.phase_fold(corr, nlag))
fold = fold.cpu().numpy()[0]

row = {"samples": int(clip.size), "frames": J, "keys": 1 + DECOYS, "bpf_xcorr_4_rows": t_front, "phase_fold": t_fold, "runs": 20, "cases": []}
for span, phases in (((0, 4096), 8), ((0, 1 << 17), 8), ((0, 4096), FL)):
    n = span[1] - span[0]
    plist = np.array([pr.pick_phases(fold, phases)], np.int32)
    hop, t_hop = events(lambda: eng.hop_window(ring, [span[0]], n + corr.shape[1] // FL - 1))
    _, t_score = events(lambda: eng.hop_score(corr, nlag, plist, hop, n))
    p, t_all = clocked(lambda: det.presence(clip, 48_000, span=span, phases=phases, decoys=DECOYS))
    row["cases"].append({"span": list(span), "phases": phases, "hop_window": t_hop, "hop_score": t_score, "presence_call_host_clock": t_all,
                         "detected": bool(p.detected), "ctr": p.ctr, "phase": p.phase, "score": p.score, "decoy_max": float(p.null.max())})
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
