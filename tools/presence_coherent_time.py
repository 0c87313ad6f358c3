"""What the coherent presence test costs.  On a 5 s clip marked on the device, under 33 keys (the detector's and 32 decoys):
the matched-filter rows, the hop window and the score call, each between two device events (medians of 20 with min and max), and
WatermarkDetector.presence_coherent as a whole by the host clock around the call (it ends in a download), for
    spans 4096 and 64, each with all 1215 phases and with the 8 phases of the keyless fold.

    python tools/presence_coherent_time.py [--out profiles/presence_coherent.json]
    ES_LIB_VARIANT=NAME python tools/presence_coherent_time.py --score-only     # an A/B build of tools/build_variant.sh: the score calls alone
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
import echoseal_amd._native as nat  # noqa: E402
from echoseal_amd import presence as pr  # noqa: E402
from echoseal_amd.detector import WatermarkDetector  # noqa: E402
from echoseal_amd.engine import RxEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--score-only", action="store_true", help="the score calls over all phases alone (A/B runs)")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("presence_coherent_time.py measures on the GPU: none found")
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


host = (0.2 * np.random.default_rng(0).standard_normal((1, 240_000))).astype(np.float32)      # a loud host: the normal operating point
clip = eng.embed(KEY, host, ctr0=0, seed=1).audio[0].cpu().numpy()[777:]
det = WatermarkDetector(KEY, list_size=8, engine=eng)
ring = det._presence_ring(DECOYS)

# what presence_coherent() reads: four band-passed rows of the clip
bid = torch.arange(4, dtype=torch.uint8, device=eng.device)
x = torch.from_numpy(np.repeat(clip[None], 4, axis=0)).to(eng.device)
y, t_bpf = events(lambda: eng.bpf(x, bid))
lens = torch.full((4,), clip.size, dtype=torch.int32, device=eng.device)
out = [torch.zeros_like(y) for _ in range(3)]
rows, t_rows = events(lambda: eng.mf_rows(y, lens, bid, out=out))
g, _ = pr.mf_tables(tables=eng.tables())
J = pr.coherent_slots(clip.size, g)
fold = eng.phase_fold(eng.xcorr(y, bid), [clip.size - 62]).cpu().numpy()[0]

row = {"samples": int(clip.size), "frames": J, "keys": 1 + DECOYS, "library": nat.LIB_VARIANT or "default", "bpf_4_rows": t_bpf, "mf_rows_4_rows": t_rows,
       "runs": 20, "cases": []}
for span, phases in (((0, 4096), FL), ((0, 64), FL), ((0, 4096), 8), ((0, 64), 8)):
    if args.score_only and phases != FL:
        continue
    n = span[1] - span[0]
    plist = np.array([pr.pick_phases(fold, phases)], np.int32)
    hop, t_hop = events(lambda: eng.hop_window(ring, [span[0]], n + (y.shape[1] - 190) // FL - 1))
    _, t_score = events(lambda: eng.coherent_score(*rows, [J], plist, ring, hop, span[0], n), reps=5 if args.score_only else 20)
    case = {"span": list(span), "phases": phases, "hop_window": t_hop, "coherent_score": t_score}
    if not args.score_only:
        p, t_all = clocked(lambda: det.presence_coherent(clip, 48_000, span=span, phases=phases, decoys=DECOYS))
        case.update({"presence_coherent_call_host_clock": t_all, "detected": bool(p.detected), "ctr": p.ctr, "phase": p.phase, "score": p.score,
                     "decoy_max": float(p.null.max())})
    row["cases"].append(case)
    print(f"span {span}, phases {phases}: score {t_score['median_ms']:.2f} ms", file=sys.stderr, flush=True)
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
