"""What the drift search of a presence test costs.  On a 5 s clip marked on the device, under 33 keys (the detector's and 32
decoys), span 4096, 8 hypotheses: the warp fold and the warp score, each between two device events (medians of 20 with min and max), for a
search of +-100 ppm and of +-300 ppm; and the new score call on a table of zeros beside es_hop_score_batch on identical inputs (the existing
kernel is the baseline; the outputs are compared byte for byte).

    python tools/presence_drift_time.py [--out profiles/presence_drift.json]

ES_LIB_VARIANT names another build of the library (tools/build_variant.sh): the JSON line says which one was timed.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import echoseal_amd._native as nat  # noqa: E402
from echoseal_amd import presence as pr  # noqa: E402
from echoseal_amd.detector import WatermarkDetector  # noqa: E402
from echoseal_amd.engine import RxEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("presence_drift_time.py measures on the GPU: none found")
eng = RxEngine(0, list_size_max=0, fs=48_000)
KEY, DECOYS, FL, SPAN, HYPS = b"\x5C" * 32, 32, 1215, 4096, 8


def events(fn, reps=20):
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
    ms = ms[3:]
    return r, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


host = (0.005 * np.random.default_rng(0).standard_normal((1, 240_000))).astype(np.float32)
clip = eng.embed(KEY, host, ctr0=0, seed=1).audio[0].cpu().numpy()[777:]
det = WatermarkDetector(KEY, list_size=8, engine=eng)
ring = det._presence_ring(DECOYS)
bid = torch.arange(4, dtype=torch.uint8, device=eng.device)
corr = eng.xcorr(eng.bpf(torch.from_numpy(np.repeat(clip[None], 4, axis=0)).to(eng.device), bid), bid)
nlag = torch.tensor([clip.size - 62], dtype=torch.int32, device=eng.device)
i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(eng.device)  # noqa: E731

row = {"samples": int(clip.size), "keys": 1 + DECOYS, "span": SPAN, "hypotheses": HYPS, "runs": 20, "lib_variant": nat.LIB_VARIANT or "stock",
       "ES_WARP_HB": nat.ES_WARP_HB if not nat.LIB_VARIANT else None, "cases": []}
for ppm in (100.0, 300.0):
    skews, J, warp = pr.skew_table(clip.size - 62, ppm)
    warp_d, nwarp, nslot = i32(warp[None]), i32([len(skews)]), i32([J])
    fold, t_fold = events(lambda: eng.warp_fold(corr, nlag, warp_d, nwarp, nslot))
    hyps = pr.pick_hypotheses(fold.cpu().numpy()[0], HYPS)
    hyp = i32([hyps])
    hop = eng.hop_window(ring, [0], SPAN + J - 1)
    (score, origin, rank), t_score = events(lambda: eng.warp_score(corr, nlag, warp_d, nwarp, nslot, hyp, hop, SPAN))
    score, best = score.cpu().numpy()[0], hyps[int(rank[0, 0])]
    row["cases"].append({"drift_ppm": ppm, "rows": len(skews), "frames": J, "warp_fold": t_fold, "warp_score": t_score, "skew": skews[best[0]],
                         "phase": best[1], "ctr": int(origin[0, 0]), "score": float(score[0]), "decoy_max": float(score[1:].max())})

# the rigid grid both ways: es_hop_score_batch, and es_warp_score_batch on one row of zeros
J = (clip.size - 62) // FL
plist = pr.pick_phases(eng.phase_fold(corr, nlag).cpu().numpy()[0], HYPS)
hop = eng.hop_window(ring, [0], SPAN + corr.shape[1] // FL - 1)
phases, hyp = i32([plist]), i32([[(0, p) for p in plist]])
zeros, one, nslot = i32(np.zeros((1, 1, J))), i32([1]), i32([J])
old, t_old = events(lambda: eng.hop_score(corr, nlag, phases, hop, SPAN))
new, t_new = events(lambda: eng.warp_score(corr, nlag, zeros, one, nslot, hyp, hop, SPAN))
old2, t_old2 = events(lambda: eng.hop_score(corr, nlag, phases, hop, SPAN))                  # the baseline again: the spread between two runs of one call
row["zero_table"] = {"frames": J, "hop_score": t_old, "warp_score": t_new, "hop_score_again": t_old2,
                     "same_bytes": all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(old, new))}
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
