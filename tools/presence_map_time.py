"""What the presence timeline costs, by the method of tools/live_presence_time.py.  One 60 s clip marked on the device; 33
keys (the detector's and 32 decoys), 8 phases, windows of 40 slots every 20.
(a) The pick.  On the folds of the clip's own windows (64 records, and 1024 by naming the windows again), rigid and under +-300 ppm:
es_fold_pick_batch between two device events, fold_pick plus the download of its lists by the host clock, and the route there was before
-- the download of the fold and presence.pick_hypotheses per record -- by the host clock.  Medians with min and max; the host's pick of
1024 drift records takes many seconds, so it is run twice, not 20 times.
(b) The map.  WatermarkDetector.presence_map on the clip by the host clock, against the only route there was before for the same
question: presence_batch over the samples of the same windows (upload, band-pass, correlation and search again per window).  Where both
routes detect a window their counters and phases are compared.  The map's two halves are timed apart: the front end of the whole clip
(band-pass and correlation, device events) and presence_search.search_map over its windows (host clock).
One run, one card.

    python tools/presence_map_time.py [--out profiles/presence_map.json]
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
from echoseal_amd.presence_search import search_map  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("presence_map_time.py measures on the GPU: none found")
eng = RxEngine(0, list_size_max=0, fs=48_000)
KEY, DECOYS, FL, SPAN, PHASES, W, S, TOTAL, DRIFT = b"\x5C" * 32, 32, 1215, (0, 4096), 8, 40, 20, 60 * 48_000, 300.0


def events(fn, reps=20):
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
    ms = ms[3:]
    return r, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": reps}


def clocked(fn, reps=20, warm=True):
    if warm:
        fn()                                                                # warm-up of every shape the timed calls use
    s = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); s.append(time.perf_counter() - t)
    return r, {"median_ms": 1e3 * statistics.median(s), "min_ms": 1e3 * min(s), "max_ms": 1e3 * max(s), "runs": reps}


host = (0.005 * np.random.default_rng(0).standard_normal((1, TOTAL))).astype(np.float32)
audio = eng.embed(KEY, host, ctr0=0, seed=1).audio.cpu().numpy()[0]
det = WatermarkDetector(KEY, list_size=8, engine=eng)
wins = pr.map_windows(TOTAL - 62, W, S)
row = {"clip_seconds": TOTAL / 48_000, "windows": len(wins), "window_slots": W, "step_slots": S, "keys": 1 + DECOYS, "phases": PHASES,
       "span": list(SPAN), "pick": [], "note": "one run on one MI355X"}

# ---- (a) the pick, on the folds of the clip's own windows
i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(eng.device)  # noqa: E731
i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(eng.device)  # noqa: E731
x = torch.from_numpy(np.tile(audio, (4, 1))).to(eng.device)
bid = torch.arange(4, dtype=torch.uint8, device=eng.device)
corr = eng.xcorr(eng.bpf(x, bid), bid)
for B in (64, 1024):
    recs = [wins[k % len(wins)] for k in range(B)]
    rows4, col, nl = i64([[0, 1, 2, 3]] * B), i64([c for _, c, _ in recs]), i32([n for _, _, n in recs])
    for name, drift in (("rigid", 0.0), ("+-300 ppm", DRIFT)):
        if drift:
            skews, J, warp = pr.skew_table(FL * W, drift)
            D, warp = len(skews), np.broadcast_to(warp, (B, *warp.shape))
        else:
            D, J, warp = 1, W, np.zeros((B, 1, W), np.int32)
        nwarp = i32(np.full(B, D))
        fold = eng.warp_fold_at(corr, rows4, col, nl, i32(warp), nwarp, i32(np.full(B, J)))
        _, t_kernel = events(lambda: eng.fold_pick(fold, nwarp, PHASES, want_val=False))
        got, t_dev = clocked(lambda: eng.fold_pick(fold, nwarp, PHASES, want_val=False)[0].cpu().numpy())
        slow = drift and B > 64
        want, t_host = clocked(lambda: [pr.pick_hypotheses(f, PHASES) for f in fold.cpu().numpy()], reps=2 if slow else 10, warm=not slow)
        same = all([tuple(e) for e in g.tolist()] == w for g, w in zip(got, want))
        row["pick"].append({"records": B, "grid": name, "rows_per_record": D, "values_per_record": D * FL, "es_fold_pick_batch_events": t_kernel,
                            "fold_pick_and_download_host_clock": t_dev, "download_fold_and_pick_hypotheses_host_clock": t_host,
                            "ratio_host_route_over_device_route": t_host["median_ms"] / t_dev["median_ms"], "lists_equal": bool(same)})

# ---- (b) the map against presence_batch over the windows' samples; first its two halves, the clip's front end and the search of its windows
_, t_front = events(lambda: eng.xcorr(eng.bpf(x, bid), bid))
_, t_search = clocked(lambda: search_map(eng, det._presence_ring(DECOYS), 1, corr, [TOTAL - 62], [SPAN], 0.0, PHASES, W, S, 2))
_, t_search_drift = clocked(lambda: search_map(eng, det._presence_ring(DECOYS), 1, corr, [TOTAL - 62], [SPAN], DRIFT, PHASES, W, S, 2))
del x, corr
m, t_map = clocked(lambda: det.presence_map(audio, 48_000, span=SPAN, window=W, step=S, phases=PHASES, decoys=DECOYS), reps=10)
clips = [audio[c:c + n + 62] for _, c, n in wins]
base, t_base = clocked(lambda: det.presence_batch(clips, 48_000, span=SPAN, phases=PHASES, decoys=DECOYS), reps=5)
both = [(p, q) for p, q in zip(m.windows, base) if p.detected and q.detected]
row["map"] = {"presence_map_host_clock": t_map, "front_bpf_and_xcorr_of_the_clip_events": t_front, "search_map_host_clock": t_search,
              "search_map_drift_300ppm_host_clock": t_search_drift, "presence_batch_over_the_windows_host_clock": t_base,
              "ratio_presence_batch_over_presence_map": t_base["median_ms"] / t_map["median_ms"],
              "windows_detected_map": sum(bool(p.detected) for p in m.windows), "windows_detected_presence_batch": sum(bool(q.detected) for q in base),
              "windows_detected_by_both": len(both), "of_those_same_counter_and_phase": sum((p.ctr, p.phase) == (q.ctr, q.phase) for p, q in both),
              "stretches": [[s.first, s.last, bool(s.confirmed)] for s in m.stretches], "splices": len(m.splices), "marked_samples": m.marked}
m, t_drift = clocked(lambda: det.presence_map(audio, 48_000, span=SPAN, window=W, step=S, phases=PHASES, decoys=DECOYS, drift_ppm=DRIFT), reps=10)
row["map_drift_300ppm"] = {"presence_map_host_clock": t_drift, "windows_detected": sum(bool(p.detected) for p in m.windows),
                           "stretches": [[s.first, s.last, bool(s.confirmed)] for s in m.stretches], "splices": len(m.splices)}
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
