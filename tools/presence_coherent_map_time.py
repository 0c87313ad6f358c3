"""What the coherent presence timeline costs, by the method of tools/presence_map_time.py: device events around each engine
call (medians of 20 with min and max), whole public calls by the host clock around the call (they end in a download).  Clips marked on the
device on a loud host (sigma 0.2), 33 keys (the detector's and 32 decoys), span 4096, windows of 40 slots every 20, every phase.
(a) The 5 s clip.  WatermarkDetector.presence_coherent_map against presence_coherent on the whole clip in the same process -- the
yardstick for the work per (origin, slot, phase) -- and its parts: mf_rows of the clip, the hop window of the windows' hop rows, and
es_coherent_score_at_batch over the windows, beside es_coherent_score_batch over the whole clip.
(b) The same map against the route there was before: presence_coherent_batch over the samples of the same windows cut out as separate
clips.  Their rows are not the clip's rows (each cut restarts the band-pass), so verdicts are compared, not bits.
(c) A 60 s clip: the map by the host clock (5 runs) and the score call over its windows between events (5 runs).
One run, one card.

    python tools/presence_coherent_map_time.py [--out profiles/presence_coherent_map.json]
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
    raise SystemExit("presence_coherent_map_time.py measures on the GPU: none found")
eng = RxEngine(0, list_size_max=0, fs=48_000)
KEY, DECOYS, FL, SPAN, W, S = b"\x5C" * 32, 32, 1215, (0, 4096), 40, 20


def events(fn, reps=20):
    ms = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); r = fn(); b.record(); b.synchronize(); ms.append(a.elapsed_time(b))
    ms = ms[3:]
    return r, {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "runs": reps}


def clocked(fn, reps=20):
    fn()                                                                    # warm-up of every shape the timed calls use
    s = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); s.append(time.perf_counter() - t)
    return r, {"median_ms": 1e3 * statistics.median(s), "min_ms": 1e3 * min(s), "max_ms": 1e3 * max(s), "runs": reps}


def marked(samples):
    host = (0.2 * np.random.default_rng(0).standard_normal((1, samples))).astype(np.float32)     # a loud host: the normal operating point
    return eng.embed(KEY, host, ctr0=0, seed=1).audio[0].cpu().numpy()[777:]


det = WatermarkDetector(KEY, list_size=8, engine=eng)
ring = det._presence_ring(DECOYS)
g, _ = pr.mf_tables(tables=eng.tables())
tail = 189 + max(len(t) for t in g)
bid = torch.arange(4, dtype=torch.uint8, device=eng.device)


def parts(clip, reps):
    """The engine calls of one map of `clip`, each between two device events."""
    x = torch.from_numpy(np.repeat(clip[None], 4, axis=0)).to(eng.device)
    y = eng.bpf(x, bid)
    lens = torch.full((4,), clip.size, dtype=torch.int32, device=eng.device)
    out = [torch.zeros_like(y) for _ in range(3)]
    rows, t_rows = events(lambda: eng.mf_rows(y, lens, bid, out=out), reps)
    wins = pr.coherent_windows(clip.size, g, W, S)
    spans = [pr.window_span(SPAN, s, J) for s, _, J in wins]
    bases = [lo for lo, _ in spans]
    width = SPAN[1] - SPAN[0]
    hop, t_hop = events(lambda: eng.hop_window(ring, bases, width + W - 1), reps)
    B = len(wins)
    rows4, col = np.tile(np.arange(4, dtype=np.int64), (B, 1)), np.array([c for _, c, _ in wins], np.int64)
    nslot = np.array([J for _, _, J in wins], np.int32)
    lists = torch.arange(FL, dtype=torch.int32, device=eng.device).repeat(B, 1)
    _, t_at = events(lambda: eng.coherent_score_at(*rows, rows4, col, nslot, lists, ring, hop, np.arange(B, dtype=np.int32), np.array(bases, np.int64),
                                                   width), reps)
    return rows, {"windows": B, "hop_rows": B, "mf_rows_4_rows_events": t_rows, "hop_window_events": t_hop, "coherent_score_at_events": t_at}


row = {"keys": 1 + DECOYS, "span": list(SPAN), "window_slots": W, "step_slots": S, "phases": FL, "host_sigma": 0.2, "note": "one run on one MI355X"}

# ---- (a) the 5 s clip: the map, the whole-clip call, and the engine calls of each
clip = marked(240_000)
J = pr.coherent_slots(clip.size, g)
rows, five = parts(clip, 20)
hop1 = eng.hop_window(ring, [SPAN[0]], SPAN[1] - SPAN[0] + (clip.size - 190) // FL - 1)
plist = np.arange(FL, dtype=np.int32)[None]
_, t_whole_score = events(lambda: eng.coherent_score(*rows, [J], plist, ring, hop1, SPAN[0], SPAN[1] - SPAN[0]))
m, t_map = clocked(lambda: det.presence_coherent_map(clip, 48_000, span=SPAN, window=W, step=S, decoys=DECOYS))
p, t_whole = clocked(lambda: det.presence_coherent(clip, 48_000, span=SPAN, decoys=DECOYS))
five.update({"samples": int(clip.size), "slots": J, "slots_summed_by_the_windows": int(sum(q.frames for q in m.windows)),
             "presence_coherent_map_host_clock": t_map, "presence_coherent_whole_clip_host_clock": t_whole,
             "coherent_score_whole_clip_events": t_whole_score,
             "ratio_map_over_whole_clip": t_map["median_ms"] / t_whole["median_ms"],
             "ratio_score_at_over_score_per_slot": (five["coherent_score_at_events"]["median_ms"] / sum(q.frames for q in m.windows))
                                                   / (t_whole_score["median_ms"] / J),
             "windows_detected": sum(bool(q.detected) for q in m.windows), "whole_clip_detected": bool(p.detected),
             "stretches": [[s.first, s.last, bool(s.confirmed)] for s in m.stretches], "splices": len(m.splices), "marked_samples": m.marked})
row["clip_5s"] = five
print(f"5 s: map {t_map['median_ms']:.1f} ms, whole clip {t_whole['median_ms']:.1f} ms", file=sys.stderr, flush=True)

# ---- (b) the route there was before: the windows cut out as separate clips (their rows are not the clip's rows)
wins = pr.coherent_windows(clip.size, g, W, S)
cuts = [clip[c:c + FL * n + tail] for _, c, n in wins]
base, t_base = clocked(lambda: [det.presence_coherent_batch([x], 48_000, span=pr.window_span(SPAN, s, n), decoys=DECOYS)[0]
                                for x, (s, _, n) in zip(cuts, wins)], reps=10)
both = [(a, b) for a, b in zip(m.windows, base) if a.detected and b.detected]
row["windows_as_separate_clips"] = {"presence_coherent_batch_per_window_host_clock": t_base,
                                    "ratio_separate_clips_over_map": t_base["median_ms"] / t_map["median_ms"],
                                    "windows_detected": sum(bool(b.detected) for b in base), "windows_detected_by_both": len(both),
                                    "of_those_same_counter_and_phase": sum((a.ctr, a.phase) == (b.ctr, b.phase) for a, b in both),
                                    "note": "one call per window, since each window has its own span; every cut restarts the band-pass, so "
                                            "the rows differ from the clip's in their first samples"}
del rows

# ---- (c) a 60 s clip
clip = marked(60 * 48_000)
_, sixty = parts(clip, 5)
m, t_map = clocked(lambda: det.presence_coherent_map(clip, 48_000, span=SPAN, window=W, step=S, decoys=DECOYS), reps=5)
sixty.update({"samples": int(clip.size), "slots": pr.coherent_slots(clip.size, g), "presence_coherent_map_host_clock": t_map,
              "windows_detected": sum(bool(q.detected) for q in m.windows), "stretches": [[s.first, s.last, bool(s.confirmed)] for s in m.stretches],
              "splices": len(m.splices), "splices_lo_hi_removed": [[s.lo, s.hi, s.removed] for s in m.splices],
              "undetected_windows_own_and_decoy_max": [[st, p.score, float(p.null.max())] for st, p in zip(m.starts, m.windows) if not p.detected],
              "marked_samples": m.marked})
row["clip_60s"] = sixty
print(json.dumps(row))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(row) + "\n")
