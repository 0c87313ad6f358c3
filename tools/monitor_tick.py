"""One tick of a live monitor (LiveMonitor.push) against the path that existed before it: WatermarkDetector.verify_batch over the same
windows on the same engine.

64 streams of noise with embedded frames at 48 kHz, 5 s windows, 0.5 s chunks, list size 8.  The streams are first filled past one
window, so that every timed tick verifies a full window.  Per tick the monitor pushes the next 0.5 s of every stream; the yardstick
verifies, in one verify_batch call, the 64 windows [w0, n) the monitor has just verified, cut from the host copies of the streams (what a
caller without the monitor does on every tick: upload and band-pass the whole window again).  Every call lies between two events on the
engine's stream and is synchronised before the next starts, so a figure is what a caller waits for: host work, copies and kernels.
Medians with min and max; the verdicts of both are compared.  The sync stage alone (monitor_step against sync over the windows) is
timed too: that is where the two paths differ, the candidate walk behind it is the same code.

    python tools/monitor_tick.py --ticks 10 --out profiles/monitor_tick.json --tag <commit>

--fs RATE: the streams arrive at RATE instead.  The same marked streams are converted to RATE on the host once; the monitor is
opened with fs=RATE and pushed chunk_s of them per tick, the yardstick is a second monitor at 48 kHz on the same engine that is pushed the
pre-conditioned chunks r[F(n_old) : F(n_new)] -- the path that existed before, with the resampling done elsewhere.  LiveMonitor.push and
monitor_step of both are timed as above and the verdicts compared.

    python tools/monitor_tick.py --fs 44100 --ticks 10 --out profiles/monitor_tick_rates.json --tag <commit>
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
from echoseal_amd.detector import WatermarkDetector  # noqa: E402
from echoseal_amd.engine import RxEngine  # noqa: E402

KEY = b"\xAA" * 32
FS = 48_000


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def stats(ev, wall):
    return {"median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "wall_median_ms": statistics.median(wall), "ticks": len(ev)}


def main_rates(args) -> None:
    """Streams at args.fs against an at-rate monitor fed the conditioned chunks."""
    from scipy.signal import resample_poly
    from echoseal_amd.utils import finalized, stream_resample_plan
    eng = RxEngine(0, fs=FS)
    stream = torch.cuda.current_stream(eng.device)
    pl = stream_resample_plan(args.fs, FS)
    S, chunk, chunk_t = args.streams, int(args.chunk_s * args.fs), int(args.chunk_s * FS)
    fill = -(-int(args.window_s * FS) // chunk_t) + 1
    ticks = fill + 2 * (args.warmup + args.ticks)
    rng = np.random.default_rng(1)
    host = (0.05 * rng.standard_normal((S, ticks * chunk_t + 4800))).astype(np.float32)
    marked = eng.embed(KEY, host, seed=7).audio.cpu().numpy()
    xs = [resample_poly(x.astype(np.float64), pl.down, pl.up).astype(np.float32)[:ticks * chunk] for x in marked]      # at args.fs
    rs = [resample_poly(x, pl.up, pl.down) for x in xs]                                                                # what the device finalizes
    F = lambda n: finalized(n, pl.up, pl.down, pl.y0)
    cmax = F(chunk) + pl.y0 + 2
    det = WatermarkDetector(KEY, fs_target=FS, list_size=args.list_size, engine=eng)
    mon = det.open_streams(S, fs=args.fs, window_s=args.window_s, chunk_max=cmax)
    ref_det = WatermarkDetector(KEY, fs_target=FS, list_size=args.list_size, engine=eng)
    ref = ref_det.open_streams(S, window_s=args.window_s, chunk_max=cmax)
    at = 0
    raw = lambda: [x[at: at + chunk] for x in xs]
    cond = lambda: [r[F(at): F(at + chunk)] for r in rs]
    for _ in range(fill):
        mon.push(raw()); ref.push(cond())
        at += chunk
    ev = {k: ([], []) for k in ("push", "push_at_rate", "step", "step_at_rate")}
    same = True
    for t in range(args.warmup + args.ticks):
        got, e, w = timed(lambda: mon.push(raw()), stream)
        want, e2, w2 = timed(lambda: ref.push(cond()), stream)
        at += chunk
        same = same and got == want
        if t >= args.warmup:
            ev["push"][0].append(e); ev["push"][1].append(w); ev["push_at_rate"][0].append(e2); ev["push_at_rate"][1].append(w2)
    ids = np.arange(S)
    for t in range(args.warmup + args.ticks):
        a, e, w = timed(lambda: eng.monitor_step(mon.table, ids, raw()), stream)
        b, e2, w2 = timed(lambda: eng.monitor_step(ref.table, ids, cond()), stream)
        at += chunk
        same = same and torch.equal(a.peaks, b.peaks) and torch.equal(a.npeaks, b.npeaks) and torch.equal(a.thr.view(torch.int64), b.thr.view(torch.int64))
        if t >= args.warmup:
            ev["step"][0].append(e); ev["step"][1].append(w); ev["step_at_rate"][0].append(e2); ev["step_at_rate"][1].append(w2)
    row = {"streams": S, "fs": args.fs, "window_s": args.window_s, "chunk_s": args.chunk_s, "list_size": args.list_size,
           "monitor_push": stats(*ev["push"]), "monitor_push_at_rate": stats(*ev["push_at_rate"]), "monitor_step": stats(*ev["step"]),
           "monitor_step_at_rate": stats(*ev["step_at_rate"]), "same_results": bool(same), "device": torch.cuda.get_device_name(eng.device),
           "tag": args.tag}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--window-s", type=float, default=5.0)
    ap.add_argument("--chunk-s", type=float, default=0.5)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--fs", type=int, default=None, help="rate the streams arrive at (default: 48 000, the monitor's own)")
    args = ap.parse_args()
    if args.fs is not None and args.fs != FS:
        return main_rates(args)
    eng = RxEngine(0, fs=FS)
    stream = torch.cuda.current_stream(eng.device)
    S, chunk, window = args.streams, int(args.chunk_s * FS), int(args.window_s * FS)
    fill = -(-window // chunk) + 1                                          # ticks that fill the window before anything is timed
    total = (fill + args.warmup + 2 * args.ticks) * chunk
    rng = np.random.default_rng(1)
    host = (0.05 * rng.standard_normal((S, total))).astype(np.float32)
    xs = eng.embed(KEY, host, seed=7).audio.cpu().numpy()

    det = WatermarkDetector(KEY, fs_target=FS, list_size=args.list_size, engine=eng)
    mon = det.open_streams(S, window_s=args.window_s, chunk_max=chunk)
    ref = WatermarkDetector(KEY, fs_target=FS, list_size=args.list_size, engine=eng)
    at = 0
    for _ in range(fill):
        mon.push([x[at: at + chunk] for x in xs])
        at += chunk
    ev_m, wall_m, ev_v, wall_v, same = [], [], [], [], True
    for t in range(args.warmup + args.ticks):
        got, e, w = timed(lambda: mon.push([x[at: at + chunk] for x in xs]), stream)
        at += chunk
        w0, n = mon.window(0)
        want, e2, w2 = timed(lambda: ref.verify_batch([x[w0:n] for x in xs], FS), stream)
        same = same and got == want
        if t >= args.warmup:
            ev_m.append(e); wall_m.append(w); ev_v.append(e2); wall_v.append(w2)
    # the sync stage alone: continued (monitor_step) against started again (upload + sync over the 64 windows)
    band = torch.from_numpy(np.tile(mon.table.bands, S)).to(eng.device)
    ev_s, wall_s, ev_r, wall_r = [], [], [], []
    for t in range(args.warmup + args.ticks):
        _, e, w = timed(lambda: eng.monitor_step(mon.table, np.arange(S), [x[at: at + chunk] for x in xs]), stream)
        at += chunk
        w0, n = mon.window(0)
        _, e2, w2 = timed(lambda: eng.sync(torch.from_numpy(np.repeat(xs[:, w0:n], 4, axis=0)).to(eng.device), band, keep_corr=False), stream)
        if t >= args.warmup:
            ev_s.append(e); wall_s.append(w); ev_r.append(e2); wall_r.append(w2)
    m, v = stats(ev_m, wall_m), stats(ev_v, wall_v)
    row = {"streams": S, "window_s": args.window_s, "chunk_s": args.chunk_s, "list_size": args.list_size, "monitor_push": m, "verify_batch": v,
           "verify_over_push": v["median_ms"] / m["median_ms"], "monitor_step": stats(ev_s, wall_s), "upload_and_sync": stats(ev_r, wall_r),
           "same_verdicts": bool(same), "device": torch.cuda.get_device_name(eng.device), "tag": args.tag}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
