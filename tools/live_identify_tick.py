"""One tick of live identification (LiveIdentifier.push) three ways on one engine:

  (a) with the verdict memo (the default),
  (b) with memo_slots=0: every push decodes its whole window,
  (c) the path that existed before: WatermarkIdentifier.identify_batch over the same windows, cut on the host and uploaded each tick.

64 streams of plain noise at 48 kHz, 16 keys, 5 s windows, 100 ms chunks, list size 8.  The streams are first filled past one window
(with half-second chunks), then every timed tick pushes the next 100 ms of every stream.  Each call lies between two events on the
engine's stream and is synchronised before the next starts: a figure is what a caller waits for.  Medians with min and max, the
candidates decoded per tick (each is four list decodes), and whether all three gave the same answers.

    python tools/live_identify_tick.py --ticks 30 --out profiles/live_identify_tick.json --tag <commit>

--ctr0 C: the streams of (a) and (b) are opened with counter origins C, C + 1000, C + 2000, ... -- planned from absolute
positions, their hop rows rebuilt on the device each push -- and (c) is given the counter of the frame each window starts in.
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
from echoseal_amd.engine import RxEngine  # noqa: E402
from echoseal_amd.identify import WatermarkIdentifier  # noqa: E402

FS = 48_000


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return out, a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def stats(ev, wall, decoded):
    return {"median_ms": statistics.median(ev), "min_ms": min(ev), "max_ms": max(ev), "wall_median_ms": statistics.median(wall),
            "decoded_per_tick_median": statistics.median(decoded), "decoded_per_tick_max": max(decoded), "ticks": len(ev)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--window-s", type=float, default=5.0)
    ap.add_argument("--chunk-s", type=float, default=0.1)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--ticks", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ctr0", type=int, default=None, help="open the streams with counter origins ctr0, ctr0 + 1000, ...")
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    eng = RxEngine(0, fs=FS)
    stream = torch.cuda.current_stream(eng.device)
    S, chunk, fill_chunk, window = args.streams, int(args.chunk_s * FS), FS // 2, int(args.window_s * FS)
    fill = -(-window // fill_chunk) + 1
    rng = np.random.default_rng(1)
    xs = (0.1 * rng.standard_normal((S, fill * fill_chunk + (args.warmup + args.ticks) * chunk))).astype(np.float32)
    keys = [rng.bytes(32) for _ in range(args.keys)]
    ident = WatermarkIdentifier(keys, fs_target=FS, list_size=args.list_size, engine=eng)
    origin = {} if args.ctr0 is None else {"ctr0": [args.ctr0 + 1000 * s for s in range(S)]}
    with_memo = ident.open_streams(S, window_s=args.window_s, chunk_max=fill_chunk, **origin)
    without = ident.open_streams(S, window_s=args.window_s, chunk_max=fill_chunk, memo_slots=0, **origin)
    at = 0
    for _ in range(fill):
        with_memo.push([x[at: at + fill_chunk] for x in xs]); without.push([x[at: at + fill_chunk] for x in xs])
        at += fill_chunk
    ev = {k: ([], [], []) for k in ("memo", "no_memo", "identify_batch")}
    skipped = []
    same = True
    for t in range(args.warmup + args.ticks):
        chunks = [x[at: at + chunk] for x in xs]
        a, ea, wa = timed(lambda: with_memo.push(chunks), stream)
        b, eb, wb = timed(lambda: without.push(chunks), stream)
        at += chunk
        w0, n = with_memo.window(0)
        # a window cut at w0 = 1216 k of a stream marked from C starts k samples into the frame of counter C + k: the clip call has no
        # pos0, so with origins (c) is timed but walks slightly other candidates than the pushes, and only (a) == (b) is compared
        clip_origin = {} if args.ctr0 is None else {"ctr0": [args.ctr0 + 1000 * s + (2 * w0 + 1215) // 2430 for s in range(S)]}
        c, ec, wc = timed(lambda: ident.identify_batch([x[w0:n] for x in xs], FS, **clip_origin), stream)
        same = same and a == b and (args.ctr0 is not None or b == c)
        if t >= args.warmup:
            skipped.append(with_memo.stats["skipped"])
        if t >= args.warmup:
            for k, e, w, d in (("memo", ea, wa, with_memo.stats["decoded"]), ("no_memo", eb, wb, without.stats["decoded"]),
                               ("identify_batch", ec, wc, without.stats["planned"])):      # (c) decodes what (b) decodes: the same walk
                ev[k][0].append(e); ev[k][1].append(w); ev[k][2].append(d)
    row = {"streams": S, "keys": args.keys, "window_s": args.window_s, "chunk_s": args.chunk_s, "list_size": args.list_size,
           "memo_slots": with_memo.memo_slots, "push_memo": stats(*ev["memo"]), "push_no_memo": stats(*ev["no_memo"]),
           "identify_batch": stats(*ev["identify_batch"]), "planned_per_tick_median": statistics.median(ev["identify_batch"][2]),
           "skipped_per_tick_median": statistics.median(skipped), "ctr0": args.ctr0, "same_answers": bool(same), "device": torch.cuda.get_device_name(eng.device), "tag": args.tag}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
