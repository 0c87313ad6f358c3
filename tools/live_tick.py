"""One tick of S live streams (RxEngine.embed_step) against the per-stream loop of embed(key, chunk, carry=prev) it replaces.

S streams under 64 keys, one 1 024-sample float32 chunk each per tick, seed= set (payloads sealed on the device in both).  Per S: a
warm-up, then --ticks timed ticks of each call in the same process, every tick between two events on the engine's stream and
synchronised before the next starts, so a figure is what a caller waits for: host work, copies and kernels.  The median is reported,
with min and max, the wall-clock median next to it, and the frame generator alone (polar encode, keyed schedule, band-pass) over the
frames of one tick.  Both calls produce the same bits (tests/test_gpu_live_streams.py); the last tick of each is compared here too.

    python tools/live_tick.py --streams 64,1024,4096 --ticks 20 --out profiles/live_tick.json --tag <commit>
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

SEED, CHUNK, NKEYS = 20260101, 1024, 64


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="64,1024,4096")
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    eng = RxEngine(0, list_size_max=0)
    stream = torch.cuda.current_stream(eng.device)
    keys = [bytes([k + 1]) * 32 for k in range(NKEYS)]
    ring = eng.keyring(keys)
    rng = np.random.default_rng(1)
    rows = []
    for S in [int(s) for s in args.streams.split(",")]:
        kidx = [s % NKEYS for s in range(S)]
        chunks = [(0.1 * rng.standard_normal(CHUNK)).astype(np.float32) for _ in range(S)]
        sid = np.arange(S)

        table = eng.open_streams(ring, kidx)
        ev, wall = [], []
        for t in range(args.warmup + args.ticks):
            got, e, w = timed(lambda: eng.embed_step(table, sid, chunks, seed=SEED), stream)
            if t >= args.warmup:
                ev.append(e); wall.append(w)
        tick = stats(ev, wall)

        prev = [None] * S

        def loop():
            for s in range(S):
                prev[s] = eng.embed(keys[kidx[s]], chunks[s][None, :], ctr0=0 if prev[s] is None else prev[s].ctr, carry=prev[s], seed=SEED)
        ev, wall = [], []
        for t in range(args.warmup + args.ticks):
            _, e, w = timed(loop, stream)
            if t >= args.warmup:
                ev.append(e); wall.append(w)
        per_stream = stats(ev, wall)
        same = all(torch.equal(got[s].audio, prev[s].audio[0]) for s in range(0, S, max(1, S // 64)))

        F = S                                                           # a tick of 1 024-sample chunks makes about one frame per stream
        ctr = torch.arange(F, dtype=torch.int64, device=eng.device)
        kf = torch.tensor(kidx, dtype=torch.int32, device=eng.device)
        blobs = torch.zeros((F, 55), dtype=torch.uint8, device=eng.device)
        ev, wall = [], []
        for t in range(args.warmup + args.ticks):
            _, e, w = timed(lambda: eng.make_frames_keyed(ring, kf, ctr, blobs), stream)
            if t >= args.warmup:
                ev.append(e); wall.append(w)
        row = {"streams": S, "keys": NKEYS, "chunk": CHUNK, "tick": tick, "loop": per_stream, "loop_over_tick": per_stream["median_ms"] / tick["median_ms"],
               "frame_generator": stats(ev, wall), "same_bits": bool(same), "device": torch.cuda.get_device_name(eng.device), "tag": args.tag}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
