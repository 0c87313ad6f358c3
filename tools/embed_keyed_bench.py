#!/usr/bin/env python3
"""A queue of uploads to mark, each under its owner's key: RxEngine.embed_batch against the loop of RxEngine.embed calls it replaces.

    python tools/embed_keyed_bench.py [--runs 3] [--repeats 3] [--limit 300] [--tag NAME] [--out profiles/embed_keyed_bench.json]

Workloads (seeded noise at 48 kHz, payloads from seed=):
  distinct64 / distinct512   64 / 512 clips of as many distinct lengths between 1 s and 6 s, each under a key of its own;
  control                    256 clips of exactly 5 s under ONE key: `embed` takes them in one call, so here the batch can only lose.
Per workload two timings: `batch` = embed_batch(keys, idx, clips, seed=...), `loop` = [embed(keys[i], clips[i], seed=...) for i]
(control: one embed over the [256, n] tensor) -- the loop is code the batch does not change, so it is the baseline.  The batch timing
asserts that its bytes equal the loop's.  Each timing runs in a child process of its own under a time limit (--limit seconds): wall
clock around the call with the device idle before and after, one warm-up call and --repeats timed ones; --runs runs, batch and loop
alternating; after a timing that fails no further one is started.  `mix` additionally times the ragged mix launch alone by device
events (bytes = 12 x real samples: the samples read, the chips read, the samples written).  Prints one JSON line per timing and
appends all lines to --out.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 48_000
SEED = 20260101


def make_case(workload: str):
    rng = np.random.default_rng(2026)
    if workload == "control":
        n = 256
        lengths = [5 * FS] * n
        keys = [bytes(range(32))]
        idx = [0] * n
    else:
        n = int(workload[len("distinct"):])
        step = (5 * FS) // max(1, n - 1)
        lengths = [FS + i * step - (i * 37) % 101 for i in range(n)]
        lengths = [lengths[i] for i in rng.permutation(n)]                 # n distinct lengths, 1 s .. 6 s, in no order
        assert len(set(lengths)) == n
        keys = [rng.bytes(32) for _ in range(n)]
        idx = list(range(n))
    clips = [(rng.standard_normal(m) * 0.1).astype(np.float32) for m in lengths]
    return keys, idx, clips


def one(workload: str, call: str, args) -> dict:
    import torch
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    keys, idx, clips = make_case(workload)
    stacked = np.stack(clips) if workload == "control" else None

    def loop():
        if stacked is not None:
            return list(eng.embed(keys[0], stacked, seed=SEED).audio)
        return [eng.embed(keys[k], c, seed=SEED).audio for k, c in zip(idx, clips)]

    def batch():
        return [r.audio for r in eng.embed_batch(keys, idx, clips, seed=SEED)]
    res = {"workload": workload, "call": call, "clips": len(clips), "samples": int(sum(c.size for c in clips))}
    if call == "mix":                                                       # the ragged mix launch alone, by device events
        from echoseal_amd.engine import embed_layout
        lengths = np.array([c.size for c in clips], np.int64)
        lay = embed_layout(lengths, 0)
        stride = (int(lengths.max()) + 3) // 4 * 4
        pad = np.zeros((len(clips), stride), np.float32)
        for j, c in enumerate(clips):
            pad[j, :c.size] = c
        x = torch.from_numpy(pad).to(eng.device)
        ring = eng.keyring(keys)
        ctr = torch.from_numpy(lay.ctr).to(eng.device)
        kf = torch.from_numpy(np.array(idx, np.int32)[lay.clip]).to(eng.device)
        frames = eng.make_frames_keyed(ring, kf, ctr, eng.seal_keyed(ring, kf, *eng._synthetic_plain(ctr, SEED)))
        ld, bd, cd = (torch.from_numpy(a).to(eng.device) for a in (lengths, lay.chip_base, lay.chip_cnt))
        out = torch.empty_like(x)
        us = []
        for k in range(args.repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.mix_ragged(x, ld, frames, bd, cd, out=out)
            b.record()
            torch.cuda.synchronize()
            if k:
                us.append(a.elapsed_time(b) * 1e3)
        us.sort()
        res.update({"median_us": us[len(us) // 2], "min_us": us[0], "max_us": us[-1], "bytes": 12 * res["samples"],
                    "padded_samples": int(len(clips) * stride), "gbytes_per_s": 12 * res["samples"] / (us[len(us) // 2] * 1e-6) / 1e9})
        return res
    fn = batch if call == "batch" else loop
    first = fn()                                                            # warm-up
    torch.cuda.synchronize()
    if call == "batch":                                                     # the same bytes as the loop it replaces
        want = loop()
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(first, want)) and len(first) == len(want)
    del first
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    res.update({"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "repeats": len(ms), "ms_per_clip": ms[len(ms) // 2] / len(clips)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds for each timing")
    ap.add_argument("--workloads", default="distinct64,distinct512,control")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=2, metavar=("WORKLOAD", "CALL"), help="(internal) run one timing in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one[0], args.one[1], args)))
        return 0
    lines, status = [], 0
    plan = [(w, c, r) for w in args.workloads.split(",") for r in range(args.runs) for c in ("batch", "loop")]
    plan += [(w, "mix", 0) for w in args.workloads.split(",")]
    for workload, call, run in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", workload, call, "--repeats", str(args.repeats)]
        try:
            p = subprocess.run(cmd, timeout=args.limit, capture_output=True, text=True)
            rec = json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0 else {"workload": workload, "call": call, "error": f"exit status {p.returncode}", "stderr": p.stderr[-600:]}
        except subprocess.TimeoutExpired:
            rec = {"workload": workload, "call": call, "error": f"no result within {args.limit} s"}
        rec.update({"run": run, "tag": args.tag})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if "error" in rec:
            status = 1
            break                                                           # nothing more is started on the device after a failure
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
