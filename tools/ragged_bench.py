#!/usr/bin/env python3
"""A queue of uploads through verify_batch and identify_batch: clips of 64 distinct lengths against 64 clips of one length.

    python tools/ragged_bench.py [--clips 64] [--list-size 8] [--keys 4] [--repeats 3] [--limit 300] [--tag NAME] [--out profiles/ragged_bench.json]

Two workloads, each through WatermarkDetector.verify_batch and WatermarkIdentifier.identify_batch (--keys keys):
  distinct   --clips clips of as many distinct lengths between 1 s and 6 s at 48 kHz: seeded noise plus slices of the clip of
             tests/golden/verify3s.npz (what a service's queue looks like: no two recordings share a length to the sample);
  equal      --clips clips of exactly 3 s, made the same way.
Only those two public calls are used, so the same file runs on a checkout of an earlier commit (copy it there): that is how a change
to the batching is measured.  Each of the four timings runs in a child process of its own under a time limit of its own (--limit
seconds), wall clock around the call with the device idle before and after, one warm-up call and --repeats timed ones; after a
timing that fails or runs out of time no further one is started.  Prints one JSON line (and appends it to --out).
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
OWN = b"\xAA" * 32


def make_clips(workload: str, n: int):
    gold = np.load(os.path.join(ROOT, "tests", "golden", "verify3s.npz"))["clip"].astype(np.float32)
    rng = np.random.default_rng(2026)
    if workload == "equal":
        lengths = [3 * FS] * n
    else:                                                                   # n distinct lengths, 1 s .. 6 s, in no order
        step = (5 * FS) // max(1, n - 1)
        lengths = [FS + i * step - (i * 37) % 101 for i in range(n)]
        lengths = [lengths[i] for i in rng.permutation(n)]
        assert len(set(lengths)) == n
    clips = []
    for i, m in enumerate(lengths):
        off = (i * 4099) % gold.size
        body = np.resize(np.roll(gold, -off), m)                            # golden-clip slices, repeated for the clips above 3 s
        clips.append((body + rng.normal(0, 0.02, m)).astype(np.float32))
    return clips


def one(workload: str, call: str, args) -> dict:
    import torch
    from echoseal_amd.detector import WatermarkDetector
    from echoseal_amd.engine import RxEngine
    from echoseal_amd.identify import WatermarkIdentifier
    eng = RxEngine(0, list_size_max=max(32, args.list_size))
    clips = make_clips(workload, args.clips)
    if call == "verify":
        def fn():
            return WatermarkDetector(OWN, list_size=args.list_size, engine=eng).verify_batch(clips, FS)
    else:
        rng = np.random.default_rng(1)
        ident = WatermarkIdentifier([rng.bytes(32) for _ in range(args.keys - 1)] + [OWN], list_size=args.list_size, engine=eng)

        def fn():
            return ident.identify_batch(clips, FS)
    first = fn()                                                            # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert [bool(r) if call == "verify" else [m is not None for m in r] for r in res] == \
               [bool(r) if call == "verify" else [m is not None for m in r] for r in first]
    ms.sort()
    return {"workload": workload, "call": call, "clips": len(clips), "samples": int(sum(c.size for c in clips)),
            "median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "repeats": len(ms), "ms_per_clip": ms[len(ms) // 2] / len(clips)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--keys", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds for each of the four timings")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=2, metavar=("WORKLOAD", "CALL"), help="(internal) run one timing in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one[0], args.one[1], args)))
        return 0
    res = {"tag": args.tag, "list_size": args.list_size, "keys": args.keys, "timings": []}
    status = 0
    for workload in ("distinct", "equal"):
        for call in ("verify", "identify"):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", workload, call, "--clips", str(args.clips), "--list-size", str(args.list_size),
                   "--keys", str(args.keys), "--repeats", str(args.repeats)]
            try:
                p = subprocess.run(cmd, timeout=args.limit, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                res["timings"].append({"workload": workload, "call": call, "error": f"no result within {args.limit} s"})
                status = 1
                break
            if p.returncode != 0:
                res["timings"].append({"workload": workload, "call": call, "error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]})
                status = 1
                break
            res["timings"].append(json.loads(p.stdout.strip().splitlines()[-1]))
        if status:
            break                                                           # nothing more is started on the device after a failure
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
