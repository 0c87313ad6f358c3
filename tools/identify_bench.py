#!/usr/bin/env python3
"""Identification time: which of N keys marked a clip?

    python tools/identify_bench.py [--keys 256 4096] [--list-size 8] [--repeats 30] [--loop-keys 256] [--out profiles/identify_bench.json]

One process, one engine, the clip of tests/golden/verify3s.npz, N random keys plus the clip's own (0xAA...).  Timed with device
events after warm-up, median and spread over the repeats (above 1 024 keys, where a call takes seconds, a sixth of the repeats):
  (a) WatermarkIdentifier.identify over N keys (conditioning and sync once, everything keyed from the key ring on the device);
  (b) the only path there was before: [WatermarkDetector(k, list_size=L, engine=e).verify(clip, 48_000) for k in keys] at
      --loop-keys keys (each detector fresh, as identify defines its answer), --loop-repeats times;
  (c) candidates decoded per second in (a): four list decodes per candidate (two PN variants, two signs).
Checks that (a) and (b) give the same booleans.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OWN = b"\xAA" * 32


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "repeats": len(ms)}


def keys_for(n, seed=1):
    rng = np.random.default_rng(seed)
    return [rng.bytes(32) for _ in range(n)] + [OWN]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--loop-keys", type=int, default=256)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--loop-repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from echoseal_amd.detector import WatermarkDetector
    from echoseal_amd.engine import RxEngine
    from echoseal_amd.identify import WatermarkIdentifier
    clip = np.load(os.path.join(ROOT, "tests", "golden", "verify3s.npz"))["clip"]
    L = args.list_size
    eng = RxEngine(0, list_size_max=max(32, L))

    def timed(fn, repeats, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return spread(ms)

    res = {"device": torch.cuda.get_device_name(0), "clip_samples": int(clip.size), "list_size": L, "identify": {}}
    answers = {}
    for n in args.keys:
        keys = keys_for(n)
        ident = WatermarkIdentifier(keys, list_size=L, engine=eng)
        ident.trace = True
        _m, traces = ident.identify(clip, 48_000)
        ident.trace = False
        cands = sum(len(t[0]) for t in traces)
        many = n > 1024                                                     # seconds per call up there: fewer repeats
        t = timed(lambda: ident.identify(clip, 48_000), max(3, args.repeats // 6) if many else args.repeats, 1 if many else args.warmup)
        answers[n] = [m is not None for m in ident.identify(clip, 48_000)]
        res["identify"][str(n + 1)] = dict(t, keys=n + 1, candidates=cands, matches=int(sum(answers[n])),
                                           candidates_per_s=cands / (t["median_ms"] * 1e-3), list_decodes_per_s=4 * cands / (t["median_ms"] * 1e-3))
    n = args.loop_keys
    keys = keys_for(n)
    loop_out = []

    def loop():
        loop_out[:] = [WatermarkDetector(k, list_size=L, engine=eng).verify(clip, 48_000) for k in keys]
    t = timed(loop, args.loop_repeats, 1)
    res["detector_loop"] = dict(t, keys=n + 1, ms_per_key=t["median_ms"] / (n + 1))
    if n in answers:
        assert loop_out == answers[n], "identify and the per-key detector loop disagree"
        res["speedup_at_%d" % (n + 1)] = t["median_ms"] / res["identify"][str(n + 1)]["median_ms"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
