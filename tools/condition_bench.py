#!/usr/bin/env python3
"""A queue of uploads at mixed sample rates through verify_batch, and the conditioning launch alone.

    python tools/condition_bench.py [--parent TREE] [--runs 3] [--workloads pcm441,mixed,control] [--clips 64] [--list-size 8] [--repeats 3] [--limit 300] [--out profiles/condition_bench.json]
    python tools/condition_bench.py --kernel            # the resampling launch alone, by device events

64 clips of distinct lengths between 1 s and 6 s (the content of tools/ragged_bench.py's queue, converted on the host), three workloads:
  pcm441     every clip 44.1 kHz int16;
  mixed      clips at 16, 32, 44.1, 48 and 96 kHz in turn, float32;
  control    every clip at 48 kHz, float32: a call that does not condition anything.
Each timing is WatermarkDetector.verify_batch at --list-size in a child process of its own under a time limit of its own (--limit
seconds): wall clock around the call with the device idle before and after, one warm-up call and --repeats timed ones.  Only that
public call is used, so with --parent TREE (a built checkout of the parent commit) the same timings run on the parent's package, parent
and this tree alternately, --runs runs each.  After a timing that fails or runs out of time no further one is started.  Every line is
printed and appended to --out.

--kernel: 64 clips of 3 s at 44.1 kHz, float32, already on the device; es_resample_ragged_batch (one launch, rep 1 and 4) next to
es_resample_batch on the same clips stacked [64, n]; median of --repeats launches by device events after one warm-up, in bytes moved
(samples read + samples written) per second.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 48_000
OWN = b"\xAA" * 32
WORKLOADS = ("pcm441", "mixed", "control")
MIX = (16_000, 32_000, 44_100, 48_000, 96_000)


def make_queue(workload: str, n: int):
    """-> (clips, rates): the queue at 48 kHz first (distinct lengths, golden-clip slices in noise), then each clip at its upload rate."""
    from math import gcd
    from scipy.signal import resample_poly
    gold = np.load(os.path.join(HERE, "tests", "golden", "verify3s.npz"))["clip"].astype(np.float32)
    rng = np.random.default_rng(2026)
    step = (5 * FS) // max(1, n - 1)
    lengths = [FS + i * step - (i * 37) % 101 for i in range(n)]
    lengths = [lengths[i] for i in rng.permutation(n)]
    assert len(set(lengths)) == n
    clips, rates = [], []
    for i, m in enumerate(lengths):
        body = (np.resize(np.roll(gold, -((i * 4099) % gold.size)), m) + rng.normal(0, 0.02, m)).astype(np.float32)
        fs = {"pcm441": 44_100, "mixed": MIX[i % len(MIX)], "control": FS}[workload]
        if fs != FS:
            g = gcd(fs, FS)
            body = resample_poly(body.astype(np.float64), fs // g, FS // g).astype(np.float32)
        if workload == "pcm441":
            body = np.clip(np.round(body.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)
        clips.append(body); rates.append(fs)
    return clips, rates


def one(workload: str, args) -> dict:
    root = os.path.abspath(args.root) if args.root else HERE
    sys.path.insert(0, root)
    import torch
    import echoseal_amd
    from echoseal_amd.detector import WatermarkDetector
    from echoseal_amd.engine import RxEngine
    assert os.path.dirname(os.path.dirname(os.path.abspath(echoseal_amd.__file__))) == root
    eng = RxEngine(0, list_size_max=max(32, args.list_size))
    clips, rates = make_queue(workload, args.clips)

    def fn():
        return WatermarkDetector(OWN, list_size=args.list_size, engine=eng).verify_batch(clips, rates)
    first = fn()                                                            # warm-up
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert res == first
    ms.sort()
    return {"workload": workload, "clips": len(clips), "samples": int(sum(c.size for c in clips)), "median_ms": ms[len(ms) // 2], "min_ms": ms[0],
            "max_ms": ms[-1], "repeats": len(ms), "accepted": int(sum(first))}


def kernel(args) -> dict:
    sys.path.insert(0, HERE)
    import torch
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    rng = np.random.default_rng(7)
    B, n = args.clips, 3 * 44_100
    x = torch.from_numpy((rng.standard_normal((B, n)) * 0.1).astype(np.float32)).to(eng.device)
    clips = list(x.unbind(0))
    plan = eng.condition_upload([n] * B, 44_100, FS, np.float32)
    n_out = int(plan.plan.n_out[0])

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return sorted(ms)[len(ms) // 2]
    pool = torch.cat(clips)
    res = {"kernel": True, "clips": B, "n_in": n, "n_out": n_out, "launches": []}
    from echoseal_amd.utils import resample_plan
    h_tf, hpp, up, down, y0, _, _ = resample_plan(n, FS, 44_100, np.float32)
    hd = torch.from_numpy(h_tf).to(eng.device)
    ref = torch.empty((B, n_out), dtype=torch.float32, device=eng.device)
    st = torch.cuda.current_stream(eng.device).cuda_stream

    def old():
        assert eng._lib.es_resample_batch(eng._ctx, x.data_ptr(), 0, B, n, hd.data_ptr(), hpp, up, down, y0, n_out, ref.data_ptr(), st) == 0
    t = timed(old)
    res["launches"].append({"entry": "es_resample_batch", "rep": 1, "ms": t, "GB_per_s": 4 * B * (n + n_out) / t / 1e6})
    for rep in (1, 4):
        out = torch.zeros((B * rep, (n_out + 3) // 4 * 4), dtype=torch.float32, device=eng.device)

        def fn():
            assert eng._lib.es_resample_ragged_batch(eng._ctx, pool.data_ptr(), 0, pool.numel(), plan.filt.data_ptr(), plan.filt.numel(),
                                                     plan.desc.data_ptr(), B, rep, out.data_ptr(), out.shape[1], n_out, st) == 0
        t = timed(fn)
        assert torch.equal(out[::rep, :n_out], ref)
        res["launches"].append({"entry": "es_resample_ragged_batch", "rep": rep, "ms": t, "GB_per_s": 4 * B * (n + rep * n_out) / t / 1e6})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3, help="runs of every workload on each tree")
    ap.add_argument("--limit", type=int, default=300, help="seconds for each timing")
    ap.add_argument("--workloads", default=",".join(WORKLOADS), help="comma-separated subset of " + ", ".join(WORKLOADS))
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, timed alternately with this tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--root", default=None, help="(internal) the tree whose package a child imports")
    ap.add_argument("--one", metavar="WORKLOAD", help="(internal) run one timing in this process")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(one(args.one, args)))
        return 0
    lines, status = [], 0

    def child(extra, tree):
        cmd = [sys.executable, os.path.abspath(__file__), "--clips", str(args.clips), "--list-size", str(args.list_size), "--repeats", str(args.repeats)] + extra
        try:
            p = subprocess.run(cmd, timeout=args.limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            return {"tree": tree, "args": extra, "error": f"no result within {args.limit} s"}
        if p.returncode != 0:
            return {"tree": tree, "args": extra, "error": f"exit status {p.returncode}", "stderr": p.stderr[-400:]}
        return dict(json.loads(p.stdout.strip().splitlines()[-1]), tree=tree)
    if args.kernel:
        lines.append(kernel(args))
    else:
        trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", HERE)]
        for run in range(args.runs):
            for workload in [w for w in WORKLOADS if w in args.workloads.split(",")]:
                for tree, root in trees:                                    # parent and this tree alternately
                    lines.append(dict(child(["--one", workload, "--root", root], tree), run=run))
                    status = int("error" in lines[-1])
                    if status:
                        break
                if status:
                    break
            if status:
                break                                                       # nothing more is started on the device after a failure
    for line in lines:
        print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return status


if __name__ == "__main__":
    sys.exit(main())
