#!/usr/bin/env python3
"""Embedding throughput: R recordings of `seconds` at 48 kHz, block 1024 (the reference's own).

    python tools/embed_bench.py [--recordings 256] [--seconds 5] [--repeats 30] [--out profiles/embed_bench.json]

On a GPU: the mix launch alone (es_mix_batch over resident audio and chips) and RxEngine.embed end to end (payload synthesis,
AEAD seal, polar encode, schedule, frame generator, mix), timed with device events after warm-up; median and spread over the
repeats; achieved bytes per second of the mix at its 12 algorithmic bytes per sample (x in, chips in, out) next to the 8 TB/s
the project grades its streaming kernels against.  Without a GPU: the host WatermarkEmbedder.process loop
over the same input (fewer recordings by default, it is slow), the only path there was before es_mix_batch.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
KEY = bytes(range(32))


def make_audio(R, n, seed=1):
    rng = np.random.default_rng(seed)
    env = np.abs(np.sin(np.linspace(0, 9, n)))[None, :] * rng.uniform(0.05, 0.7, (R, 1))      # quiet to loud passages, no clipping
    return (env * rng.standard_normal((R, n)) * 0.3).astype(np.float32)


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "repeats": len(ms)}


def gpu(args, n):
    import torch
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    R = args.recordings
    x = torch.from_numpy(make_audio(R, n)).to(eng.device)
    nf = -(-n // 1215)
    first = eng.embed(KEY, x, seed=7)
    frames, _ = eng.synthetic_frames(KEY, 0, nf)
    chips = frames.reshape(1, -1).repeat(R, 1).contiguous()
    out = torch.empty_like(x)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return spread(ms)
    mix = timed(lambda: eng.mix(x, chips, out=out))
    e2e = timed(lambda: eng.embed(KEY, x, seed=7))
    again = eng.embed(KEY, x, seed=7)
    assert torch.equal(first.audio, again.audio)
    byts = 12.0 * R * n
    res = {"device": torch.cuda.get_device_name(0), "recordings": R, "samples": n, "block": 1024,
           "mix": dict(mix, bytes=byts, bytes_per_s=byts / (mix["median_ms"] * 1e-3), share_of_hbm=byts / (mix["median_ms"] * 1e-3) / HBM_PEAK),
           "embed_end_to_end": dict(e2e, audio_seconds_per_second=R * args.seconds / (e2e["median_ms"] * 1e-3)),
           "checksum": float(first.audio.double().abs().sum().item())}
    return res


def cpu(args, n):
    from echoseal_amd.embedder import WatermarkEmbedder, synthetic_payloads
    R = args.host_recordings
    x = make_audio(R, n)
    t0 = time.perf_counter()
    acc = 0.0
    for r in range(R):
        tx = WatermarkEmbedder(KEY)
        ctrs = iter(range(1 << 30))
        tx._build_payload = lambda tx=tx, ctrs=ctrs: synthetic_payloads(tx.sec, [next(ctrs)], seed=7)[0]
        y = np.concatenate([tx.process(x[r, s:s + 1024]) for s in range(0, n, 1024)])
        acc += float(np.abs(y).sum(dtype=np.float64))
    dt = time.perf_counter() - t0
    return {"device": "host NumPy (WatermarkEmbedder.process loop)", "recordings": R, "samples": n, "block": 1024,
            "host_process": {"seconds": dt, "ms_per_recording": 1e3 * dt / R, "audio_seconds_per_second": R * args.seconds / dt}, "checksum": acc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", type=int, default=256)
    ap.add_argument("--host-recordings", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="time the host loop even where a GPU is present")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = int(round(args.seconds * 48_000))
    import torch
    res = cpu(args, n) if (args.host or not torch.cuda.is_available()) else gpu(args, n)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
