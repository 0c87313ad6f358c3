#!/usr/bin/env python3
"""Golden vectors of the reference's level mix, WatermarkEmbedder.process (rtwm/embedder.py:44-75): build container only.

    python tools/gen_golden_embed.py        # writes tests/golden/embed_mix.npz

The reference is loaded through the oracle's shim (by name: nothing under tools/ imports the oracle package at module level, and
nothing in the product does at all), its `_build_payload` is replaced by seeded payloads that are recorded, its prints are
swallowed.  Per case the file holds: the block length, the first frame counter, the input recording, the payload of every frame
the reference generated and the concatenated outputs of process() called block by block.  Only data, none of the reference's text.

The inputs ramp from digital silence to beyond full scale, so that the absolute floor, the RMS-proportional gain, the headroom
limit and scale = 0 all occur; one case carries a NaN in one block, one an infinity.
"""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

KEY = bytes(range(32))
N = 19_000                                   # 0.4 s at 48 kHz; every block length below leaves a short last block
CASES = (                                    # (block, first counter, special sample: (index, value) or None)
    (1024, 0, None),
    (480, 65_534, (7_000, np.nan)),          # the header's 16-bit counter wraps inside the recording
    (1215, 2 ** 32 - 3, (11_111, np.inf)),   # the 32-bit counter wraps
    (9000, 7, None),                         # blocks beyond NumPy's 8192-element reduction buffer
)


def recording(rng, special):
    t = np.arange(N, dtype=np.float64) / N
    amp = np.where(t < 0.12, 0.0, 1.35 * (np.maximum(t - 0.12, 0.0) / 0.88) ** 2.2)          # silence, then quiet ... loud ... clipping
    x = (amp * rng.uniform(-1.0, 1.0, N)).astype(np.float32)
    x[int(0.2 * N):int(0.2 * N) + 700] *= np.float32(1e-3)                       # a passage near the floor
    if special is not None:
        x[special[0]] = special[1]
    return x


def main():
    load_reference = importlib.import_module("oracle.refshim.shim").load_reference
    load_reference()
    from rtwm.embedder import WatermarkEmbedder
    rng = np.random.default_rng(20261016)
    out = {"key": np.frombuffer(KEY, np.uint8), "count": np.array(len(CASES))}
    sink = io.StringIO()
    for i, (block, ctr0, special) in enumerate(CASES):
        x = recording(rng, special)
        payloads = []

        def seeded_payload(self):
            p = rng.integers(0, 256, 55, dtype=np.uint8)
            payloads.append(p)
            return p.tobytes()
        with contextlib.redirect_stdout(sink), np.errstate(all="ignore"):
            tx = WatermarkEmbedder(KEY)
            tx.frame_ctr = ctr0
            tx._build_payload = types.MethodType(seeded_payload, tx)
            y = np.concatenate([tx.process(x[s:s + block]) for s in range(0, N, block)])
        assert y.dtype == np.float32 and y.shape == x.shape
        t = f"case{i}"
        out[f"{t}/block"] = np.array(block)
        out[f"{t}/ctr0"] = np.array(ctr0, dtype=np.int64)
        out[f"{t}/x"] = x
        out[f"{t}/payloads"] = np.stack(payloads)
        out[f"{t}/y"] = y
        out[f"{t}/ctr_end"] = np.array(tx.frame_ctr, dtype=np.int64)
        print(f"{t}: block {block}, {len(payloads)} frames, frame_ctr {ctr0} -> {tx.frame_ctr}, "
              f"NaN out {int(np.isnan(y).sum())}, unchanged {int((y == x).sum())}", file=sys.stderr)
    path = os.path.join(ROOT, "tests", "golden", "embed_mix.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
