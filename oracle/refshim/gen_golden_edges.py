#!/usr/bin/env python3
"""Demodulator and header decoder at the payload-length edges, captured by RUNNING the reference (build container only;
/root/reference is read-only and never travels).  Only inputs and outputs are stored under tests/golden/ -- no reference source.

    python -m oracle.refshim.gen_golden_edges

    front_edges.npz   for fs_target in (48 000, 211 790): the reference's own WatermarkDetector._llr (PN variants 0 and 1) and
                      _decode_header (rtwm/detector.py:296-416, 452-515) on
                        * every payload length 1 .. 64 and a spread up to 1 024, in all four bands: a frame of the reference
                          embedder at -6 / 0 / +6 dB SNR, band-passed by the reference's design, cut 191 + length samples after
                          its start (a causal filter: the prefix of the band-passed window is what a window ending there gives);
                        * header lengths 189 .. 200 (frame slices shorter than, equal to and just above preamble + header);
                        * degenerate rows: silence, a constant, a single spike, period-7 and period-64 rows, +-A alternation,
                          noise at amplitudes 1e15 and 1e-20, noise only.
                      Per record: the frame slice (float32-exact float64: both functions cast to float32 first), counter, band,
                      _llr of both variants, the chosen shift of each (from the function's own log line, as gen_golden_r2 does),
                      and (ok, val, score, best_s) of _decode_header.  The header's chosen shift is a local of the real function:
                      it is read from the function's frame when it returns (sys.setprofile).
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLD = os.path.join(ROOT, "tests", "golden")
KEY = b"\xAA" * 32
RATES = (48_000, 211_790)
SHORT = tuple(range(1, 65))
SPREAD = (65, 96, 127, 128, 129, 191, 256, 383, 512, 700, 1000, 1023, 1024)
HDR_LENS = tuple(range(189, 201))
FRAME_AT = 600                 # frame start inside the 2 048-sample window
T_WIN = 2048


def degenerate_rows(np):
    """Rows the detector sees directly (no band-pass): name -> float64 [1215], float32-exact."""
    rng = np.random.default_rng(77)
    i = np.arange(1215)
    rows = {
        "silence": np.zeros(1215),
        "constant": np.full(1215, 0.25),
        "spike": np.where(i == 400, 1.0, 0.0),
        "period7": np.sin(2 * np.pi * i / 7.0),
        "period64": ((i % 64) < 32).astype(np.float64) - 0.5,
        "alternating": np.where(i % 2 == 0, 0.5, -0.5),
        "noise_1e15": 1e15 * rng.standard_normal(1215),
        "noise_1e-20": 1e-20 * rng.standard_normal(1215),
        "noise": 0.1 * rng.standard_normal(1215),
    }
    return {k: v.astype(np.float32).astype(np.float64) for k, v in rows.items()}


def main():
    import numpy as np
    from scipy.signal import lfilter
    from oracle.refshim.shim import load_reference
    load_reference()
    from rtwm.detector import WatermarkDetector
    from rtwm.utils import choose_band, BAND_PLAN, butter_bandpass
    from oracle.refshim.gen_golden_r2 import ref_frames, best_s_from
    ctrs = []
    for b in range(4):                                              # one counter per band (the detector derives the band from it)
        ctrs.append(next(c for c in range(64) if BAND_PLAN.index(choose_band(KEY, c)) == b))
    frames, _ = ref_frames(np, ctrs)
    rng = np.random.default_rng(2026)
    degen = degenerate_rows(np)

    hdr_best = []

    def profiler(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "_decode_header":
            hdr_best.append(int(frame.f_locals.get("best_s", 0)))

    recs = {k: [] for k in ("fs", "ctr", "band", "kind", "flen", "llr0", "llr1", "best_s", "hdr")}
    slices = []
    sink = io.StringIO()
    for fs in RATES:
        with contextlib.redirect_stdout(sink):
            rx = WatermarkDetector(KEY, fs_target=fs, list_size=8)
        jobs = []                                                   # (kind, ctr, band, frame slice)
        for b, ctr in enumerate(ctrs):
            for snr_db in (-6.0, 0.0, 6.0):
                win = np.zeros(T_WIN, np.float32)
                win[FRAME_AT:FRAME_AT + 1215] = frames[b]
                rms = float(np.sqrt(np.mean(frames[b].astype(np.float64) ** 2)))
                win += (rng.standard_normal(T_WIN) * rms * 10 ** (-snr_db / 20)).astype(np.float32)
                bb, aa = butter_bandpass(*BAND_PLAN[b], fs, order=4)
                y = lfilter(bb, aa, win).astype(np.float32).astype(np.float64)
                lens = [L for k, L in enumerate(SHORT + SPREAD) if k % 3 == int(snr_db / 6) + 1]    # each length at one SNR
                for L in lens:
                    jobs.append((0, ctr, b, y[FRAME_AT:FRAME_AT + 191 + L]))
                if snr_db == 0.0:
                    for fl in HDR_LENS:
                        jobs.append((1, ctr, b, y[FRAME_AT:FRAME_AT + fl]))
        for k, (name, row) in enumerate(degen.items()):
            b = k % 4
            jobs.append((2 + k, ctrs[b], b, row))
        for kind, ctr, b, fr in jobs:
            band = BAND_PLAN[b]
            with contextlib.redirect_stdout(sink):
                sink.seek(0); sink.truncate()
                l0 = rx._llr(fr, ctr, 0)
                l1 = rx._llr(fr, ctr, 1)
                del hdr_best[:]
                sys.setprofile(profiler)
                try:
                    h = rx._decode_header(fr, band)
                finally:
                    sys.setprofile(None)
            b_s = best_s_from(sink.getvalue())
            short = fr.size <= 191
            assert len(b_s) == (0 if short else 2), (fs, kind, fr.size, b_s)
            assert len(hdr_best) == 1
            recs["fs"].append(fs); recs["ctr"].append(ctr); recs["band"].append(b); recs["kind"].append(kind)
            recs["flen"].append(fr.size); recs["llr0"].append(l0); recs["llr1"].append(l1)
            recs["best_s"].append(b_s if b_s else [0, 0])
            recs["hdr"].append((float(h[0]), float(h[1]), float(h[2]), float(hdr_best[0])))
            slices.append(fr)
            print(f"  fs {fs} kind {kind} band {b} flen {fr.size} best_s {recs['best_s'][-1]} hdr {recs['hdr'][-1]}", flush=True)
    off = np.concatenate([[0], np.cumsum([s.size for s in slices])]).astype(np.int64)
    out = dict(fs=np.array(recs["fs"], np.int32), ctr=np.array(recs["ctr"], np.int64), band=np.array(recs["band"], np.uint8),
               kind=np.array(recs["kind"], np.int32), flen=np.array(recs["flen"], np.int32),
               samples=np.concatenate(slices).astype(np.float32), offsets=off,
               llr0=np.stack(recs["llr0"]).astype(np.float32), llr1=np.stack(recs["llr1"]).astype(np.float32),
               best_s=np.array(recs["best_s"], np.int32), hdr=np.array(recs["hdr"], np.float64),
               degenerate_names=np.array(list(degen.keys())))
    np.savez_compressed(os.path.join(GOLD, "front_edges.npz"), **out)
    print("wrote", os.path.join(GOLD, "front_edges.npz"), len(slices), "records")


if __name__ == "__main__":
    main()
