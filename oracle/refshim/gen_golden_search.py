#!/usr/bin/env python3
"""Golden traces of the reference's whole-recording search at every branch (build container only, CPU only).

    python -m oracle.refshim.gen_golden_search     # writes tests/golden/search_traces.npz

verify() and _scan_band_multi_frame (rtwm/detector.py:44-152) decide which band comes first, which peaks are looked at, which window
each peak's counters come from and when the 400-try budget ends a band.  verify_trace.npz and verify3s.npz pin that order on two clips
under one key; the clips here are found by a seeded search so that between them the reference goes through every branch of that code:

    a      a band ends at 400 tries inside a peak's candidate list
    b      a band ends at 400 tries exactly at a peak's last candidate (bounded search; absent from `cases` when no seed gave one)
    c      a band with more than 25 peaks above threshold and fewer than 400 tries: PEAK_LIMIT ends it, and peak 26 could hold a frame
    d      a fallback band (top 5, descending correlation) with a peak that cannot hold a frame ahead of one that can (1 300-2 500 samples)
    e      a header-gated peak without candidates, failed headers that take the +-3 and the +-200 window, all in one clip
    f      5.2 s or more of exact zeros, then 0.3 s marked from counter 205: every estimate is above 200, so no window starts at 0,
           some +-200 window begins with its very first counter, est - 200, and -- by the length of the lead -- one header decodes
           to the estimate of its own peak: the header-gated peak WITH a candidate
    h*     clips at 44 100, 32 000 (float64), 96 000 and 24 000 Hz
    i*     62, 63, 1 214, 1 215 and 1 216 samples with a marked frame at sample 0
    (g)    the own keys of the cases are four keys whose counter 0 hops to the four different bands
    (j)    every clip also runs under two stranger keys

What is stored is read from the REAL functions: every try from the log lines ("Peak@", "Trying ctr="), thr / peaks / tried from the
locals of _scan_band_multi_frame's frame when it returns (sys.setprofile; `k` exists only where the fallback ran), header results from
the return values of _decode_header.  Which window a failed header took is worked out with the reference's choose_band and checked
against the candidate count the log line gives.  Own-key runs use the reference's real decode at list_size = 1; stranger-key runs and
the seed search replace _try_decode_frame by `return False`, which touches no search state: the two smallest own-key cases are
captured both ways and the traces asserted equal.

The declared ambiguities of DESIGN section 2 are kept out: no fallback band with two equal values among its six largest, no band whose
correlation is identically zero (checked for every band of every run, own key and strangers; a seed that has one is passed over).

Header scores.  The bar on a header score is 1e-6 relative.  The reference convolves the header slice with the matched
filter in float32 (np.convolve of two float32 arrays, rtwm/detector.py:473); where the chosen shift lies in a stretch with next to no
signal -- a band above the Nyquist rate of a clip that came in at 24 kHz holds resampler residue only -- that rounding alone moves its
score by more than the bar: 1.25e-6 at one peak of the first 24 kHz seed, against the function's own formula evaluated in float64 on
its own float32 inputs at its own shift.  Such a score is the reference's rounding, not its rule, so a seed is also passed over when
any visited peak's score, under the own key or a stranger, is more than SCORE_NOISE = 5e-7 from that float64 value: half the bar, which
leaves the other half to an implementation that rounds to float32 elsewhere (the C oracle and the kernels accumulate the convolution in
float64 and are within 3e-7 of the float64 value on these clips).  The float64 value of every visited peak is stored as `score_f64`.
"""
from __future__ import annotations

import contextlib
import hashlib
import io
import multiprocessing
import os
import re
import sys
import time
import types
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "search_traces.npz")
FRAME_LEN, PRE_L, MAX_TRIES, PEAK_LIMIT, TIGHT, WIDE = 1215, 63, 400, 25, 3, 200
GATED, TIGHT_WINDOW, WIDE_WINDOW = 0, 1, 2                                  # the window branch of a visited peak
FIELDS = ("result", "tries", "bands", "thr", "npeaks", "fallback", "peaks", "tried", "visited", "score", "score_f64")
SCORE_NOISE = 5e-7                                                          # see "Header scores" in the module's docstring


class Ambiguous(Exception):
    """The clip is one on which the reference's own answer is not settled to the bars: the search takes the next seed."""

B_TRIALS = 60                                                               # seeds per length looked at for case b before giving up
F_TRIALS = 24                                                               # seeds looked at for case f: the shortest lead among them


def derived_key(tag: str) -> bytes:
    return hashlib.sha256(("echoseal search traces: " + tag).encode()).digest()


def marked(np, emb_mod, key: bytes, n: int, noise: float, seed: int, ctr0: int = 0):
    """n samples of the reference embedder's output from counter ctr0 over silence (noise 0) or faint noise, float32; payloads are seeded
    random bytes (nothing here decodes: SURVEY section 0.2)."""
    rng = np.random.default_rng(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        tx = emb_mod.WatermarkEmbedder(key)
        tx.frame_ctr = ctr0
        tx._build_payload = types.MethodType(lambda self: rng.integers(0, 256, 55, dtype=np.uint8).tobytes(), tx)
        host = (noise * rng.standard_normal(n)).astype(np.float32) if noise else np.zeros(n, np.float32)
        return tx.process(host).astype(np.float32)


def reference_trace(np, det_mod, utils_mod, key: bytes, clip, fs_in: int, real: bool) -> dict:
    """Run the reference's verify(clip, fs_in) under `key` and return what its search did (FIELDS)."""
    sink = io.StringIO()
    with contextlib.redirect_stdout(sink):
        rx = det_mod.WatermarkDetector(key, list_size=1)
    scan_code = det_mod.WatermarkDetector._scan_band_multi_frame.__code__
    hdr_code = det_mod.WatermarkDetector._decode_header.__code__
    scans, hdrs, exact = [], [], []

    def profiler(frame, event, arg):
        if event != "return":
            return
        loc = frame.f_locals
        if frame.f_code is scan_code:
            scans.append({k: loc.get(k) for k in ("band", "thr", "peaks", "corr", "tried", "signal")} | {"fallback": "k" in loc})
        elif frame.f_code is hdr_code:
            if "sums" not in loc:                                           # the early return of a short slice: (False, 0, 0.0)
                exact.append(0.0)
                return
            # the function's own score formula in float64, on its own float32 inputs at its own shift (rtwm/detector.py:473, 498-512)
            mf = np.convolve(loc["seg_full"].astype(np.float64), loc["h"].astype(np.float64), mode="full")
            d = mf[loc["start"]:loc["stop"]][loc["i0"]:loc["i1"]] * loc["self"]._hdr_pn_sy.astype(np.float64)
            exact.append(float(np.mean(np.abs(d.reshape(16, 8).sum(axis=1))) / (np.std(d) + 1e-12)))

    orig_hdr, orig_try = type(rx)._decode_header, type(rx)._try_decode_frame

    def hdr_spy(self, frame, band):
        r = orig_hdr(self, frame, band)
        hdrs.append((bool(r[0]), int(r[1]), float(r[2])))
        return r

    def try_real(self, frame, ctr):                                         # the decode itself is not profiled: nothing of it is recorded
        sys.setprofile(None)
        try:
            return orig_try(self, frame, ctr)
        finally:
            sys.setprofile(profiler)

    rx._decode_header = types.MethodType(hdr_spy, rx)
    rx._try_decode_frame = types.MethodType(try_real if real else (lambda self, frame, ctr: False), rx)
    with contextlib.redirect_stdout(sink):
        sink.seek(0); sink.truncate()
        sys.setprofile(profiler)
        try:
            res = rx.verify(clip, fs_in)
        finally:
            sys.setprofile(None)
    assert res is False                                                     # the reference's own DSP cannot decode its frames
    bands, visited, scores, tries, bi = [], [], [], [], -1
    for line in sink.getvalue().splitlines():
        m = re.match(r"\[SCAN\] Band \((\d+), (\d+)\)", line)
        if m:
            bi += 1
            bands.append((int(m.group(1)), int(m.group(2))))
            continue
        m = re.match(r"\s+Peak@(\d+): ctr_est=(\d+), (?:hdr_lo16=0x([0-9A-F]{4}), score=\S+ )?trying (\d+) counters \((header gated|\S+ then \S+)\)", line)
        if m:
            start, est, ncand, gated = int(m.group(1)), int(m.group(2)), int(m.group(4)), m.group(5) == "header gated"
            ok, lo16, score = hdrs[len(visited)]
            assert ok == gated and (not gated or lo16 == int(m.group(3), 16)) and est == int(round(start / FRAME_LEN))
            hops = lambda c: utils_mod.choose_band(key, c) == bands[bi]
            wide = [c for c in range(max(0, est - WIDE), est + WIDE + 1) if hops(c)]
            tight = [c for c in range(max(0, est - TIGHT), est + TIGHT + 1) if hops(c)]
            branch, cands = (GATED, [c for c in wide if (c & 0xFFFF) == lo16]) if gated else (TIGHT_WINDOW, tight) if tight else (WIDE_WINDOW, wide)
            assert len(cands) == ncand, (start, est, branch, len(cands), ncand)
            visited.append((bands[bi][0], start, int(ok), lo16, ncand, branch)); scores.append(score)
            continue
        m = re.match(r"\s+Trying ctr=(\d+)$", line)
        if m:
            tries.append((bands[bi][0], visited[-1][1], int(m.group(1))))
    assert len(scans) == len(bands) and len(hdrs) == len(visited) == len(exact) and [s["band"] for s in scans] == bands
    noise = [abs(s - e) / max(1.0, abs(e)) for s, e in zip(scores, exact)]
    if noise and max(noise) > SCORE_NOISE:
        raise Ambiguous(f"a header score {max(noise):.2e} relative from the float64 value of its own formula")
    nb = len(bands)
    out = {"result": np.array(res), "tries": np.array(tries, np.int64).reshape(-1, 3), "bands": np.array([b[0] for b in bands], np.int64),
           "thr": np.full(nb, np.nan), "npeaks": np.zeros(nb, np.int64), "fallback": np.zeros(nb, bool), "peaks": np.full((nb, 32), -1, np.int64),
           "tried": np.zeros(nb, np.int64), "visited": np.array(visited, np.int64).reshape(-1, 6), "score": np.array(scores, np.float64),
           "score_f64": np.array(exact, np.float64)}
    for i, s in enumerate(scans):
        if s["corr"] is None:                                               # shorter than the template: rtwm/detector.py:71-73
            continue
        corr, peaks = s["corr"], [int(p) for p in s["peaks"]]
        if not corr.any():
            raise Ambiguous("a band's correlation is identically zero (DESIGN section 2)")
        if s["fallback"] and np.unique(np.sort(corr)[-6:]).size < min(6, corr.size):
            raise Ambiguous("a fallback band with equal values among its largest (DESIGN section 2)")
        out["thr"][i], out["npeaks"][i], out["fallback"][i], out["tried"][i] = s["thr"], len(peaks), s["fallback"], s["tried"]
        out["peaks"][i, :min(32, len(peaks))] = peaks[:32]
        fit = [p for p in peaks[:PEAK_LIMIT] if p + FRAME_LEN <= s["signal"].size]
        seen = [v[1] for v in visited if v[0] == bands[i][0]]
        assert seen == fit[:len(seen)] and (len(seen) == len(fit) or s["tried"] == MAX_TRIES)
        assert s["tried"] == sum(1 for t in tries if t[0] == bands[i][0])
    out["zero_corr"] = np.array([0 if s["corr"] is None else int((s["corr"] == 0).sum()) for s in scans], np.int64)
    out["length"] = np.array(max([s["signal"].size for s in scans], default=0))
    return out


# ----------------------------------------------------------------------------------------------- what a trace reaches
def band_rows(np, t: dict, i: int):
    """The visited peaks of the i-th band scanned, and how many candidates they had in all."""
    v = t["visited"][t["visited"][:, 0] == t["bands"][i]]
    return v, int(v[:, 4].sum())


def reaches(np, t: dict, length: int) -> set:
    """The branches of rtwm/detector.py:97-151 a trace went through, from its records alone (tests/test_golden_search.py states the same)."""
    got = set()
    for i in range(t["bands"].size):
        v, cands = band_rows(np, t, i)
        if t["tried"][i] == MAX_TRIES:
            got.add("a" if cands > MAX_TRIES else "b")
        if not t["fallback"][i] and t["npeaks"][i] > PEAK_LIMIT and t["tried"][i] < MAX_TRIES and 0 <= t["peaks"][i, PEAK_LIMIT] <= length - FRAME_LEN:
            got.add("c")
        if t["fallback"][i]:
            fits = [p + FRAME_LEN <= length for p in t["peaks"][i, :t["npeaks"][i]]]
            if any(not a and any(fits[j + 1:]) for j, a in enumerate(fits)):
                got.add("d")
    v = t["visited"]
    kinds = {(int(r[5]), bool(r[4] > 0)) for r in v}
    if {(GATED, False), (TIGHT_WINDOW, True), (WIDE_WINDOW, True)} <= kinds:
        got.add("e")
    if (GATED, True) in kinds:
        got.add("gated")
    est = (2 * v[:, 1] + FRAME_LEN) // (2 * FRAME_LEN)
    first = {(int(b), int(s)): int(c) for b, s, c in t["tries"][::-1]}      # the first counter tried at each (band, peak)
    if v.size and (est > WIDE).all() and any(r[5] == WIDE_WINDOW and first.get((int(r[0]), int(r[1]))) == e - WIDE for r, e in zip(v, est)):
        got.add("f")
    return got


_JOB: dict = {}                                                            # what a forked worker needs of main()


def _own_run(name: str):
    j, t1 = _JOB, time.time()
    clip, fs, ki = j["cases"][name]
    return reference_trace(j["np"], j["det"], j["utils"], j["keys"][ki], clip, fs, True), time.time() - t1


def main():
    import numpy as np
    from scipy.signal import resample_poly
    from oracle.refshim.shim import load_reference
    load_reference()
    import rtwm.detector as det_mod
    import rtwm.embedder as emb_mod
    import rtwm.utils as utils_mod
    t0 = time.time()
    say = lambda *a: print(f"[{time.time() - t0:6.1f} s]", *a, file=sys.stderr, flush=True)
    trace = lambda key, clip, fs, real=False: reference_trace(np, det_mod, utils_mod, key, clip, fs, real)

    # (g) four keys, one per band of counter 0; two strangers
    keys, n = {}, 0
    while len(keys) < 4:
        k = derived_key(f"key {n}"); n += 1
        keys.setdefault(utils_mod.BAND_PLAN.index(utils_mod.choose_band(k, 0)), k)
    keys = [keys[b] for b in range(4)]
    strangers = [derived_key("stranger 0"), derived_key("stranger 1")]
    cases: dict[str, tuple] = {}                                            # name -> (clip, fs_in, key index)

    def settled(key, clip, fs, wanted) -> bool:
        """The stubbed own-key trace has what is wanted, and neither it nor a stranger's is Ambiguous."""
        try:
            return bool(wanted(trace(key, clip, fs))) and all(trace(k, clip, fs) is not None for k in strangers)
        except Ambiguous:
            return False

    def search(name, want, lengths, first_key, trials, noise=(0.0, 1e-3)):
        """The first (length, seed) whose stubbed own-key trace reaches `want`; lengths ascend, so the shortest clip that does wins."""
        for n in lengths:
            for s in range(trials):
                ki = (first_key + s) % 4
                clip = marked(np, emb_mod, keys[ki], n, noise[s % len(noise)], 1000 * n + s)
                if settled(keys[ki], clip, 48_000, lambda t: want in reaches(np, t, n)):
                    cases[name] = (clip, 48_000, ki)
                    say(f"case {name}: {n} samples, seed {s}, key {ki}")
                    return True
        return False

    assert search("a", "a", (48_000, 72_000, 96_000), 0, 24)
    if not search("b", "b", (48_000, 96_000), 1, B_TRIALS):
        say(f"case b: none among 2 x {B_TRIALS} seeds")
    assert search("c", "c", (24_000, 36_000, 48_000), 2, 8)
    assert search("d", "d", (1_300, 1_700, 2_100, 2_500), 3, 16)
    assert search("e", "e", (12_000, 24_000, 36_000), 0, 16)
    # (f) exact zeros, then 0.3 s marked from counter 205 = round(249 600 / 1215).  The zeros leave the band-passed frames, hence their
    # peaks and header values, as they are, whatever their number; so the lead is lengthened by whole frames until the value one
    # header decodes to is the estimate of its own peak and hops to its band: the header-gated peak WITH a candidate, which no short
    # clip has (the reference's header decode does not return its frames' counters: values such as 0x0602 or 0x40b0).
    leads = []
    for s in range(F_TRIALS):
        ki = (1 + s) % 4
        try:
            t = trace(keys[ki], np.concatenate((np.zeros(249_600, np.float32), marked(np, emb_mod, keys[ki], 14_400, 0.0, 7000 + s, ctr0=205))), 48_000)
        except Ambiguous:
            continue
        for band, start, ok, lo16, _, _ in t["visited"]:
            est = (2 * start + FRAME_LEN) // (2 * FRAME_LEN)
            if ok and lo16 >= est and utils_mod.choose_band(keys[ki], int(lo16))[0] == band:
                leads.append((int(lo16 - est), s, ki))
    for frames, s, ki in sorted(leads):                                     # the shortest lead that also has a +-200 window starting at est - 200
        clip = np.concatenate((np.zeros(249_600 + frames * FRAME_LEN, np.float32), marked(np, emb_mod, keys[ki], 14_400, 0.0, 7000 + s, ctr0=205)))
        if settled(keys[ki], clip, 48_000, lambda t: {"f", "gated"} <= reaches(np, t, clip.size) and t["zero_corr"].min() > 200_000):
            cases["f"] = (clip, 48_000, ki)
            say(f"case f: seed {s}, key {ki}, {clip.size} samples ({clip.size / 48_000:.1f} s)")
            break
    assert "f" in cases
    # (h) other rates: half a second marked at 48 kHz, brought to the rate with SciPy in float64; one clip stays float64
    for j, (fs, dt) in enumerate(((44_100, np.float32), (32_000, np.float64), (96_000, np.float32), (24_000, np.float32))):
        g = int(np.gcd(fs, 48_000))
        for s in range(16):
            ki = (2 + j) % 4
            clip = resample_poly(marked(np, emb_mod, keys[ki], 24_000, (0.0, 1e-3)[s % 2], 8000 + 100 * j + s).astype(np.float64), fs // g, 48_000 // g).astype(dt)
            if settled(keys[ki], clip, fs, lambda t: t["tries"].shape[0] >= 20):
                cases[f"h{fs}"] = (clip, fs, ki)
                say(f"case h{fs}: {clip.size} samples {clip.dtype}, seed {s}")
                break
        assert f"h{fs}" in cases
    # (i) a marked frame at sample 0, cut at the lengths where the template and the frame begin to fit
    for s in range(16):
        frame = marked(np, emb_mod, keys[3], 1216, 0.0, 9000 + s)
        if all(settled(keys[3], frame[:n], 48_000, lambda t: True) for n in (62, 63, 1214, 1215, 1216)):
            break
    else:
        raise AssertionError("case i: no settled seed")
    for n in (62, 63, 1214, 1215, 1216):
        cases[f"i{n}"] = (frame[:n].copy(), 48_000, 3)

    out = {"cases": np.array(sorted(cases)), "strangers": np.stack([np.frombuffer(k, np.uint8) for k in strangers]),
           "keys": np.stack([np.frombuffer(k, np.uint8) for k in keys])}
    # own-key runs decode for real (about 0.3 s per try): one process per case, the traces do not depend on who ran them
    _JOB.update(np=np, det=det_mod, utils=utils_mod, keys=keys, cases=cases)
    order = sorted(cases, key=lambda n: -cases[n][0].size)
    with ProcessPoolExecutor(max_workers=min(6, os.cpu_count() or 1), mp_context=multiprocessing.get_context("fork")) as pool:
        own = dict(zip(order, pool.map(_own_run, order)))
    cost = {}
    for name in sorted(cases):
        clip, fs, ki = cases[name]
        out[f"{name}/clip"], out[f"{name}/fs_in"], out[f"{name}/key"] = clip, np.array(fs), np.array(ki)
        runs = {"own": own[name][0], "s0": trace(strangers[0], clip, fs), "s1": trace(strangers[1], clip, fs)}
        cost[name] = runs["own"]["tries"].shape[0]
        say(f"{name}: {cost[name]} own-key tries decoded in {own[name][1]:.1f} s; strangers {runs['s0']['tries'].shape[0]}, {runs['s1']['tries'].shape[0]}")
        for tag, t in runs.items():
            for f in FIELDS:
                out[f"{name}/{tag}/{f}"] = t[f]
    # the stub touches no search state: the two own-key cases with the fewest tries above a hundred, captured both ways
    for name in sorted((n for n in cases if cost[n] >= 100), key=lambda n: cost[n])[:2]:
        clip, fs, ki = cases[name]
        t = trace(keys[ki], clip, fs)
        assert all(np.array_equal(t[f], out[f"{name}/own/{f}"], equal_nan=f == "thr") for f in FIELDS), name
        say(f"{name}: stubbed trace == decoded trace")
    # every case reaches its branch (asserted again by tests/test_golden_search.py), and the own keys start on all four bands
    for name in "abcdef":
        if name in cases:
            t = {f: out[f"{name}/own/{f}"] for f in FIELDS}
            assert name in reaches(np, t, cases[name][0].size) and (name != "f" or "gated" in reaches(np, t, cases[name][0].size)), name
    assert {int(out[f"{n}/own/bands"][0]) for n in cases if out[f"{n}/own/bands"].size} == {b[0] for b in utils_mod.BAND_PLAN}
    np.savez_compressed(OUT, **out)
    say(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(cases)} cases, {sum(cost.values())} own-key tries")


if __name__ == "__main__":
    main()
