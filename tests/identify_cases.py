"""Randomised scans for the candidate planner (helper of the identify tests, CPU and GPU): sync rows with 0..32 peaks, starts up to
and past M - 1215, header results that hit and miss, and hop schedules that make every branch of the reference's rules
(rtwm/detector.py:105-142) run: the +-3 window, the wide fallback when the hop never selects the band inside +-3, header-gated
windows, and lists that reach MAX_TRIES in the middle of a peak."""
import numpy as np

from echoseal_amd.detector import FRAME_LEN, WatermarkDetector, _Scan
from echoseal_amd.utils import BAND_PLAN

MAX_PEAKS = 32


class Scan:
    """One sync row and one key's view of it."""
    __slots__ = ("M", "band", "peaks", "npeaks", "fit", "hdr_ok", "hdr_lo16", "hop", "kind")


def hop_width(M):
    return -(-M // FRAME_LEN) + 201


def random_scan(rng, kind=None, M=None):
    s = Scan()
    s.kind = kind if kind is not None else rng.choice(["mixed", "dense", "sparse", "all", "gap"])
    s.M = int(rng.choice([1215, 1300, 12_000, 48_000, 240_000, 3_000_000])) if M is None else int(M)
    s.band = int(rng.integers(0, 4))
    n = int(rng.choice([0, 1, 2, 7, 24, 25, 26, 31, 32]))
    hi = s.M - FRAME_LEN
    starts = np.sort(rng.integers(0, max(1, s.M - 62), n))
    if n and rng.random() < 0.5:                                   # starts at and just past the last one that can hold a frame
        edge = np.array([hi - 1, hi, hi + 1, hi + 2][:n])
        starts[-len(edge):] = np.clip(edge, 0, None)
        starts = np.sort(starts)
    s.peaks = np.full(MAX_PEAKS, -1, np.int32)
    s.peaks[:n] = starts
    s.npeaks = np.int32(n | (int(rng.random() < 0.3) << 30))       # bit 30: the sync kernels' fallback flag, not part of the count
    look = s.peaks[:min(n, 25)]
    s.fit = look[(look >= 0) & (look + FRAME_LEN <= s.M)]
    C = hop_width(s.M)
    p = {"mixed": 0.25, "dense": 0.9, "sparse": 0.02, "all": 1.0, "gap": 0.25}[s.kind]
    other = (s.band + 1 + rng.integers(0, 3, C)) % 4
    s.hop = np.where(rng.random(C) < p, s.band, other).astype(np.uint8)
    est = (2 * s.fit.astype(np.int64) + FRAME_LEN) // (2 * FRAME_LEN)
    if s.kind == "gap":                                            # the hop never selects the band inside +-3 of any estimate
        for e in est:
            lo = max(0, int(e) - 3)
            s.hop[lo:int(e) + 4] = other[lo:int(e) + 4]
    s.hdr_ok = (rng.random(s.fit.size) < 0.4).astype(np.uint8)
    s.hdr_lo16 = rng.integers(0, 65536, s.fit.size).astype(np.int32)
    for j in np.flatnonzero(rng.random(s.fit.size) < 0.6):         # lo16 of a counter inside the window (a hit if the hop agrees)
        c = int(est[j]) + int(rng.integers(-200, 201))
        if c >= 0:
            s.hdr_lo16[j] = c & 0xFFFF
            if rng.random() < 0.7:
                s.hop[c] = s.band
    return s


class _Hop:
    def __init__(self, hop):
        self._hop = hop

    def band(self, ctr):
        return BAND_PLAN[int(self._hop[ctr])]


def detector_plan(s):
    """WatermarkDetector._scan_plan on the scan -> ([(start, ctr, header-log index)], len(header log))."""
    det = WatermarkDetector(bytes(32), list_size=1)
    det._hop = _Hop(s.hop)
    nf = s.fit.size
    scan = _Scan(bands=[BAND_PLAN[s.band]], src=None, sel=np.arange(nf), rows=np.zeros(nf, np.int64), starts=s.fit.astype(np.int64),
                 hdr=(s.hdr_ok.astype(bool), s.hdr_lo16.astype(np.int64), np.zeros(nf)))
    plan, hdr_log = det._scan_plan(scan, 0)
    return [(start, ctr, h) for (_j, start, ctr, h) in plan], len(hdr_log)


def reference_plan(s):
    """identify.plan_reference on the scan, in detector_plan's terms."""
    from echoseal_amd.identify import plan_reference
    plan, looked = plan_reference(s.peaks, s.npeaks, s.M, s.band, s.hdr_ok, s.hdr_lo16, s.hop)
    fit_rank = np.cumsum((s.peaks >= 0) & (s.peaks + FRAME_LEN <= s.M)) - 1
    return [(int(s.peaks[slot]), ctr, int(fit_rank[slot])) for slot, ctr in plan], looked, plan


def plan_inputs(rng, M, rows, N):
    """Inputs of one es_plan_batch call: `rows` random sync rows of M samples seen by N keys
    -> (peaks, npeaks, rowband, hdr_base, hdr_ok [N, P], hdr_lo16 [N, P], hop [N, C])."""
    scans = [random_scan(rng, M=M) for _ in range(rows)]
    peaks = np.stack([s.peaks for s in scans]); npeaks = np.array([s.npeaks for s in scans], np.int32)
    rowband = np.array([s.band for s in scans], np.uint8)
    nfit = np.array([s.fit.size for s in scans])
    base = (np.cumsum(nfit) - nfit).astype(np.int32)
    P, C = int(nfit.sum()), hop_width(M)
    dens = rng.choice([0.25, 0.9, 0.02, 1.0], N)
    hop = (rng.random((N, C)) >= dens[:, None]).astype(np.uint8) * rng.integers(1, 4, (N, C), dtype=np.uint8)    # band 0 with density dens[k]
    hop = ((hop + rowband[0]) % 4).astype(np.uint8)                            # ... shifted so that every band has a dense key somewhere
    hop[3::5] = scans[1].hop if rows > 1 else hop[3::5]                         # rows' own schedules (the generator's gaps and lo16 hits)
    hok = (rng.random((N, P)) < 0.4).astype(np.uint8)
    hlo = rng.integers(0, 65536, (N, P)).astype(np.int32)
    fit_all = np.concatenate([s.fit for s in scans]) if P else np.zeros(0, np.int64)
    near = ((2 * fit_all.astype(np.int64) + FRAME_LEN) // (2 * FRAME_LEN))[None, :] + rng.integers(-200, 201, (N, P))
    hit = (rng.random((N, P)) < 0.6) & (near >= 0)
    hlo[hit] = (near[hit] & 0xFFFF).astype(np.int32)
    return peaks, npeaks, rowband, base, hok, hlo, hop
