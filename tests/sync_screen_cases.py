"""Host-only builders of the sync picker's worst cases (numpy + the CPU oracle; no GPU, no torch).

The default sync path settles thresholds and peaks from a float32 screen of the correlation row and promises the float64 result for
ANY screen within DELTA = 3e-5 of the exact row (es_sync32.hip, sync_pick_row).  Two things are built here:

  build_rows(T, band)   float64 records y [R, T], handed to the kernels as they are (no band-pass in front), with near-ties planted
                        where the picker decides: at the median, at the MAD, at the threshold, among the rivals of a peak, in the
                        top-five band, and at the capacities (192 exact values, 64 rivals) on either side.
  screens(...)          for one exact row, the float32 screens float32(corr + e), |e| <= a, that are worst for each decision.

A "zone" is a geometric run y[at : at+Z+62] = amp * r**(Z+61-k): all Z windows inside it are scaled copies of one another, so their
normalised correlations are equal up to rounding, at c0(r) = sum r**(62-k) tpl[k] / sqrt(sum r**(2(62-k))).  (Only "up to": the
reference's denominator is sqrt(energy) + 1e-12, so windows whose samples are below ~1e3 sit a relative 1e-15 .. 1e-12 lower.)

cases(T) joins the rows of all four bands with the oracle's answer for each; tests/test_sync_screen_cases.py asserts from the
oracle alone that every row has the property it was built for, tests/test_gpu_sync_screen.py runs them through the kernels.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from echoseal_amd.tables import pack_tables
from oracle import oracle as O

DELTA = 3e-5                 # the bound the picker claims to tolerate
A = 2.9e-5                   # |e| of the built screens: DELTA less the float32 rounding of the sum, with room
NMS = 607                    # non-maximum suppression half window (ES_FRAME_LEN / 2)
L = 63
SWEEP = (186, 187, 188, 189, 190, 191, 192, 193, 194)
SEED = 3
F32_SAFE = 1e15              # rows whose samples stay below this go through the float32 kernels too

_BA, _TPL, _, _, _ = pack_tables()


def _rng(family: str, T: int, band: int, extra: int = 0):
    return np.random.default_rng([SEED, zlib.crc32(family.encode()), T, band, extra])


def zone_start(T: int) -> int:
    return 700 if T >= 2048 else 450


def white(family, T, band, extra=0):
    return _rng(family, T, band, extra).normal(0.0, 1.0, T)


def bandpassed(family, T, band, extra=0):
    x = _rng(family, T, band, extra).normal(0.0, 0.3, T).astype(np.float32)
    return O.lfilter(_BA[band, :9], _BA[band, 9:], x)


def put_zone(y, at, Z, r, amp):
    k = np.arange(Z + 62, dtype=np.float64)
    v = r ** (-k)
    y[at:at + Z + 62] = amp * v / v.max()
    return y


def c0(r, band):
    w = r ** (62.0 - np.arange(L))
    return float((w * _TPL[band]).sum() / np.sqrt((w * w).sum()))


def exact(y, band):
    """The oracle's answer for one record: dict(corr, thr, med, mad, peaks, total, fallback)."""
    corr = O.ncc(y, _TPL[band])
    thr, med, mad = O.cfar_threshold(corr)
    peaks, tot, fb = O.pick_peaks(corr, thr)
    return dict(corr=corr, thr=thr, med=med, mad=mad, peaks=peaks, total=tot, fallback=fb)


def _bisect(f, lo, hi, iters=200):
    """f(lo) < 0 <= f(hi): halve until lo and hi are adjacent doubles (or `iters` halvings); -> (lo, hi, halvings)."""
    assert f(lo) < 0 <= f(hi), (f(lo), f(hi))
    n = 0
    while n < iters:
        mid = 0.5 * (lo + hi)
        if not (lo < mid < hi):
            break
        if f(mid) < 0:
            lo = mid
        else:
            hi = mid
        n += 1
    return lo, hi, n


# ------------------------------------------------------------------------------------------------------------ families
def _near_tied_crossers(T, band):
    """c0(0.6) = 0.678 > thr of white noise: Z crossers that are each other's rivals, decided in the last ulps (r = 0.5: exact ties)."""
    rows = []
    for Z in (20, 50, 63, 64, 65, 66, 67, 100):
        y = put_zone(white("crossers", T, band), zone_start(T), Z, 0.6, 1e14)
        rows.append((y, dict(family="crossers", name=f"crossers r0.6 Z{Z}", Z=Z, r=0.6)))
    for Z, amp in ((50, 1e20), (100, 1e30)):
        y = put_zone(white("crossers", T, band), zone_start(T), Z, 0.5, amp)
        rows.append((y, dict(family="crossers", name=f"crossers r0.5 Z{Z} amp{amp:g}", Z=Z, r=0.5)))
    return rows


def _near_tied_fallback(T, band):
    """c0(0.8) = 0.527 < thr: no crosser, the fallback takes five of Z near-equal values."""
    rows = []
    for Z in (100,) + SWEEP + (250,):
        # (Z = 100 over noise of 1e8: over noise of 1 the run's first samples, 1e20 * 0.8**161 = 2.5e4, tower over the noise in
        #  front of them, and the windows that straddle the zone's start would cross the threshold instead of leaving a fallback)
        y = put_zone((1e8 if Z == 100 else 1.0) * white("fallback", T, band), zone_start(T), Z, 0.8, 1e20)
        rows.append((y, dict(family="fallback", name=f"fallback Z{Z} amp1e20", Z=Z, r=0.8)))
    for Z in (100, 192, 193, 250):
        y = put_zone(white("fallback", T, band), zone_start(T), Z, 0.8, 1e12)
        rows.append((y, dict(family="fallback", name=f"fallback Z{Z} amp1e12", Z=Z, r=0.8)))
    return rows


def _mad_lock_row(T, band, Z, frac):
    """A zone whose plateau |c0(r) - med| holds the middle rank of the absolute deviations, `frac` of the way through the plateau:
    the MAD is then one of Z near-equal values.  r is bisected around 1 (c0 falls from 0.16 at 0.98 to 0.04 at 1.02, the MAD of a
    white row's correlations is 0.085), since a fixed ratio locks only for some T and Z."""
    base = white("madlock", T, band)
    at = zone_start(T)

    def build(r):
        return put_zone(base.copy(), at, Z, r, 10.0)

    def g(r):                                         # >= 0: the middle rank lies at least `frac` of the way through the plateau
        corr = O.ncc(build(r), _TPL[band])
        med = float(np.median(corr))
        dev = np.abs(corr - med)
        p = dev[at + Z // 2]
        return (dev.size - 1) / 2.0 - (np.count_nonzero(dev < p - 1e-9) + frac * Z)

    _, r, _ = _bisect(g, 0.98, 1.02, iters=40)        # c0, and with it the plateau's rank, falls as r grows
    return build(r), r


def _mad_lock(T, band):
    rows = []
    for Z in (150,) + SWEEP + (250,):
        y, r = _mad_lock_row(T, band, Z, 0.5)
        rows.append((y, dict(family="madlock", name=f"madlock Z{Z}", Z=Z, r=r)))
    for Z in (150, 250):
        for frac in (0.2, 0.8):
            y, r = _mad_lock_row(T, band, Z, frac)
            rows.append((y, dict(family="madlock", name=f"madlock Z{Z} frac{frac}", Z=Z, r=r)))
    return rows


def _median_lock(T, band, sweep):
    """A zero zone: Z correlations are exactly 0 and hold the median.  The windows that overlap the zone by a few samples, where
    the template's first and last taps are nearly zero, add a band-dependent handful of values within 2 DELTA of it; the sweep
    is shifted by that count so that the median's band, not Z, walks over 186 .. 194."""
    def row(Z):
        y = white("medlock", T, band)
        y[zone_start(T):zone_start(T) + Z + 62] = 0.0
        return y

    e = exact(row(150), band)
    extra = near_count(e["corr"], e["med"]) - 150
    Zs = (150,) + (tuple(s - extra for s in SWEEP) if sweep else ()) + (250,)
    return [(row(Z), dict(family="medlock", name=f"medlock Z{Z}", Z=Z, sweep=Z not in (150, 250))) for Z in Zs]


def _exact_repeats(T, band, periods):
    rows = []
    for p in periods:
        pat = _rng("repeats", T, band, p).normal(0.0, 1.0, p)
        rows.append((np.tile(pat, T // p + 1)[:T].copy(), dict(family="repeats", name=f"repeats period {p}", period=p)))
    return rows


def unsaturated_thr(y, band):
    corr = O.ncc(y, _TPL[band])
    _, med, mad = O.cfar_threshold(corr)
    return med + 4.5 * 1.4826 * mad


def _saturation_edge(T, band, targets):
    """w * (band-passed noise) + (1 - w) * (white noise at the band-passed level), w bisected so that med + 6.6717 MAD lands on each target around 0.95."""
    rows = []
    for i, t in enumerate(targets):
        bp, wh = bandpassed("satedge", T, band, i), 0.1 * white("satedge", T, band, 100 + i)
        mix = lambda w: w * bp + (1.0 - w) * wh       # noqa: E731
        _, w, _ = _bisect(lambda w: unsaturated_thr(mix(w), band) - t, 0.0, 1.0, iters=30)
        rows.append((mix(w), dict(family="satedge", name=f"satedge target {t:.4f}", target=float(t))))
    return rows


def _plant(y, p, a, band):
    y = y.copy()
    y[p:p + L] += a * _TPL[band]
    return y


def _crosser_at_threshold(T, band, kinds=("white", "bandpassed")):
    """A template planted at lag p, its amplitude bisected to the two adjacent doubles between which (largest correlation within
    31 lags of p) - thr changes sign -- the largest, since a narrow band's template nearly repeats every few lags and noise can
    hand the maximum to a neighbour of p; and two templates 300 lags apart (inside one suppression window), the second bisected
    until the two peaks swap order."""
    rows = []
    p = zone_start(T) - 200
    for kind in kinds:
        base = white("crosser", T, band) if kind == "white" else bandpassed("crosser", T, band)
        top = 100.0 * float(np.abs(base).max())

        def f(a):
            e = exact(_plant(base, p, a, band), band)
            return e["corr"][p - 31:p + 32].max() - e["thr"]

        lo, hi, n = _bisect(f, 0.0, top)
        for side, a in (("below", lo), ("at", hi)):
            rows.append((_plant(base, p, a, band), dict(family="crosser", name=f"crosser {kind} {side}", lag=p, halvings=n, side=side, kind=kind)))
        q = p + 300
        strong = _plant(base, p, 3.0 * hi, band)

        def g(a):
            c = O.ncc(_plant(strong, q, a, band), _TPL[band])
            return c[q - 31:q + 32].max() - c[p - 31:p + 32].max()

        lo2, hi2, n2 = _bisect(g, 0.0, top)
        for side, a in (("first", lo2), ("second", hi2)):
            rows.append((_plant(strong, q, a, band), dict(family="swap", name=f"swap {kind} {side}", lag=p, lag2=q, halvings=n2, side=side, kind=kind)))
    return rows


def _ordinary(T, band, count):
    rows = []
    for i in range(count):
        rows.append((bandpassed("ordinary", T, band, i), dict(family="ordinary", name=f"ordinary noise {i}")))
    for i in range(count):
        y = bandpassed("ordinary", T, band, 50 + i)
        p = 100 + (97 * i) % (T - 62 - 200)
        a = 6.0 * float(np.sqrt((y[p:p + L] ** 2).sum()))
        rows.append((_plant(y, p, a, band), dict(family="ordinary", name=f"ordinary planted {i}", lag=p)))
    return rows


# Rows that once showed a mismatch, kept by name after the fix: (name, T, band, builder(T, band) -> y).  None: no built row has.
REGRESSIONS: tuple = ()


def build_rows(T: int, band: int):
    """-> (y float64 [R, T], info: one dict per row with 'family', 'name' and the family's parameters).  Band 0 carries every
    family; the families that need c0 above the noise (near-tied crossers and fallback, MAD lock) exist only there: the other
    bands' c0 is negative or below 0.05."""
    if band == 0:
        rows = (_near_tied_crossers(T, 0) + _near_tied_fallback(T, 0) + _mad_lock(T, 0) + _median_lock(T, 0, True)
                + _exact_repeats(T, 0, (38, 40)) + _saturation_edge(T, 0, np.linspace(0.93, 0.97, 16)) + _crosser_at_threshold(T, 0)
                + _ordinary(T, 0, 8))
    else:
        rows = (_median_lock(T, band, False) + _exact_repeats(T, band, (38,)) + _saturation_edge(T, band, (0.94, 0.96))
                + _crosser_at_threshold(T, band, ("bandpassed",)) + _ordinary(T, band, 1))
    rows += [(b(T, band), dict(family="regression", name=name)) for name, t, bd, b in REGRESSIONS if (t, bd) == (T, band)]
    y = np.stack([r[0] for r in rows])
    info = [dict(r[1], band=band, f32_safe=bool(np.abs(r[0]).max() <= F32_SAFE)) for r in rows]
    return y, info


class Cases:
    """All bands' rows of one T with the oracle's answers: y [R, T], band [R], info [R], ref [R] (see exact())."""

    def __init__(self, T):
        ys, self.info = [], []
        for band in range(4):
            y, info = build_rows(T, band)
            ys.append(y); self.info += info
        self.T = T
        self.y = np.concatenate(ys)
        self.y.setflags(write=False)
        self.band = np.array([i["band"] for i in self.info], np.uint8)
        self.ref = [exact(self.y[i], int(self.band[i])) for i in range(len(self.info))]
        self.thr = np.array([r["thr"] for r in self.ref])
        self.npeaks = np.array([r["total"] | (int(r["fallback"]) << 30) for r in self.ref], np.int32)
        self.peaks = np.full((len(self.ref), 32), -1, np.int32)
        for i, r in enumerate(self.ref):
            self.peaks[i, :len(r["peaks"])] = r["peaks"]

    def rows(self, family, **match):
        return [i for i, d in enumerate(self.info) if d["family"] == family and all(d.get(k) == v for k, v in match.items())]


@functools.lru_cache(maxsize=None)
def cases(T: int) -> Cases:
    return Cases(T)


# ------------------------------------------------------------------------------------------------------------ screens
PATTERNS = ("zero", "plus", "minus", "random sign", "uniform", "toward median", "away from median", "crossers down", "crossers up",
            "peaks down", "top five down", "bin edge")


def screens(corr, thr, med, peaks, a=A, seed=0):
    """-> {pattern: float32 screen row}, each within DELTA of `corr` after rounding (asserted: it is the picker's contract).
    `peaks`: the oracle's peak lags (or its top-five lags when the fallback ran)."""
    n = corr.size
    rng = np.random.default_rng([SEED, seed, n])
    order = np.argsort(corr, kind="stable")
    near = np.zeros(n, bool)
    for p in peaks:
        near[max(0, int(p) - NMS):int(p) + NMS + 1] = True
    pk = np.zeros(n, bool); pk[np.asarray(peaks, int)] = True
    top5 = np.zeros(n, bool); top5[order[-5:]] = True
    edge = np.round(corr * 128.0) / 128.0                                # the nearer 1/128 histogram bin edge ...
    to_edge = np.where(edge > corr, a, -a)                               # ... and past it where a reaches (everywhere: a full step)
    e = {
        "zero": np.zeros(n),
        "plus": np.full(n, a),
        "minus": np.full(n, -a),
        "random sign": a * rng.choice([-1.0, 1.0], n),
        "uniform": rng.uniform(-a, a, n),
        "toward median": -a * np.sign(corr - med),
        "away from median": a * np.sign(corr - med),
        "crossers down": np.where(corr >= thr, -a, a),
        "crossers up": np.where(corr >= thr, a, -a),
        "peaks down": np.where(pk, -a, np.where(near, a, 0.0)),
        "top five down": np.where(top5, -a, a),
        "bin edge": to_edge,
    }
    out = {}
    for name in PATTERNS:
        s = (corr + e[name]).astype(np.float32)
        assert np.abs(s.astype(np.float64) - corr).max() <= DELTA, name
        out[name] = s
    return out


def near_count(values, centre, width=2 * DELTA):
    return int(np.count_nonzero(np.abs(values - centre) <= width))
