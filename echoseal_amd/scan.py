"""The scan front end of WatermarkDetector and WatermarkIdentifier: from a list of clips with their rates to sync results with the
peaks that can hold a frame.  Host code only: the clips of a call are cut into launches (cut_launches), a launch's samples reach the
device in one place (Launch.rows) and one sync call finds its peaks (sync_launch).  Nothing here is keyed: header decodes and everything
after them belong to the callers, who share the host statement of the reference's try order (plan_tries) and the widths of the hop
tables it reads.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as nat
from .utils import resample_limits, resampled_length

PRE_L = nat.ES_PRE_L              # 63 chips of the sync template (utils.mseq_63)
FRAME_LEN = nat.ES_FRAME_LEN      # 1215 = PRE_L + 128 header chips + 1024 code bits
PEAK_LIMIT = nat.ES_PEAK_LIMIT    # 25, rtwm/detector.py:108

MAX_TRIES = nat.ES_MAX_TRIES      # 400, rtwm/detector.py:107
TIGHT_DELTA = 3          # rtwm/detector.py:131: the counter window around a peak's estimate when its header failed ...
WIDE_DELTA = 200         # rtwm/detector.py:118: ... and the widest one
CTR_END = 1 << 32        # frame counters are 32-bit words: the header carries their low 16 bits, the payload all of them


def counter_estimate(start: int, pos0: int = 0, ctr0: int = 0) -> int:
    """The counter of the frame a peak lies on: the peak at `start` of a window whose first sample is absolute sample pos0
    of a stream marked from counter ctr0 -> ctr0 + round((pos0 + start) / 1215), in integers (1215 is odd: no ties).  At pos0 = ctr0 = 0
    it is rtwm/detector.py:117, round(start / 1215)."""
    return int(ctr0) + (2 * (int(pos0) + int(start)) + FRAME_LEN) // (2 * FRAME_LEN)


def plan_tries(starts, hdr_ok, hdr_lo16, hops, pos0: int = 0, ctr0: int = 0):
    """The reference's try order for one band row (rtwm/detector.py:105-142), stated once on the host.  starts: the row's peaks that can
    hold a frame, in peak order; hdr_ok / hdr_lo16: their header results; hops(c): counter c hops to the row's band; pos0 / ctr0: as
    for counter_estimate.  Counters stay inside [0, 2^32); MAX_TRIES tries end the row, between peaks or inside one.
    -> ([(peak index, its counters)] in try order, peaks looked at)."""
    tries, left = [], MAX_TRIES
    for j, start in enumerate(starts):
        if left <= 0:
            break
        est = counter_estimate(start, pos0, ctr0)
        wide = range(max(0, est - WIDE_DELTA), min(est + WIDE_DELTA + 1, CTR_END))      # counters end at 2^32 - 1
        if hdr_ok[j]:                                                       # rtwm/detector.py:122-127
            lo16 = int(hdr_lo16[j])
            cands = [c for c in wide if (c & 0xFFFF) == lo16 and hops(c)]
        else:                                                               # :131-140
            cands = [c for c in range(max(0, est - TIGHT_DELTA), min(est + TIGHT_DELTA + 1, CTR_END)) if hops(c)]
            if not cands:
                cands = [c for c in wide if hops(c)]
        tries.append((j, cands[:left]))
        left -= len(cands)
    return tries, len(tries)


def hop_width(samples: int) -> int:         # counters from 0 that the tries of a record of `samples` samples reach: the hop table of es_plan_batch
    return -(-int(samples) // FRAME_LEN) + WIDE_DELTA + 1


def hop_at_width(samples: int) -> int:      # the same from 200 below any window base's estimate: what es_plan_at_batch asks of a hop row
    return -(-int(samples) // FRAME_LEN) + 2 * WIDE_DELTA + 2


def rate_list(fs_in, n: int) -> list:        # `fs_in` of a batch call, one rate or one per clip, as a list of n
    return list(fs_in) if isinstance(fs_in, (list, tuple)) else [fs_in] * n


def counter_origins(ctr0, n: int, what: str = "clip") -> list:
    """`ctr0` (None; one origin; or one per clip / stream, entries may be None) as a list of n entries, each None or an int in [0, 2^32).
    A ValueError names what is refused: a negative origin, one of 2^32 or more, one that is not an integer, a wrong count."""
    n = int(n)
    if ctr0 is None or isinstance(ctr0, (int, np.integer)) or np.ndim(ctr0) == 0:
        vals = [ctr0] * n
    else:
        vals = list(ctr0)
        if len(vals) != n:
            raise ValueError(f"ctr0 names {len(vals)} counter origins for {n} {what}s: give one origin, or one per {what}")
    out = []
    for v in vals:
        if v is not None:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"ctr0 = {v!r}: a counter origin is an integer in [0, 2^32) (or None: counters relative to the {what})")
            v = int(v)
            if not 0 <= v < CTR_END:
                raise ValueError(f"ctr0 = {v}: a counter origin is an integer in [0, 2^32) (counters that wrap are out of scope)")
        out.append(v)
    return out


def check_counter_reach(origin, samples: int, what: str = "clip") -> None:
    """Refuse an origin from which `samples` samples reach the end of the counter range: origin + ceil(samples / 1215) + 201 must not
    pass 2^32 - 1 (the widest candidate window of the last frame stays inside the counters that exist)."""
    if origin is not None and int(origin) + hop_width(samples) > CTR_END - 1:
        raise ValueError(f"ctr0 = {int(origin)}: a {what} of {int(samples)} samples would reach counter ctr0 + ceil(samples / 1215) + 201 > 2^32 - 1 "
                         "(counters that wrap past 2^32 are out of scope)")


# Padded samples (sync rows x longest clip) of one launch over clips of unequal length.  A memory bound, not a tuned value: a padded row
# sample costs 20 bytes on the device (float32 in, float64 y, float64 corr), so 2^26 of them are 1.3 GB.
RAGGED_ROW_SAMPLES = 1 << 26

_DEVICE_SAMPLE_TYPES = (np.dtype(np.float32), np.dtype(np.float64), np.dtype(np.int16))      # what es_resample_ragged_batch reads


def ragged_buckets(lengths, rows_per_clip: int, budget: int) -> list[list[int]]:
    """Cut clips into launches: indices sorted by length (equal lengths in input order, hence adjacent), then taken greedily while
    rows x longest clip = len(bucket) * rows_per_clip * max(length) <= budget.  A clip that is over the budget on its own still gets a
    bucket, alone.  -> buckets of indices, lengths ascending within each and from bucket to bucket."""
    order = sorted(range(len(lengths)), key=lambda i: (int(lengths[i]), i))
    out: list[list[int]] = []
    cur: list[int] = []
    for i in order:
        if cur and (len(cur) + 1) * rows_per_clip * int(lengths[i]) > budget:      # lengths ascend: clip i would be the longest
            out.append(cur); cur = []
        cur.append(i)
    if cur:
        out.append(cur)
    return out


def dev(eng, arr: np.ndarray, dtype):
    """A host array on the engine's device, contiguous and of `dtype`: the one upload helper of the receive side."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=dtype)).to(eng.device)


@dataclass
class Launch:
    """The clips of one sync launch, all of one sample type.  rates None: host signals already at fs_target (int16 or float32);
    otherwise raw samples as they came, clip c at rates[c]."""
    idx: list            # positions of the clips in the call
    sizes: list          # length of each clip at fs_target
    clips: list          # 1-D host arrays
    rates: list | None
    fs_target: int

    def part(self, a: int, b: int) -> "Launch":
        return Launch(self.idx[a:b], self.sizes[a:b], self.clips[a:b], None if self.rates is None else self.rates[a:b], self.fs_target)

    def rows(self, eng, nb: int):
        """-> (device rows [clips * nb, >= longest clip], row = clip * nb + band, clip c in the first sizes[c] samples of its rows;
        sizes).  The one place that decides how samples reach the device."""
        if self.rates is not None:
            # conditioned on the device: ONE es_resample_ragged_batch launch writes the padded rows, no sample makes a round trip
            rows, lens = eng.resample_ragged(self.clips, self.rates, self.fs_target, rep=nb)
            return rows, [int(n) for n in lens]
        M = max(self.sizes)
        if min(self.sizes) == M:
            host = np.stack(self.clips)
        else:                                                               # unequal lengths: rows padded to the longest clip
            host = np.zeros((len(self.clips), M), self.clips[0].dtype)
            for c, sg in enumerate(self.clips):
                host[c, :sg.size] = sg
        return dev(eng, np.repeat(host, nb, axis=0), host.dtype), self.sizes


def cut_launches(clips, fs_list, fs_target: int, nb: int, condition, budget: int = RAGGED_ROW_SAMPLES) -> list[Launch]:
    """Which clips share a sync launch: by sample type, then ragged_buckets over the lengths at fs_target (nb sync rows per clip).
    Clips shorter than the template (rtwm/detector.py:71-73) are in none.  A call whose 1-D non-empty clips are all at fs_target takes
    the host path: signals as float32 or int16 (what the band-pass kernels read), launches float32 then int16.  A call with any such
    clip at another rate takes the device path: int16 / float32 / float64 clips stay raw, bucketed by their resampled
    lengths, launches float32, float64, int16; 2-D, empty and oddly typed clips, and a clip whose rate pair is outside what the
    ragged kernel takes (utils.resample_limits: it would write nothing for it), enter as host signals at fs_target.
    condition(clip, rate) -> the clip at fs_target, on the host; asked only where rate != fs_target.  The budget holds for clips of
    one length too: an over-budget group of equally long clips is several launches, each on the equal-length sync path."""
    mixed = any(f != fs_target and np.ndim(c) == 1 and np.size(c) for c, f in zip(clips, fs_list))
    arrs, rates = [], []
    for c, f in zip(clips, fs_list):
        a = np.asarray(c)
        if not (mixed and a.ndim == 1 and a.size and a.dtype in _DEVICE_SAMPLE_TYPES and resample_limits(a.size, f, fs_target) is None):
            a = (np.asarray(condition(a, f)) if f != fs_target else a).reshape(-1)
            a, f = (a if a.dtype == np.int16 else a.astype(np.float32, copy=False)), fs_target
        arrs.append(a); rates.append(int(f))
    sizes = [resampled_length(a.size, f, fs_target) for a, f in zip(arrs, rates)]
    out: list[Launch] = []
    for dt in _DEVICE_SAMPLE_TYPES:                                         # (host path: no float64 signal is left)
        idx = [i for i, a in enumerate(arrs) if a.dtype == dt and sizes[i] >= PRE_L]
        for b in ragged_buckets([sizes[i] for i in idx], nb, budget):
            ids = [idx[k] for k in b]
            out.append(Launch(ids, [sizes[i] for i in ids], [arrs[i] for i in ids], [rates[i] for i in ids] if mixed else None, fs_target))
    return out


@dataclass
class SyncScan:
    """One launch after sync.  Peak j that can hold a frame = sy.y[rows[j], starts[j] : starts[j] + 1215], in (row, peak) order."""
    sy: object           # the SyncResult as the kernels wrote it
    sizes: list          # samples of each clip
    nb: int              # sync rows per clip
    rows: np.ndarray     # int64 clip * nb + band
    starts: np.ndarray   # int64, relative to the clip's first sample
    yrows: np.ndarray | None = None      # where the frames lie when not at sy.y[rows, starts] (a monitor tick: history rows ...
    cols: np.ndarray | None = None       # ... and columns, start + the window's offset)

    @property
    def frame_rows(self) -> np.ndarray:
        return self.rows if self.yrows is None else self.yrows

    @property
    def frame_cols(self) -> np.ndarray:
        return self.starts if self.cols is None else self.cols

    @classmethod
    def from_monitor(cls, tick) -> "SyncScan":
        """The scan of one monitor tick (engine.MonitorTick): every pushed stream is a clip, its window [w0, n) the clip's samples.
        Peaks and starts are window-relative, as for a clip cut at w0; the frames are read in place at history column offset + start."""
        rows, starts = fitting_peaks(tick.peaks, tick.npeaks, tick.length)
        return cls(tick, [int(n) for n in tick.length[::tick.nb]], tick.nb, rows, starts, tick.rows[rows], tick.offset[rows] + starts)


def fitting_peaks(peaks, npeaks, row_sizes):
    """The peaks of a sync result that can hold a frame, in (row, peak) order: of the first PEAK_LIMIT peaks of each row those with
    start + 1215 <= the row's samples (rtwm/detector.py:108, 112-113) -> (rows int64, starts int64)."""
    npk = (npeaks.cpu().numpy() & 0xFFFF)
    pk = peaks.cpu().numpy()
    rows, starts = [], []
    for r in range(pk.shape[0]):
        for st in pk[r, :min(int(npk[r]), pk.shape[1], PEAK_LIMIT)]:
            if st + FRAME_LEN <= row_sizes[r]:
                rows.append(r); starts.append(int(st))
    return np.array(rows, np.int64), np.array(starts, np.int64)


def sync_launch(eng, launch: Launch, band_ids) -> SyncScan:
    """Band-pass, correlate and pick peaks for every (clip, band) of a launch in one sync call: row = clip * len(band_ids) + band."""
    import torch
    nb = len(band_ids)
    x, sizes = launch.rows(eng, nb)
    bid = dev(eng, np.tile(np.asarray(band_ids, np.uint8), len(sizes)), np.uint8)
    M = max(sizes)
    if min(sizes) < M:
        sy = eng.sync_ragged(x, torch.from_numpy(np.repeat(np.array(sizes, np.int32), nb)), bid, keep_corr=False)
    else:
        x = x[:, :M]                                                        # (device rows: made contiguous there where the stride is longer)
        sy = eng.sync_fast(x, bid) if M - (PRE_L - 1) <= eng.FAST_MAX_LAGS else eng.sync(x, bid, keep_corr=False)
    rows, starts = fitting_peaks(sy.peaks, sy.npeaks, np.repeat(np.asarray(sizes, np.int64), nb))      # against each clip's own length
    return SyncScan(sy, sizes, nb, rows, starts)
