"""WatermarkDetector with the reference's interface (rtwm/detector.py:24-515), MI355X inside.

Host orchestration (band order, counter candidates, AEAD validation, anti-replay nonce) is plain
Python as in the reference; every numeric stage runs on the GPU through echoseal_amd.engine:

    resample_to             -> es_resample_ragged_batch            (rtwm/utils.py:58-66; clips of a batch call at other rates)
                               es_resample_stream_batch            (the same for live streams at other rates, chunk by chunk)
    _scan_band_multi_frame  -> es_bpf / es_xcorr / es_pick        (rtwm/detector.py:59-99)
    _decode_header          -> es_header_batch, es_header_at_batch at the peaks of a scan (rtwm/detector.py:452-515)
    _llr                    -> es_llr_batch, es_llr_at_batch at the peaks of a scan       (rtwm/detector.py:296-416)
    polar decode            -> es_scl_batch + host validator scan (rtwm/fastpolar.py:254-359)

Constructing a detector needs no GPU (keys, static sequences); the first numeric call creates the
engine and raises if the HIP library or the device is missing.  The reference's unconditional
print() debugging is not reproduced.
"""
from __future__ import annotations

import copy
import itertools
from dataclasses import dataclass

import numpy as np

from ._native import NativeError
from .acquire import FULL_SPAN, Acquired, check_max_records, check_span, origin_of, record_order
from .crypto import SecureChannel
from .monitor import LiveTable
from .polar_fast import N_DEFAULT
from .primitives import InvalidTag
from .scan import (CTR_END, FRAME_LEN, MAX_TRIES, PEAK_LIMIT, PRE_L, RAGGED_ROW_SAMPLES, TIGHT_DELTA, WIDE_DELTA, Launch,  # noqa: F401 (re-exported)
                   SyncScan, check_counter_reach, counter_estimate, counter_origins, cut_launches, dev, plan_tries, ragged_buckets, rate_list,
                   sync_launch)
from .tables import matched_filter_taps
from .utils import BAND_PLAN, BandHop, butter_bandpass, choose_band, mseq_63, resample_to, resampled_length  # noqa: F401 (re-exported)

PRE_BITS = mseq_63()
HDR_BITS = 16
HDR_REPEAT = 8
HDR_L = 128
assert PRE_L == len(PRE_BITS) and FRAME_LEN == PRE_L + HDR_L + N_DEFAULT
EPS = 1e-12


def decode_four(eng, y, rows, cols, pn, bands, list_size: int):
    """The four decodes the reference tries per candidate (+llr0, -llr0, +llr1, -llr1; rtwm/detector.py:161-190) for n candidates at
    once, candidate i the frame at y[rows[i], cols[i]:] with PN row pn[i] on band bands[i] (device tensors): two demodulations read in
    place, one list decode -> the SclResult of the 4 n rows, row v * n + i = variant v of candidate i.  Scheduling and selection are the callers'."""
    import torch
    if list_size > eng.list_size_max:
        raise NotImplementedError(f"list_size={list_size}: the HIP decoder supports list sizes up to {eng.list_size_max}")
    l0 = eng.llr(y, bands, pn, variant=0, rows=rows, start=cols)
    l1 = eng.llr(y, bands, pn, variant=1, rows=rows, start=cols)
    return eng.scl(torch.cat((l0, -l0, l1, -l1), dim=0), list_size=list_size, skip_if_hard_ok=False)


def check_decoded(ok: np.ndarray) -> np.ndarray:
    """The host copy of a selection's verdicts, refused where the list decoder skipped a record (-2)."""
    if (ok == -2).any():
        raise NativeError("es_scl_batch: some candidate records were not decoded (no free scratch-slab slot)")
    return ok


@dataclass(eq=False)
class _Frames:
    """Where the frames of a scan lie, without copying them: frame j = y[rows[j], starts[j] : starts[j] + 1215] of the band-passed
    records y (device, float64), read in place by es_header_at_batch / es_llr_at_batch.  rows, starts: host int arrays."""
    y: object
    rows: np.ndarray
    starts: np.ndarray


@dataclass
class _Scan:
    """What _scan_band_multi_frame needs for every band of one clip: the clip's peaks that can hold a frame, in (band, peak) order."""
    bands: list
    src: _Frames | None         # the frames of the clip's whole launch; None: no peak of it can hold a frame
    rows: np.ndarray            # band index (into bands) of each of the clip's peaks
    sel: np.ndarray             # their places in src and hdr
    starts: np.ndarray          # of the whole launch, like src and hdr
    hdr: tuple                  # header decodes under the detector's key: (ok, low 16 counter bits, score)
    ctr0: int | None = None     # counter origin of the clip or stream; None: estimates are relative to the scan, as the reference's
    pos0: int = 0               # absolute sample of the scan's first sample in its stream (a monitor window's w0; 0 for a clip)


@dataclass(eq=False)
class _Front:
    """One launch of the presence calls' front (WatermarkDetector._presence_front): row 4 * clip + band is BAND_PLAN band `band` of a clip."""
    sizes: list                 # samples of each clip at fs_target
    lens: np.ndarray            # int32, the same per row
    bid: object                 # uint8 per row on the device: its band index
    y: object                   # float64 [rows, >= longest clip] on the device: the band-passed rows
    corr: object                # their correlation rows, or None where they were not asked for
    J: np.ndarray | None        # the slots of each clip, where the caller counts them


def clip_origins(ctr0, clips, fs_list, fs_target: int) -> list:
    """The counter origins of a batch call's clips (scan.counter_origins), each checked against its clip's length at fs_target
    (scan.check_counter_reach).  Host arithmetic only."""
    origins = counter_origins(ctr0, len(clips))
    for c, f, o in zip(clips, fs_list, origins):
        if o is not None:
            check_counter_reach(o, resampled_length(int(np.size(c)), int(f), fs_target))
    return origins


class WatermarkDetector:
    """Recover an EchoSeal watermark from a recording (reference docstring: >= 3 s)."""

    def __init__(self, key32: bytes, *, fs_target: int = 48_000, list_size: int = 256, engine=None) -> None:
        self.sec = SecureChannel(key32)
        self.fs_target = fs_target
        self.session_nonce: bytes | None = None
        self._band_key = getattr(self.sec, "band_key", key32)
        self._hop = BandHop(self._band_key)                 # choose_band(self._band_key, .) memoised for the life of this detector
        self._mf_cache: dict = {}
        self._list_size = int(list_size)
        self._aead = getattr(self.sec, "_aead", None)
        self._pre_sy = 2.0 * PRE_BITS.astype(np.float32) - 1.0
        self._hdr_pn_sy = 2.0 * self.sec.pn_bits(0, HDR_L).astype(np.float32) - 1.0
        if self._hdr_pn_sy.size != HDR_L:
            raise RuntimeError(f"Header PN length {self._hdr_pn_sy.size} != expected {HDR_L}")
        self._engine = engine
        self._ring = None                                   # (engine, one-row key ring of this detector's key): acquire
        self._decoy_ring = None                             # (engine, decoys, ring of this key and that many decoy keys): presence
        self._presence_rows: list | None = None             # set to [] to record (clip indices, correlation rows, lags) of every presence launch
        self._trace: list[tuple[int, int, int]] | None = None   # set to [] to record (band_lo, peak, ctr) tries
        self._hdr_trace: list[tuple[float, float, float]] | None = None   # set to [] to record every header decode of a scan

    # ------------------------------------------------------------------ engine plumbing
    @property
    def engine(self):
        from .fastpolar import SMALL_LIST_MAX, check_list_size
        check_list_size(self._list_size)
        large = self._list_size > SMALL_LIST_MAX
        if self._engine is None or self._engine.fs != self.fs_target or (large and self._engine.list_size_max < self._list_size):
            from .fastpolar import engine_for_fs, engine_for_large_list
            try:
                # tables (band-pass, template, taps) of this rate; lists above 256 paths: the large-list engine
                self._engine = engine_for_large_list(fs=self.fs_target) if large else engine_for_fs(self.fs_target)
            except ValueError as e:                                 # SciPy's own error (band above Nyquist) passes through, as in the reference
                if "taps" not in str(e):
                    raise
                raise NotImplementedError(f"fs_target = {self.fs_target}: {e} (DESIGN.md section 7)") from None
        return self._engine

    def _band_id(self, band) -> int:
        return BAND_PLAN.index((int(band[0]), int(band[1])))

    # ------------------------------------------------------------------ API
    def verify_wav(self, path: str) -> bool:
        """verify() for a WAV file (f-4 ingest): PCM16 samples stay int16 up to the band-pass kernel (x / 32768 there: the
        values soundfile.read hands the reference, rx_app.py:25-28)."""
        from .audiofile import read_wav
        samples, fs = read_wav(path)
        return self.verify(samples, fs)

    def _conditioned(self, audio, fs_in: int) -> np.ndarray:
        audio = np.asarray(audio)
        if audio.dtype == np.int16:
            if fs_in == self.fs_target:
                return audio                                 # ingested as int16 by the band-pass kernel
            audio = audio.astype(np.float32) / np.float32(32768.0)
        if fs_in != self.fs_target and audio.ndim == 1 and audio.size:
            # polyphase resampling on the device (es_resample_batch): the values scipy.signal.resample_poly returns
            return self.engine.resample(audio, fs_in, self.fs_target).cpu().numpy()
        signal, _ = resample_to(self.fs_target, audio, fs_in)
        return signal

    def _band_order(self):
        hop0 = self._hop.band(0)
        return [hop0] + [b for b in BAND_PLAN if b != hop0]                 # rtwm/detector.py:46-52

    def verify(self, audio: np.ndarray, fs_in: int, ctr0: int | None = None) -> bool:
        return self.verify_batch([audio], fs_in, None if ctr0 is None else [ctr0])[0]

    def verify_batch(self, clips, fs_in, ctr0=None) -> list[bool]:
        """verify() for several recordings ("full batched verify()"): the result, the order of tries
        and the evolution of `session_nonce` are those of calling the reference's verify() on the clips one after the other
        (rtwm/detector.py:44-53, 105-152); what is batched is the GPU work.  Clips of one sample type share launches whatever their
        lengths (ragged_buckets: sorted by length, rows x longest clip <= RAGGED_ROW_SAMPLES per launch).  Per launch: ONE sync launch
        sequence over (clips x 4 bands) records, ONE header decode over every peak that can hold a frame and ONE demodulate +
        list-decode + validate batch over the (peak, counter) candidates of all clips and bands; the host then walks clip by clip,
        in input order, and band by band in the reference's order with its early returns.
        ctr0: the counter origin of every clip, or one per clip with None entries allowed: the clip's first sample is
        where the frame of counter ctr0 starts, so a peak at `start` is looked for around ctr0 + round(start / 1215).  None (the
        default): the reference's estimate round(start / 1215), which finds frames of counters up to about the clip's length + 200."""
        fs_list = rate_list(fs_in, len(clips))
        origins = clip_origins(ctr0, clips, fs_list, self.fs_target)       # refused by name before any engine exists
        order = self._band_order()
        launches = cut_launches(clips, fs_list, self.fs_target, len(order), self._conditioned)
        scans: list = [None] * len(clips)
        for la in launches:
            for i, sc in zip(la.idx, self._scan_prepare(la, order)):
                sc.ctr0 = origins[i]
                scans[i] = sc
        return self._verify_scans(scans, [la.idx for la in launches], order)

    def _verify_scans(self, scans: list, launches: list, order: list, walkers: list | None = None) -> list[bool]:
        """Decode and walk the prepared scans of a verify_batch call (scans[i] None: clip i is shorter than the template).
        walkers: the detector that walks clip i -- its traces and its session_nonce -- where that is not this one (a LiveMonitor's
        private detector per stream, all of this detector's key: planning and decoding are stateless and stay here)."""
        # Decoding is stateless (the validator's verdict depends on blob and counter only; nonce bookkeeping happens on the host, in
        # _accept), so it is batched ahead of the walk; the WALK is clip by clip and band by band, in the reference's order with its
        # early returns.  When the walk needs a (clip, band) that is not decoded yet, that band and -- in walk order: the clip's
        # further bands, then the later clips of its launch -- as many further ones as fit under a cap on the candidates per batch go
        # through ONE demodulate + list-decode + validate batch.  A lone clip (a few hundred candidates) is decoded in one batch,
        # as before; a hundred unwatermarked clips at list size 256 (4 x 400 candidates x 4 variants each) no longer ask for
        # gigabytes of candidate rows at once, and what an early return makes unnecessary is bounded by the cap.
        plans: dict[int, list] = {i: [self._scan_plan(scans[i], bi) for bi in range(len(order))] for i in range(len(scans)) if scans[i] is not None}
        cache: dict[tuple[int, int], list] = {}
        group_of = {i: walk for walk in map(sorted, launches) for i in walk}         # a launch's clips in input order
        cap = self._pair_cap()

        def need(i: int, bi: int) -> list:
            if (i, bi) not in cache:
                todo = [(i, r) for r in range(bi, len(order))] + [(j, r) for j in group_of[i] if j > i and scans[j] is not None for r in range(len(order))]
                batch, n = [], 0
                for (j, r) in todo:
                    if (j, r) in cache:
                        continue
                    m = len(plans[j][r][0])
                    if batch and n + m > cap:
                        break
                    batch.append((j, r)); n += m
                flat = [(j, p) for (j, r) in batch for p in plans[j][r][0]]
                res = iter(self._decode_pairs_grouped([(scans[j].src, p[0], p[2]) for j, p in flat]) if flat else [])
                for (j, r) in batch:
                    cache[(j, r)] = list(itertools.islice(res, len(plans[j][r][0])))
            return cache[(i, bi)]

        def walk(i: int) -> bool:                                           # (any() stops at the first band that verifies: the early return)
            w = self if walkers is None else walkers[i]
            return any(w._scan_replay(scans[i], bi, plan, hdr_log, need(i, bi) if plan else []) for bi, (plan, hdr_log) in enumerate(plans[i]))
        return [scans[i] is not None and walk(i) for i in range(len(scans))]

    # ------------------------------------------------------------------ acquisition
    def acquire(self, audio: np.ndarray, fs_in: int, *, span=FULL_SPAN, max_records: int = 8) -> Acquired | None:
        return self.acquire_batch([audio], fs_in, span=span, max_records=max_records)[0]

    def acquire_batch(self, clips, fs_in, *, span=FULL_SPAN, max_records: int = 8) -> list:
        """Find a frame of this detector's key in each clip without knowing the clip's counter origin, and with it the origin: -> per
        clip None, or an Acquired whose ctr0 makes verify(clip, fs_in, ctr0=ctr0) the ordinary verify.  Where verify looks for a peak's
        counter around an estimate, this looks at every counter of `span` (default: all 2^32) that carries the low 16 bits the peak's
        header decoded to and hops to the band the peak was found in -- about a quarter of 65 536 per header over the full span.  The
        front is verify_batch's (cut_launches, one sync and one header decode per launch, mixed rates and int16 included); per launch
        ONE es_acquire_mask_batch and ONE es_acquire_list_batch enumerate the candidates of all its clips' records (at most max_records
        per clip, acquire.record_order); the walk is clip by clip in input order, record by record, counters ascending, and stops at the
        first candidate _accept takes -- with its session-nonce bookkeeping, and each try appended to _trace.  An empty span: all None,
        no GPU work.  ValueError before any engine exists: a span outside [0, 2^32] or reversed, max_records < 1."""
        span, max_records = check_span(span), check_max_records(max_records)
        fs_list = rate_list(fs_in, len(clips))
        out: list = [None] * len(clips)
        if span[0] == span[1]:
            return out
        order = self._band_order()
        plans: dict[int, tuple] = {}
        for la in cut_launches(clips, fs_list, self.fs_target, len(order), self._conditioned):
            scans = self._scan_prepare(la, order)
            for i, plan in zip(la.idx, self._acquire_plan(scans, [0] * len(scans), span, max_records)):
                plans[i] = plan
        for i in sorted(plans):
            out[i] = self._acquire_walk(*plans[i], self)
        return out

    def _key_ring(self):
        """This detector's key as a ring of one row, derived once per engine."""
        eng = self.engine
        if self._ring is None or self._ring[0] is not eng:
            self._ring = (eng, eng.keyring([self._band_key]))
        return self._ring[1]

    def _acquire_plan(self, scans: list, pos0: list, span, max_records: int) -> list:
        """The candidates of every scan of one launch, by one mask and one list launch over all their records
        -> per scan (scan, pos0, [header index j of each searched record], [its counters, ascending])."""
        recs = [record_order(sc.hdr[0][sc.sel], sc.hdr[1][sc.sel], sc.rows[sc.sel], sc.starts[sc.sel], p0, max_records) if sc.sel.size else []
                for sc, p0 in zip(scans, pos0)]
        recs = [[int(sc.sel[k]) for k in r] for sc, r in zip(scans, recs)]     # places in the launch's header decode
        flat = [(c, j) for c, r in enumerate(recs) for j in r]
        ctrs: list = [np.zeros(0, np.int64)] * len(flat)
        if flat:
            eng = self.engine
            lo16 = np.array([scans[c].hdr[1][j] for c, j in flat], np.int32)
            band = np.array([self._band_id(scans[c].bands[int(scans[c].rows[j])]) for c, j in flat], np.uint8)
            mask, count = eng.acquire_mask(self._key_ring(), np.zeros(len(flat), np.int32), np.ones(len(flat), np.uint8), lo16, band, span)
            count = count.cpu().numpy().astype(np.int64)
            base, total = np.cumsum(count) - count, int(count.sum())            # walk order: clip by clip, record by record
            if total:
                _, cc = eng.acquire_list(mask, lo16, span, base, total)
                cc = cc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                ctrs = [cc[b:b + n] for b, n in zip(base.tolist(), count.tolist())]
        ctrs = iter(ctrs)
        return [(sc, p0, r, [next(ctrs) for _ in r]) for sc, p0, r in zip(scans, pos0, recs)]

    def _acquire_walk(self, scan, pos0: int, recs: list, ctrs: list, walker) -> Acquired | None:
        """Decode one clip's candidates in try order, in chunks of _pair_cap(), and walk them with `walker` (its _trace, its
        session_nonce) up to the first it accepts."""
        tries = [(j, int(c)) for j, cs in zip(recs, ctrs) for c in cs]
        cap, tried = self._pair_cap(), 0
        for k in range(0, len(tries), cap):
            part = tries[k:k + cap]
            for (j, ctr), blobs in zip(part, self._decode_pairs(scan.src, [j for j, _ in part], [c for _, c in part])):
                band, start = scan.bands[int(scan.rows[j])], int(scan.starts[j])
                tried += 1
                if walker._trace is not None:
                    walker._trace.append((int(band[0]), start, ctr))
                if walker._accept(blobs, ctr):
                    blob = next(b for b in blobs if b is not None)
                    try:
                        plain = self.sec.open(blob)
                    except Exception:
                        plain = self._decrypt_blob_fallback(blob)[0] or blob
                    return Acquired(origin_of(ctr, start, pos0), ctr, start, (int(band[0]), int(band[1])), blob, plain, len(recs), tried)
        return None

    # ------------------------------------------------------------------ presence
    def presence(self, audio: np.ndarray, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), phases: int = 8, decoys: int = 32,
                 drift_ppm=0.0):
        return self.presence_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, phases=phases, decoys=decoys,
                                   drift_ppm=drift_ppm)[0]

    def presence_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0) -> list:
        """Tell whether each clip carries this key's mark, without demodulating anything: -> per clip a presence.Presence, or None for a
        clip without one whole 1215-sample slot.  The 63-chip preamble of every frame survives the channel where the payload does not
        (DESIGN 4.23), and it peaks in the band the HMAC-keyed hop sequence names: the score of a key is the mean, over the clip's
        frame slots on one 1215-sample grid, of the correlation rows the key hops through from some counter of `span`, maximised over
        the span and over the `phases` grid phases of largest keyless fold.  The same search runs under `decoys` public decoy keys
        (presence.decoy_keys); detected = the own score is strictly above every decoy's.  No threshold is tuned anywhere; the verdict
        is statistical, not authenticated.  ctr0 = c (one value, or one per clip with None entries allowed) is shorthand for
        span = (c, c + 2).  phases = 1215 searches every phase.
        drift_ppm > 0: the clip may have been captured on another sample clock than it was played on, up to drift_ppm
        parts per million fast or slow.  The grid then stretches: every total skew of -E .. E samples across the clip is tried
        (presence.skew_table), `phases` counts the (skew, phase) pairs of largest fold, and Presence.skew / drift_ppm / hypotheses say
        what was found; per launch ONE warp fold, ONE download and pick, ONE hop window and ONE warp score (es_warp_fold_batch,
        es_warp_score_batch).  All keys search the same pairs, so the verdict and its 1 / (decoys + 1) bound stand.  drift_ppm = 0 is
        the rigid grid: the calls and the bits of before.
        The front is verify_batch's (cut_launches, four rows per clip in BAND_PLAN order, mixed rates, int16 and unequal lengths
        included) with the correlation rows kept; per launch ONE fold, ONE hop window over the ring [key] + decoys and ONE score call.
        session_nonce and the traces are not touched.  ValueError before any engine exists: a span outside [0, 2^32], reversed or
        reaching past 2^32 from its last origin, phases outside 1 .. 1215, decoys < 0, a bad ctr0, a drift_ppm that is negative, not
        finite or no number, or that skews some clip by a whole frame or leaves it no slot."""
        return [None if r is None else r[0] for r in self._presence_clips(clips, fs_in, ctr0, span, phases, decoys, drift_ppm, None)]

    # ------------------------------------------------------------------ the presence timeline
    def presence_map(self, audio: np.ndarray, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), window: int = 40, step: int = 20,
                     confirm: int = 2, phases: int = 8, decoys: int = 32, drift_ppm=0.0):
        return self.presence_map_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, window=window, step=step, confirm=confirm,
                                       phases=phases, decoys=decoys, drift_ppm=drift_ppm)[0]

    def presence_map_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2, phases: int = 8,
                           decoys: int = 32, drift_ppm=0.0) -> list:
        """Which parts of each clip carry this key's mark, and where it was cut: -> per clip a presence.PresenceMap, or None for a clip
        without one whole 1215-sample slot.  The presence test (presence_batch) runs on windows of `window` slots every `step` slots
        (presence.map_windows; about 1 s every 0.5 s by default), each on its own frame grid, so a cut between two windows does not
        blur either.  A clip of at most `window` slots is one window: the map's single entry is presence() on the clip, field for field.
        span = (lo, hi) names the counters the clip's slot 0 may carry; the window that starts s slots in searches (lo + s, hi + s),
        lowered at 2^32 (presence.window_span), so a cut that removes up to hi - lo frames stays inside the search, and an insertion
        of up to lo.  ctr0 = c is shorthand for span = (c, c + 2), which follows no cut.  A detected window gives the grid anchor
        t = col + phase - 1215 ctr; adjacent detected windows whose anchors agree (presence.consistent: within 1 sample, plus what
        drift_ppm allows between them) form a stretch, one of at least `confirm` windows is confirmed, and successive confirmed
        stretches are joined by a Splice that says how many samples are missing between their grids.  A lone detected window is the
        1 / (decoys + 1) event the rule allows per window and confirms nothing; every verdict stays statistical.
        drift_ppm > 0 gives each window the drift search of DESIGN 4.24 over its own length.
        The front is presence_batch's; then per launch the windows of all its clips go through presence_search.search_map: per group of
        windows ONE fold, ONE device pick (es_fold_pick_batch), ONE hop window and ONE score per span width, never a launch per window.
        ValueError before any engine exists: what presence_batch refuses of span, ctr0, decoys and drift_ppm (the drift judged on a
        window), window, step or confirm that are no integers, step < 1, step > window, confirm < 1, phases outside 1 .. 64."""
        return [None if r is None else r[0] for r in self._presence_clips(clips, fs_in, ctr0, span, phases, decoys, drift_ppm, None,
                                                                          grid=(window, step, confirm))]

    def _presence_clips(self, clips, fs_in, ctr0, span, phases, decoys, drift_ppm, keys, grid=None) -> list:
        """presence_batch under each of `keys` (None: this detector's key alone) -> per clip None or one Presence per key.  The checks,
        the front and the launches are the same whatever the keys: the fold and the hypothesis list are keyless, so one front and one
        score call over the ring keys + decoys serve them all (presence_search.search).  grid = (window, step, confirm):
        presence_map_batch instead, one PresenceMap per key, the same front with presence_search.search_map behind it."""
        from . import presence as pr, presence_search as ps
        clips = list(clips)
        fs_list = rate_list(fs_in, len(clips))
        P, R, drift = pr.check_phases(phases), pr.check_decoys(decoys), pr.check_drift(drift_ppm)
        if grid is not None:
            grid = pr.check_map(*grid, P)[:3]
        spans = pr.clip_spans(ctr0, span, len(clips))
        for c, f, s in zip(clips, fs_list, spans):                          # refused by name before any engine exists
            samples = resampled_length(int(np.size(c)), int(f), self.fs_target)
            if grid is None:
                pr.check_reach(s, samples)
            if drift > 0:
                for n in {samples - (PRE_L - 1)} if grid is None else {w[2] for w in pr.map_windows(samples - (PRE_L - 1), *grid[:2])}:
                    pr.skew_table(n, drift)
        out: list = [None] * len(clips)
        n_own = 1 if keys is None else len(keys)
        for span, ids, f in self._presence_front(clips, fs_list, spans, want_corr=True):
            nlag = np.array(f.sizes, np.int64) - (PRE_L - 1)
            if not n_own:
                res = [None] * len(ids)
            elif grid is None:
                res = ps.search(self.engine, self._presence_ring(R, keys), n_own, f.corr, nlag, [span] * len(ids), drift, P)
            else:
                res = ps.search_map(self.engine, self._presence_ring(R, keys), n_own, f.corr, nlag, [span] * len(ids), drift, P, *grid)
            if self._presence_rows is not None and any(r is not None for r in res):
                self._presence_rows.append((ids, f.corr.cpu().numpy(), nlag))
            for i, r in zip(ids, res):
                out[i] = r
        return out

    def _presence_front(self, clips, fs_list, spans, want_corr: bool, slots=None):
        """The front the presence calls share -> per span, in sorted order, and per launch of the clips of that span (cut_launches: clips
        of one span share launches; one span: the whole call): (span, the clips' indices in the call, _Front) with the launch's
        band-passed rows y and, where want_corr, its correlation rows -- four rows per clip in BAND_PLAN order; equal lengths run bpf
        and xcorr, unequal ones sync_ragged.  slots(sizes) -> the slots of each clip: a launch without any is skipped before an engine
        is touched, and the others carry them as _Front.J."""
        import torch
        band_ids = np.arange(len(BAND_PLAN), dtype=np.uint8)
        nb = band_ids.size
        for span in sorted(set(spans)):
            ids = [i for i, s in enumerate(spans) if s == span]
            for la in cut_launches([clips[i] for i in ids], [fs_list[i] for i in ids], self.fs_target, nb, self._conditioned):
                J = None if slots is None else slots(la.sizes)
                if J is not None and not J.max():
                    continue
                eng = self.engine
                x, sizes = la.rows(eng, nb)
                bid = dev(eng, np.tile(band_ids, len(sizes)), np.uint8)
                M = max(sizes)
                lens = np.repeat(np.array(sizes, np.int32), nb)
                if min(sizes) < M:
                    sy = eng.sync_ragged(x, torch.from_numpy(lens), bid, keep_corr=want_corr)
                    y, corr = sy.y, sy.corr
                else:
                    y = eng.bpf(x[:, :M], bid)
                    corr = eng.xcorr(y, bid) if want_corr else None
                yield span, [ids[i] for i in la.idx], _Front(sizes, lens, bid, y, corr, J)

    # ------------------------------------------------------------------ the coherent presence test
    def presence_coherent(self, audio: np.ndarray, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), phases: int = FRAME_LEN,
                          decoys: int = 32):
        return self.presence_coherent_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, phases=phases, decoys=decoys)[0]

    def presence_coherent_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), phases: int = FRAME_LEN, decoys: int = 32) -> list:
        """presence_batch with a statistic that also works on loud hosts: -> per clip a presence.Presence, or None for a clip without
        one whole slot.  Per hypothesised (key, counter) the receiver knows 191 chips of every frame: the 63 of the preamble and the 128
        of the header, the counter's low 16 bits over 8 chips each times the key's header PN.  The score of a key is the mean, over the
        clip's frame slots on one 1215-sample grid, of the normalised correlation of all 191 with the matched-filter row of the band
        the key hops to (presence.coherent_score_model), maximised over the span and over EVERY phase of the grid (phases = 1215, the
        identity list): no keyless guess of the phase is needed, which is what failed on loud hosts.  phases < 1215 searches the top
        of presence_batch's keyless fold instead: the cheap mode, kept for comparison.  The verdict is presence_batch's
        (presence.verdict): strictly above every decoy, every key scored on the same rows, span and phases; statistical, never
        authenticated.  Presence.frames is J = max(0, n - 189 - L_max) // 1215 for a clip of n samples and a longest matched filter of
        L_max taps.  ctr0 as for presence_batch.
        The front is presence_batch's (cut_launches; mixed rates, int16 and unequal lengths included: equal lengths run bpf, ragged
        ones sync_ragged, whose y is kept); per launch, for each span, ONE mf_rows, ONE hop window over the ring [key] + decoys and ONE
        score call (es_mf_rows_batch, es_coherent_score_batch).  session_nonce and the traces are not touched.  ValueError before any
        engine exists: what presence_batch refuses of span, ctr0, phases and decoys, the reach of the span judged with this J."""
        return [None if r is None else r[0] for r in self._presence_coherent_clips(clips, fs_in, ctr0, span, phases, decoys, None)]

    # ------------------------------------------------------------------ the coherent presence timeline
    def presence_coherent_map(self, audio: np.ndarray, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), window: int = 40, step: int = 20,
                              confirm: int = 2, decoys: int = 32):
        return self.presence_coherent_map_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, window=window, step=step,
                                                confirm=confirm, decoys=decoys)[0]

    def presence_coherent_map_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2,
                                    decoys: int = 32) -> list:
        """presence_map_batch with the statistic that works on loud hosts: -> per clip a presence.PresenceMap, or None for a clip without
        one whole slot.  The coherent test (presence_coherent_batch) runs on windows of `window` slots every `step` slots
        (presence.coherent_windows, cut by the coherent J = max(0, n - 189 - L_max) // 1215), each on its own frame grid and under its
        own span (presence.window_span); detected windows whose grid anchors agree form stretches, one of at least `confirm` windows is
        confirmed, and successive confirmed stretches are joined by a Splice (presence.stretches, on the rigid grid).  A clip of at
        most `window` slots is one window: the map's single entry is presence_coherent() on the clip, field for field -- except for a
        span that reaches past 2^32 from its last origin, which presence_coherent() refuses and the window lowers.  Every phase
        is always searched -- the keyless cheap mode is what fails on loud hosts -- and there is no drift search.  A lone detected
        window is the 1 / (decoys + 1) event the rule allows per window and confirms nothing; every verdict stays statistical.
        The front is presence_coherent_batch's (cut_launches; mixed rates, int16 and unequal lengths; bpf or sync_ragged) with ONE
        mf_rows per launch; the windows of all its clips then read the clip's own rows in place (presence_search.search_coherent_map):
        per group of windows ONE hop window and ONE score call per span width (es_coherent_score_at_batch), never a launch per window.
        ValueError before any engine exists: what presence_coherent_batch refuses of span, ctr0 and decoys (the reach is judged per
        window, which lowers its span at 2^32), and what presence.check_map refuses of window, step and confirm."""
        return [None if r is None else r[0] for r in self._presence_coherent_clips(clips, fs_in, ctr0, span, FRAME_LEN, decoys, None,
                                                                                   grid=(window, step, confirm))]

    def _presence_coherent_clips(self, clips, fs_in, ctr0, span, phases, decoys, keys, grid=None) -> list:
        """presence_coherent_batch under each of `keys` (None: this detector's key alone) -> per clip None or one Presence per key: the
        rows are keyless, so one front and one score call over the ring keys + decoys serve them all.  grid = (window, step, confirm):
        presence_coherent_map_batch instead, one PresenceMap per key, the same front with presence_search.search_coherent_map behind it
        (without one: presence_search.search_coherent)."""
        from . import presence as pr, presence_search as ps
        from .tables import pack_tables
        clips = list(clips)
        fs_list = rate_list(fs_in, len(clips))
        P, R = pr.check_phases(phases), pr.check_decoys(decoys)
        if grid is not None:
            grid = pr.check_map(*grid, 1)[:3]
        spans = pr.clip_spans(ctr0, span, len(clips))
        g, _ = pr.mf_tables(tables=pack_tables(self.fs_target))
        if grid is None:
            for c, f, s in zip(clips, fs_list, spans):                      # refused by name before any engine exists
                pr.check_coherent_reach(s, resampled_length(int(np.size(c)), int(f), self.fs_target), g)
        n_own = 1 if keys is None else len(keys)
        out: list = [None] * len(clips)
        if not n_own:
            return out
        slots = lambda sizes: np.array([pr.coherent_slots(n, g) for n in sizes], np.int64)
        for (lo, hi), ids, f in self._presence_front(clips, fs_list, spans, want_corr=P < FRAME_LEN, slots=slots):
            eng = self.engine
            if P < FRAME_LEN:                                               # the cheap mode: the top of the keyless fold (presence_batch's list)
                fold = eng.phase_fold(f.corr, np.array(f.sizes, np.int64) - (PRE_L - 1)).cpu().numpy()
                lists = [pr.pick_phases(row, P) for row in fold]
            else:
                lists = [list(range(FRAME_LEN))] * len(ids)
            rows = eng.mf_rows(f.y, f.lens, f.bid)
            ring = self._presence_ring(R, keys)
            if grid is None:
                res = ps.search_coherent(eng, ring, n_own, *rows, f.J, lists, lo, hi)
            else:
                res = ps.search_coherent_map(eng, ring, n_own, *rows, f.sizes, [(lo, hi)] * len(ids), g, *grid)
            if self._presence_rows is not None:
                self._presence_rows.append((ids, f.y.cpu().numpy(), np.array(f.sizes, np.int64)))
            for i, r in zip(ids, res):
                out[i] = r
        return out

    def _presence_ring(self, decoys: int, keys=None):
        """The ring [own keys] + the first `decoys` public decoy keys (keys None: this detector's key alone), derived once per engine,
        count and key list."""
        from .presence import decoy_keys
        eng = self.engine
        own = (self._band_key,) if keys is None else tuple(bytes(k) for k in keys)
        if self._decoy_ring is None or self._decoy_ring[0] is not eng or self._decoy_ring[1] != (decoys, own):
            self._decoy_ring = (eng, (decoys, own), eng.keyring(list(own) + decoy_keys(decoys)))
        return self._decoy_ring[2]

    def open_streams(self, n: int, *, fs=None, window_s: float = 5.0, chunk_max: int | None = None, trace: bool = False,
                     ctr0=None) -> "LiveMonitor":
        """A monitor of n live streams, all verified under this detector's key: LiveMonitor.push takes their next chunks and says, stream
        by stream, whether the last window_s seconds verify.  fs: the rate the streams arrive at, one or one per stream (None:
        fs_target); a stream at another rate is conditioned on the device chunk by chunk, to the samples of
        resample_poly(whole stream) that no later sample changes (finite samples only).  window_s and chunk_max (default
        half a second) count time and samples at fs_target: a chunk may finalize at most chunk_max conditioned samples.  trace=True
        records each stream's tries and header decodes of its last push (LiveMonitor.traces).  ctr0: the counter origin of every
        stream, or one per stream with None entries allowed -- what the issuer opened the stream with (WatermarkIssuer.open_streams):
        frame k of the stream carries counter ctr0 + k, and a push looks for a peak's counter around that of its absolute position
        (DESIGN 4.18).  None: estimates relative to the window, which follow a stream marked from counter 0 for its first seconds."""
        from .monitor import open_arguments
        band_ids = [self._band_id(b) for b in self._band_order()]
        how = open_arguments(n, self.fs_target, bands=band_ids, fs=fs, window_s=window_s, chunk_max=chunk_max, ctr0=ctr0)      # refuses before any engine exists
        return LiveMonitor(self, self.engine.open_monitor(int(n), **how), trace=trace)

    # one scan = what _scan_band_multi_frame needs for every band of one clip, produced in batched launches
    def _scan_prepare(self, signals, bands: list) -> list:
        """signals: a Launch, or host signals at fs_target (one sample type, none shorter than the template) that make one."""
        eng = self.engine
        launch = signals if isinstance(signals, Launch) else Launch(list(range(len(signals))), [sg.size for sg in signals], signals, None, self.fs_target)
        band_ids = np.array([self._band_id(b) for b in bands], np.uint8)
        return self._scans_of(sync_launch(eng, launch, band_ids), bands, band_ids)

    def _scans_of(self, ss, bands: list, band_ids: np.ndarray) -> list:
        """The scans of a SyncScan's clips: one header decode over every peak that can hold a frame, under this detector's key."""
        eng = self.engine
        nb, rows_a = ss.nb, ss.rows
        src = None
        hdr = (np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0))
        if rows_a.size:
            # frame j = sy.y[frame_rows[j], frame_cols[j] : frame_cols[j] + 1215], read in place (no [P, 1215] copy)
            src = _Frames(ss.sy.y, ss.frame_rows, ss.frame_cols)
            okh, val, score = eng.header(ss.sy.y, dev(eng, band_ids[rows_a % nb], np.uint8), dev(eng, np.packbits(self.sec.pn_bits(0, HDR_L)).reshape(1, -1), np.uint8),
                                         rows=dev(eng, src.rows, np.int32), start=dev(eng, src.starts, np.int32))
            hdr = (okh.cpu().numpy().astype(bool), val.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64))
        return [_Scan(bands, src, rows_a - c * nb, np.flatnonzero((rows_a // nb) == c), ss.starts, hdr) for c in range(len(ss.sizes))]

    def _scan_plan(self, scan, bi: int):
        """The candidate (peak, counter) pairs of one band in the reference's try order (rtwm/detector.py:105-140):
        -> (plan [(peak slot j, start, ctr, header-log index)], header log of the peaks looked at)."""
        band = scan.bands[bi]
        sel = np.asarray(scan.sel, np.int64)[np.asarray(scan.rows)[scan.sel] == bi]     # this band's peaks, in peak order
        idx, starts, ok, lo16, score = [sel.tolist()] + [np.asarray(a)[sel].tolist() for a in (scan.starts, *scan.hdr)]
        # estimates: rtwm/detector.py:117, or with an origin the counter of the frame at the peak's absolute position
        at = (0, 0) if scan.ctr0 is None else (scan.pos0, scan.ctr0)
        tries, looked = plan_tries(starts, ok, lo16, lambda ctr: self._hop.band(ctr) == band, *at)
        hdr_log = [(float(bool(a)), float(int(b)), float(c)) for a, b, c in zip(ok[:looked], lo16[:looked], score[:looked])]
        return [(idx[h], starts[h], ctr, h) for h, cs in tries for ctr in cs], hdr_log    # (.., index of the peak's header decode in hdr_log)

    def _scan_replay(self, scan, bi: int, plan, hdr_log, results) -> bool:
        """Walk one band's decoded candidates as the reference does (early return, traces, nonce bookkeeping in _accept)."""
        band = scan.bands[bi]
        for (j, start, ctr, h), blobs in zip(plan, results):
            if self._trace is not None:
                self._trace.append((int(band[0]), int(start), int(ctr)))
            if self._accept(blobs, ctr):
                if self._hdr_trace is not None:                             # the reference decodes a peak's header when it reaches the peak:
                    self._hdr_trace.extend(hdr_log[:h + 1])                 # peaks after the accepted one were never looked at
                return True
        if self._hdr_trace is not None:
            self._hdr_trace.extend(hdr_log)
        return False

    def _scan_decide(self, scan, bi: int) -> bool:
        """The per-band loop of _scan_band_multi_frame (rtwm/detector.py:105-152) over prepared peaks / headers."""
        plan, hdr_log = self._scan_plan(scan, bi)
        results = self._decode_pairs(scan.src, [p[0] for p in plan], [p[2] for p in plan]) if plan else []
        return self._scan_replay(scan, bi, plan, hdr_log, results)

    def verify_raw_frame(self, signal: np.ndarray) -> bool:
        signal = np.asarray(signal)
        if len(signal) == FRAME_LEN:
            for ctr in range(4):
                band = self._hop.band(ctr)
                y = self._bandpass(signal, band)
                if self._try_decode_frame(y, ctr):
                    return True
        return self._scan_band_multi_frame(signal, self._hop.band(0))

    def _scan_band(self, signal: np.ndarray, band, skip_filtering: bool = False) -> bool:
        return self._scan_band_multi_frame(signal, band)

    def _try_window(self, frame: np.ndarray, ctr0: int, delta: int) -> bool:
        for ctr in range(max(0, ctr0 - delta), ctr0 + delta + 1):
            if self._try_decode_frame(frame, ctr):
                return True
        return False

    # ------------------------------------------------------------------ sync (GPU)
    def _bandpass(self, signal: np.ndarray, band) -> np.ndarray:
        x = dev(self.engine, np.asarray(signal).astype(np.float32, copy=False).reshape(1, -1), np.float32)
        b = dev(self.engine, np.array([self._band_id(band)]), np.uint8)
        return self.engine.bpf(x, b)[0].cpu().numpy()

    def _sync(self, signal: np.ndarray, band):
        """-> (y float64[M], thr, peaks list) or None when the record is shorter than the template."""
        sig = np.asarray(signal).astype(np.float32, copy=False).reshape(-1)
        if sig.size < PRE_L:                               # rtwm/detector.py:71-73
            return None
        x = dev(self.engine, sig.reshape(1, -1), np.float32)
        b = dev(self.engine, np.array([self._band_id(band)]), np.uint8)
        sy = self.engine.sync(x, b, keep_corr=False)
        n = int(sy.npeaks[0].item()) & 0xFFFF
        peaks = [int(p) for p in sy.peaks[0, : min(n, sy.peaks.shape[1])].cpu().numpy()]
        return sy.y[0].cpu().numpy(), float(sy.thr[0].item()), peaks

    def _scan_band_multi_frame(self, signal: np.ndarray, band) -> bool:
        sig = np.asarray(signal).reshape(-1)
        if sig.dtype != np.int16:
            sig = sig.astype(np.float32, copy=False)
        if sig.size < PRE_L:                                   # rtwm/detector.py:71-73
            return False
        return self._scan_decide(self._scan_prepare([sig], [band])[0], 0)

    # ------------------------------------------------------------------ demod + FEC (GPU)
    def _matched_filter_taps(self, band):
        key = (band[0], band[1], self.fs_target)
        h = self._mf_cache.get(key)
        if h is None:
            h = self._mf_cache[key] = matched_filter_taps((int(band[0]), int(band[1])), self.fs_target)
        return h

    def _pn_rows(self, ctrs) -> np.ndarray:
        return self.sec.pn_bytes_batch(list(ctrs), 152)

    def _llr(self, frame: np.ndarray, frame_id: int, pn_variant: int = 0) -> np.ndarray:
        frame = np.asarray(frame, dtype=np.float64).reshape(-1)
        if frame.size == 0:
            return np.zeros(N_DEFAULT, dtype=np.float32)
        band = self._hop.band(frame_id)
        y = dev(self.engine, frame.reshape(1, -1), np.float64)
        out = self.engine.llr(y, dev(self.engine, np.array([self._band_id(band)]), np.uint8),
                              dev(self.engine, self._pn_rows([frame_id]), np.uint8), variant=int(pn_variant))
        return out[0].cpu().numpy()

    def _decode_header(self, frame: np.ndarray, band) -> tuple[bool, int, float]:
        frame = np.asarray(frame, dtype=np.float64).reshape(-1)
        if frame.size < PRE_L + HDR_L:                     # rtwm/detector.py:461-462
            return False, 0, 0.0
        y = dev(self.engine, frame.reshape(1, -1), np.float64)
        ok, val, score = self.engine.header(y, dev(self.engine, np.array([self._band_id(band)]), np.uint8),
                                            dev(self.engine, np.packbits(self.sec.pn_bits(0, HDR_L)).reshape(1, -1), np.uint8))
        return bool(ok[0].item()), int(val[0].item()), float(score[0].item())

    def _validator(self, frame_ctr: int):
        def check(payload: bytes) -> bool:
            try:
                pt = self.sec.open(payload)
            except Exception:
                return False
            return pt.startswith(b"ESAL") and int.from_bytes(pt[4:8], "big") == frame_ctr
        return check

    def _decode_candidates(self, frame: np.ndarray, ctrs) -> list[list[bytes | None]]:
        """For every counter: the four polar decodes the reference tries in order
        (+llr0, -llr0, +llr1, -llr1; rtwm/detector.py:161-190), each None or a 55-byte blob."""
        ctrs = list(ctrs)
        if not ctrs:
            return []
        y = dev(self.engine, np.asarray(frame, dtype=np.float64).reshape(1, -1), np.float64)
        return self._decode_pairs(_Frames(y, np.zeros(1, np.int64), np.zeros(1, np.int64)), [0] * len(ctrs), ctrs)

    def _decode_pairs_grouped(self, triples) -> list[list[bytes | None]]:
        """_decode_pairs for (frames, frame index, ctr) triples that may come from several clips (each group of equally long clips
        has its own _Frames): consecutive triples of one _Frames go through one call."""
        out: list = []
        for _, run in itertools.groupby(triples, key=lambda t: id(t[0])):
            run = list(run)
            out += self._decode_pairs(run[0][0], [t[1] for t in run], [t[2] for t in run])
        return out

    def _pair_cap(self) -> int:
        """(frame, counter) pairs per decode launch: at most 2^18 list paths per sign / PN variant (1 024 pairs at the default list
        size 256 -- the candidate rows of one launch are then 58 MB --, 32 768 at list size 8)."""
        return max(64, (1 << 18) // max(1, self._list_size))

    def _decode_pairs(self, frames, rows, ctrs) -> list[list[bytes | None]]:
        """Chunked front of _decode_pairs_chunk, so that a long candidate list never asks for gigabytes at once."""
        cap = self._pair_cap()
        return [r for k in range(0, max(1, len(ctrs)), cap) for r in self._decode_pairs_chunk(frames, rows[k:k + cap], ctrs[k:k + cap])]

    def _decode_pairs_chunk(self, frames, rows, ctrs) -> list[list[bytes | None]]:
        """The same for (frame, counter) pairs: frames = _Frames, pair i = (frame rows[i] of it, ctrs[i]).
        One batch: two demodulations (PN variants 0 / 1) read in place at the frames' (row, start), one list decode of the 4 B
        sign / variant combinations, one validation + selection (es_select_batch with the AEAD key) -- no host round trip per
        candidate."""
        from .engine import select_payload
        import torch
        eng = self.engine
        B = len(ctrs)
        j = np.asarray(rows, np.int64)
        # PN rows and band indices of the candidate counters straight from the device schedule (es_schedule_batch)
        at = dev(eng, frames.rows[j], np.int32), dev(eng, frames.starts[j], np.int32)
        pn, bands = eng.schedule(self.sec._prng.sub_key, self._band_key, ctrs=torch.tensor(ctrs, dtype=torch.int64))
        res = decode_four(eng, frames.y, *at, pn, bands, self._list_size)
        key = getattr(self._aead, "_key", None)
        if key is not None:
            # validator + candidate selection on the GPU (es_select_batch): same rules as select_payload with
            # self._validator(ctr), without a Python callback per candidate
            payload, ok, _which = eng.select(res, key32=key, ctrs=torch.tensor(ctrs * 4, dtype=torch.int64))
            payload = payload.cpu().numpy(); ok = check_decoded(ok.cpu().numpy())
            return [[payload[v * B + i].tobytes() if ok[v * B + i] == 1 else None for v in range(4)] for i in range(B)]
        out = []
        for i, ctr in enumerate(ctrs):
            val = self._validator(ctr)
            row = []
            for v in range(4):
                payload, ok = select_payload(res, v * B + i, val)
                row.append(payload if ok else None)
            out.append(row)
        return out

    def _accept(self, blobs, frame_ctr: int) -> bool:
        """Tail of _try_decode_frame (rtwm/detector.py:182-233): first non-None blob, AEAD open,
        magic, counter, session-nonce bookkeeping."""
        blob = next((b for b in blobs if b is not None), None)
        if blob is None:
            return False
        try:
            plain = self.sec.open(blob)
        except Exception:
            fb, _layout = self._decrypt_blob_fallback(blob)
            if fb is not None:
                plain = fb
            elif len(blob) >= 4 and blob[:4] == b"ESAL":
                plain = blob
            else:
                return False
        if not plain.startswith(b"ESAL"):
            return False
        if int.from_bytes(plain[4:8], "big") != frame_ctr:
            return False
        nonce = plain[8:16]
        if self.session_nonce and nonce == self.session_nonce:
            return True
        if self.session_nonce is None:
            self.session_nonce = nonce
            return True
        return False

    def _try_decode_frame(self, frame: np.ndarray, frame_ctr: int) -> bool:
        return self._accept(self._decode_candidates(frame, [frame_ctr])[0], frame_ctr)

    def _decrypt_blob_fallback(self, blob: bytes):
        if self._aead is None:
            return None, None
        if len(blob) >= 12:
            for nonce, body, name in ((blob[:12], blob[12:], "nonce-front"), (blob[-12:], blob[:-12], "nonce-tail")):
                try:
                    return self._aead.decrypt(nonce, body, b""), name
                except InvalidTag:
                    pass
        return None, None


class LiveMonitor(LiveTable):
    """The monitored streams of a WatermarkDetector (WatermarkDetector.open_streams); stream ids are the slots of `table`.

    Stream s behaves as a private WatermarkDetector(key, fs_target, list_size) that is called once per push, in push order, on the
    stream's window [w0, n) -- while the stream is shorter than the window, exactly verify(everything received so far, fs_target) --
    with its own session_nonce and, with trace=True, its own traces.  What differs is the work: the band-pass and the correlation are
    continued from the previous push instead of started again, and nothing but the new chunk is uploaded.  Every push
    walks its whole window, as verify would.  A stream opened at another rate is conditioned on the device first; "the stream" above is
    then its conditioned stream, resample_poly(everything received)[:F(n)]."""

    def __init__(self, detector: WatermarkDetector, table, *, trace: bool = False) -> None:
        self._det, self.table, self._trace = detector, table, bool(trace)
        self._order = detector._band_order()
        self._walkers: dict[int, WatermarkDetector] = {}

    @property
    def fs_target(self) -> int:
        return self._det.fs_target

    @property
    def engine(self):
        return self._det.engine

    def _fresh_walkers(self, ids) -> list:
        """The walkers of streams `ids` -- the detector's key, tables and engine, a session nonce and traces of their own --, the traces
        emptied for the call at hand."""
        walkers = []
        for s in map(int, ids):
            w = self._walkers.get(s)
            if w is None:
                w = self._walkers[s] = copy.copy(self._det)
                w.session_nonce = None
            w._trace, w._hdr_trace = ([], []) if self._trace else (None, None)
            walkers.append(w)
        return walkers

    def _window_scans(self, ids, chunks):
        """One tick over streams `ids` -> (the scans of their windows under the detector's key, each window's absolute first sample)."""
        tick = self.engine.monitor_step(self.table, ids, chunks)
        return self._det._scans_of(SyncScan.from_monitor(tick), self._order, self.table.bands), (self.table.base_host[ids] + tick.offset[::tick.nb]).tolist()

    def push(self, chunks, streams=None, *, fs: int | None = None) -> list[bool]:
        """chunks[i], 1-D int16 or float32 at the rate its stream was opened with, continues stream streams[i] (None: one chunk per open
        stream, in order) -> per chunk, whether the stream's window now verifies.  Streams not named are not touched.  fs= is a
        check, not a conversion: every named stream must have been opened at that rate.  Raises ValueError before any GPU work for
        that, a chunk that is not 1-D, longer than chunk_max or (at another rate) finalizing more than chunk_max samples, a stream
        named twice, outside the table or closed."""
        from .monitor import push_arguments
        ids, arrs, _ = push_arguments(self.table, self.fs_target, chunks, streams, fs)
        if not ids.size:
            return []
        scans, pos0 = self._window_scans(ids, arrs)
        for sc, s, p0 in zip(scans, ids.tolist(), pos0):                    # a stream with an origin: estimates from absolute positions
            if self.table.origin_host[s] >= 0:
                sc.ctr0, sc.pos0 = int(self.table.origin_host[s]), p0
        return self._det._verify_scans(scans, [list(range(len(scans)))], self._order, self._fresh_walkers(ids))

    def acquire_streams(self, streams) -> np.ndarray:
        """The streams an acquire call names, checked on the host: None = every open stream without an origin; a named stream must be
        open, named once and without an origin."""
        from .monitor import monitor_ids
        if streams is None:
            return np.flatnonzero(self.table.live & (self.table.origin_host < 0))
        ids = monitor_ids(self.table, streams)
        for s in ids.tolist():
            if self.table.origin_host[s] >= 0:
                raise ValueError(f"stream {s} already has a counter origin ({int(self.table.origin_host[s])}): there is nothing to acquire")
        return ids

    def acquire(self, streams=None, *, span=FULL_SPAN, max_records: int = 8) -> list:
        """WatermarkDetector.acquire on the current window of each named stream (None: every open stream without an origin), with no new
        samples: -> per stream None or an Acquired.  The window's absolute position is known, so a found frame gives the stream's counter
        origin, ctr0 = ctr - round((w0 + start) / 1215): it is stored (origin(s) answers it) and later pushes plan from absolute positions
        as for a stream opened with it -- unless the samples received so far would reach the end of the counter range from
        it (scan.check_counter_reach), in which case the result is returned and the stream stays without an origin.  Each stream is
        walked by its own walker: the session nonce is the stream's, and with trace=True traces(s) then holds the tries of this call.
        ValueError before any GPU work: a span outside [0, 2^32] or reversed, max_records < 1, a stream that is closed, named twice,
        outside the table or has an origin already.  An empty span: all None, no GPU work."""
        span, max_records = check_span(span), check_max_records(max_records)
        ids = self.acquire_streams(streams)
        if not ids.size or span[0] == span[1]:
            return [None] * int(ids.size)
        det, tab = self._det, self.table
        scans, pos0 = self._window_scans(ids, [np.zeros(0, np.float32)] * int(ids.size))       # no samples: the windows as they stand
        plans = det._acquire_plan(scans, pos0, span, max_records)
        out = []
        for s, plan, w in zip(ids.tolist(), plans, self._fresh_walkers(ids)):
            acq = det._acquire_walk(*plan, w)
            if acq is not None:
                try:
                    check_counter_reach(acq.ctr0, int(tab.n_host[s]), "stream")
                    tab.origin_host[s] = acq.ctr0
                except ValueError:
                    pass
            out.append(acq)
        return out

    def presence(self, streams=None, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0) -> list:
        """WatermarkDetector.presence on the current window [w0, n) of each named stream (None: every open stream), with no new samples:
        -> per stream a presence.Presence, or None for a window without one whole 1215-sample slot.  The window's correlation rows are
        the table's own: nothing but a few small tables is uploaded, no band-pass and no correlation runs again.  A stream
        with a counter origin searches the two counters its window's first frame can carry (presence.live_span); one without searches
        `span`, read as absolute counters of the window's first frame.  Presence.ctr is the counter of the window's first whole frame,
        phase its first sample relative to the window, ctr0 = acquire.origin_of(ctr, phase, w0).  drift_ppm as for
        WatermarkDetector.presence, over the window.
        Per call ONE fold launch over all named streams, ONE download and pick, ONE hop window over the ring [key] + decoys with a hop
        row per distinct span base, and ONE score launch per group of equal span width (streams with an origin, streams without).
        The verdict is statistical, not authenticated: it never sets a stream's origin, and the table, the session nonces
        and the traces are not touched.  ValueError before any GPU work: a bad span, phases, decoys or drift_ppm, a span that reaches
        past 2^32 from its last origin, a stream that is closed, named twice or outside the table."""
        return [None if r is None else r[0] for r in self._presence(self._det, None, streams, span, phases, decoys, drift_ppm)]

    def session_nonce(self, stream: int) -> bytes | None:
        """The session nonce stream `stream` is locked to (None: nothing accepted yet)."""
        w = self._walkers.get(int(stream))
        return None if w is None else w.session_nonce

    def traces(self, stream: int):
        """(tries, header decodes) of the stream's last push, as WatermarkDetector._trace / _hdr_trace record them (trace=True)."""
        w = self._walkers.get(int(stream))
        return (None, None) if w is None else (w._trace, w._hdr_trace)

    def _slots_changed(self, ids, closed: bool) -> None:
        for s in ids if closed else ():                                     # a closed stream's session nonce and traces go with it
            self._walkers.pop(int(s), None)
