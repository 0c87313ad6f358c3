"""WatermarkIdentifier: which of many keys marked a recording?

For a clip and keys k_0 .. k_{N-1} the answer for key k_i is exactly what a freshly built
WatermarkDetector(k_i, fs_target=..., list_size=...).verify(clip, fs_in) gives (same boolean, same tries in the same order, and for a
match the blob it accepted) -- that single-key path, pinned to the reference by tests/golden/, is the definition.  What differs is the
work: the key-independent half of the search (conditioning, four band-passes, four correlation rows, peak picking) runs once per clip,
and everything keyed runs for all keys at once from a key ring on the device:

    keys -> es_keyring_derive_batch                      (rtwm/crypto.py:19-30, rtwm/utils.py:86-88)
    header decode per (key, peak) -> es_header_at_batch  (rtwm/detector.py:452-515)
    hop table per (key, counter) -> es_schedule_keyed_batch, bands only
    candidate planning per (key, clip, band) -> es_plan_batch                  (rtwm/detector.py:105-142)
    band rank by band rank (rank 0 = each key's band of counter 0): es_schedule_keyed_batch -> es_llr_at_batch x 2 variants ->
    es_scl_batch -> es_select_keyed_batch over the candidates of every key still unmatched

Each key starts with session_nonce = None, so a key matches iff some candidate of its walk validates (AEAD opens, "ESAL", counter
equal), and the first such candidate in the reference's walk order is the reported one.  Nonce state across calls is out of scope.

Live streams (WatermarkIdentifier.open_streams -> LiveIdentifier): the same walk over a monitor tick's scan instead of a
sync call's, frames read in place in the monitor's history, and a memo on the device (memo.py, es_memo_probe_batch /
es_memo_insert_batch) of candidates already known to fail, so that a push decodes only what no earlier push has decoded.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import memo
from ._native import ES_MAX_PEAKS, ES_MAX_TRIES, NativeError
from .detector import WatermarkDetector, check_decoded, clip_origins, decode_four
from .monitor import LiveTable
from .scan import FRAME_LEN, MAX_TRIES, PEAK_LIMIT, WIDE_DELTA, SyncScan, cut_launches, dev, hop_at_width, hop_width, plan_tries, rate_list, sync_launch
from .utils import BAND_PLAN

assert MAX_TRIES == ES_MAX_TRIES
NB = len(BAND_PLAN)
PAIR_BUDGET = 1 << 16           # (key, clip-band) pairs planned per call: the bounded candidate table is 2 000 bytes per pair


@dataclass
class KeyMatch:
    key: int            # index into the identifier's key list
    ctr: int            # frame counter of the accepted candidate
    band: int           # index into BAND_PLAN
    start: int          # peak (sample offset of the frame in the conditioned clip)
    variant: int        # 0..3: +llr0, -llr0, +llr1, -llr1 (rtwm/detector.py:161-190)
    blob: bytes         # the 55 bytes the validator accepted
    plain: bytes        # their 27-byte plaintext


def plan_reference(peaks, npeaks: int, M: int, band: int, hdr_ok, hdr_lo16, hop, pos0: int = 0, ctr0: int = 0, hop_base: int = 0):
    """Host twin of es_plan_batch / es_plan_at_batch for one (key, row): scan.plan_tries on the kernel's inputs.  peaks: the row's
    ES_MAX_PEAKS sync peaks, npeaks: its raw count word, M: samples per record, band: the row's band index, hdr_ok / hdr_lo16: header
    results of the row's fitting peaks in order, hop[ctr - hop_base]: band index of the key's counters (a counter outside the table is
    skipped, as the kernels skip it); pos0: the absolute sample of the row's first sample, ctr0: the counter origin of its stream (DESIGN
    4.18; both 0: the reference's estimate).  -> (plan [(peak slot, ctr)] in try order, fitting peaks looked at)."""
    hop_base, C = int(hop_base), len(hop)
    n = min(int(npeaks) & 0xFFFF, ES_MAX_PEAKS, PEAK_LIMIT)
    slots = [slot for slot in range(n) if 0 <= int(peaks[slot]) <= M - FRAME_LEN]       # the kernel's own filter of the raw peaks
    tries, looked = plan_tries([int(peaks[slot]) for slot in slots], hdr_ok, hdr_lo16,
                               lambda c: 0 <= c - hop_base < C and hop[c - hop_base] == band, pos0, ctr0)
    return [(slots[j], c) for j, cs in tries for c in cs], looked


@dataclass
class _LiveWalk:
    """What WatermarkIdentifier._walk needs of a monitor tick beyond its SyncScan (which says where the frames lie)."""
    w0: np.ndarray              # int64 per scan row: absolute index of the window's first sample
    epoch: np.ndarray           # int64 per scan row: epoch of the row's stream slot
    origin: np.ndarray          # int64 per pushed stream: its counter origin, -1 for none
    window: int                 # samples of the monitor's window: what the hop tables are sized for, whatever the tick's windows hold
    hop: object                 # uint8 [N, hop_width(window)] device: the window's hop table, counters from 0 (streams without an origin)
    hop_at: object              # () -> uint8 [N, 1, hop_at_width(window)] device: the same table as a hop row of es_plan_at_batch
    memo: object                # engine.Memo, or None: every candidate is decoded
    stats: dict                 # planned / decoded / skipped candidates, summed over the walk
    trace: bool                 # record traces (the live identifier's own switch, not its WatermarkIdentifier's)


@dataclass
class _Planned:
    """The plan of one scan under every key: row = clip * 4 + band index, P fitting peaks in (row, peak) order."""
    plan: object                # engine.PlanResult on the device: [N * R, 400] slots and counters in try order
    count: np.ndarray           # int64 [N, R] tries of each (key, row)
    order: np.ndarray           # int64 [N, 4] band index of each key's rank (rtwm/detector.py:46-52)
    log: tuple | None = None    # with traces: (first fitting peak [R], looked [N, R], header ok / value / score [N, P], header-log index [R, 32])


@dataclass
class _Rank:
    """The candidates of one band rank: the tries of every (key, clip) pair still unmatched on the pair's band of that rank, pair by
    pair (keys ascending) in try order.  _h: host arrays; _d: device tensors, None where there is no candidate at all."""
    ks: np.ndarray; cs: np.ndarray; rs: np.ndarray; cnt: np.ndarray          # per pair: key, clip, scan row, tries
    pair_of: np.ndarray; row_h: np.ndarray                                   # per candidate: its pair, its scan row ...
    ctr_h: np.ndarray = None; start_h: np.ndarray = None; yrow_h: np.ndarray = None      # ... counter, peak (relative to the clip or window), a tick's history row
    key_d: object = None; ctr_d: object = None; slot_d: object = None        # int32 key index, int32 counter word, int64 slot of the peak in its row
    yrow_d: object = None; col_d: object = None                              # int32: where the frame lies in sy.y, row and column

    @property
    def total(self) -> int:
        return int(self.pair_of.size)


class WatermarkIdentifier:
    """identify(audio, fs_in) -> one entry per key: a KeyMatch, or None where WatermarkDetector(key).verify would return False.
    With `.trace = True` a call returns (matches, traces), traces[i] = (the `_trace`, the `_hdr_trace`) a fresh detector of key i
    would have recorded."""

    def __init__(self, keys, *, fs_target: int = 48_000, list_size: int = 256, engine=None) -> None:
        self.keys = [bytes(k) for k in keys]
        if any(len(k) != 32 for k in self.keys):
            raise ValueError("master_key must be 32 bytes (256 bit)")
        self.fs_target = fs_target
        self._list_size = int(list_size)
        self.trace = False
        # conditioning, sync and the engine choice are the detector's; its key plays no part in what is used of it
        self._det = WatermarkDetector(self.keys[0] if self.keys else bytes(32), fs_target=fs_target, list_size=list_size, engine=engine)
        self._ring = None

    @property
    def engine(self):
        return self._det.engine

    def _pair_cap(self) -> int:
        return self._det._pair_cap()

    def identify(self, audio, fs_in: int, ctr0: int | None = None):
        res = self.identify_batch([audio], fs_in, None if ctr0 is None else [ctr0])
        return (res[0][0], res[1][0]) if self.trace else res[0]

    def identify_batch(self, clips, fs_in, ctr0=None):
        """identify() for several recordings -> one list of per-key entries per clip (with .trace: (those, per clip the per-key
        traces)).  Clips of one sample type share their launches whatever their lengths (scan.cut_launches).  ctr0: the counter origin
        of every clip, or one per clip with None entries allowed, as for WatermarkDetector.verify_batch."""
        N, clips = len(self.keys), list(clips)
        fs_list = rate_list(fs_in, len(clips))
        origins = clip_origins(ctr0, clips, fs_list, self.fs_target)       # refused by name before any engine exists
        out = [[None] * N for _ in clips]
        traces = [[([], []) for _ in range(N)] for _ in clips]
        if N:
            per_call = max(1, PAIR_BUDGET // (N * NB))
            for la in cut_launches(clips, fs_list, self.fs_target, NB, self._det._conditioned):      # (clips shorter than the template are in none)
                for at in range(0, len(la.idx), per_call):
                    part = la.part(at, at + per_call)                       # conditioning + sync once, whatever the number of keys
                    self._walk(sync_launch(self.engine, part, range(NB)), [out[i] for i in part.idx], [traces[i] for i in part.idx],
                               origins=[origins[i] for i in part.idx])
        return (out, traces) if self.trace else out

    def presence(self, audio, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0):
        return self.presence_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, phases=phases, decoys=decoys,
                                   drift_ppm=drift_ppm)[0]

    def presence_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0) -> list:
        """WatermarkDetector.presence_batch under every key at once -> per clip None (no whole 1215-sample slot) or a list with one
        presence.Presence per key: entry k is field for field what WatermarkDetector(keys[k]).presence_batch gives for the clip.  The
        fold and the hypothesis list are keyless, so the front and the launches are the single detector's, with the ring keys + decoys
        in place of [key] + decoys: entry k has score = key row k and null = the decoy rows.
        Each entry keeps its own bound of 1 / (decoys + 1) on a false alarm.  The chance that SOME key of the N is flagged on unmarked
        audio is bounded by N / (decoys + 1), not 1 / (decoys + 1): ask for decoys accordingly.  Arguments and ValueErrors are
        WatermarkDetector.presence_batch's."""
        return self._det._presence_clips(clips, fs_in, ctr0, span, phases, decoys, drift_ppm, self.keys)

    def presence_map(self, audio, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2,
                     phases: int = 8, decoys: int = 32, drift_ppm=0.0):
        return self.presence_map_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, window=window, step=step, confirm=confirm,
                                       phases=phases, decoys=decoys, drift_ppm=drift_ppm)[0]

    def presence_map_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2, phases: int = 8,
                           decoys: int = 32, drift_ppm=0.0) -> list:
        """WatermarkDetector.presence_map_batch under every key at once -> per clip None (no whole 1215-sample slot) or a list with one
        presence.PresenceMap per key: entry k is field for field what WatermarkDetector(keys[k]).presence_map_batch gives for the clip.
        The windows' folds and lists are keyless, so one front, one fold and one pick serve every key, and one score call covers the
        ring keys + decoys; each key is ranked against the decoys alone, so for N keys the chance that some key's window is detected
        falsely is at most N / (decoys + 1).  Arguments and ValueErrors are WatermarkDetector.presence_map_batch's."""
        return self._det._presence_clips(clips, fs_in, ctr0, span, phases, decoys, drift_ppm, self.keys, grid=(window, step, confirm))

    def presence_coherent(self, audio, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), phases: int = FRAME_LEN, decoys: int = 32):
        return self.presence_coherent_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, phases=phases, decoys=decoys)[0]

    def presence_coherent_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), phases: int = FRAME_LEN, decoys: int = 32) -> list:
        """WatermarkDetector.presence_coherent_batch under every key at once -> per clip None (no whole slot) or a list with one
        presence.Presence per key: entry k is field for field what WatermarkDetector(keys[k]).presence_coherent_batch gives for the clip.
        The matched-filter rows are keyless, so the front and the launches are the single detector's, with the ring keys + decoys in
        place of [key] + decoys: entry k has score = key row k and null = the decoy rows.  Each entry keeps its own bound
        of 1 / (decoys + 1) on a false alarm; the chance that SOME key of the N is flagged on unmarked audio is bounded by
        N / (decoys + 1), not 1 / (decoys + 1): ask for decoys accordingly.  Arguments and ValueErrors are
        WatermarkDetector.presence_coherent_batch's."""
        return self._det._presence_coherent_clips(clips, fs_in, ctr0, span, phases, decoys, self.keys)

    def presence_coherent_map(self, audio, fs_in: int, ctr0: int | None = None, *, span=(0, 4096), window: int = 40, step: int = 20,
                              confirm: int = 2, decoys: int = 32):
        return self.presence_coherent_map_batch([audio], fs_in, None if ctr0 is None else [ctr0], span=span, window=window, step=step,
                                                confirm=confirm, decoys=decoys)[0]

    def presence_coherent_map_batch(self, clips, fs_in, ctr0=None, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2,
                                    decoys: int = 32) -> list:
        """WatermarkDetector.presence_coherent_map_batch under every key at once -> per clip None (no whole slot) or a list with one
        presence.PresenceMap per key: entry k is field for field what WatermarkDetector(keys[k]).presence_coherent_map_batch gives for
        the clip.  One front, one mf_rows and one score call per group of windows and span width cover the ring keys + decoys; each key
        is ranked against the decoys alone, so for N keys the chance that some key's window is detected falsely is at most
        N / (decoys + 1).  Arguments and ValueErrors are WatermarkDetector.presence_coherent_map_batch's."""
        return self._det._presence_coherent_clips(clips, fs_in, ctr0, span, FRAME_LEN, decoys, self.keys, grid=(window, step, confirm))

    def open_streams(self, n: int, *, fs=None, window_s: float = 5.0, chunk_max: int | None = None, trace: bool = False,
                     memo_slots: int | None = None, ctr0=None) -> "LiveIdentifier":
        """A monitor of n live streams that says, per push and stream, which of this identifier's keys marks the stream's last window_s
        seconds (LiveIdentifier.push).  fs, window_s, chunk_max and trace are those of WatermarkDetector.open_streams.  memo_slots:
        entries of the verdict memo, a power of two; 0: no memo, every push decodes its whole window; None:
        memo.default_slots -- the next power of two above 2 x keys x 4 n x 400, between 2^10 and 2^25 entries of 20 bytes each (16 keys
        and 64 streams: 2^22 entries, 80 MiB; never more than 640 MiB).  ctr0: the counter origin of every stream, or one per stream
        with None entries allowed, as for WatermarkDetector.open_streams."""
        from .monitor import open_arguments, origin_words
        how = open_arguments(n, self.fs_target, bands=tuple(range(NB)), fs=fs, window_s=window_s, chunk_max=chunk_max, ctr0=ctr0)      # refuses before any engine exists
        slots = memo.default_slots(len(self.keys), int(n)) if memo_slots is None else int(memo_slots)
        LiveIdentifier.check_memo(slots, len(self.keys), how["window"], bool((origin_words(ctr0, int(n)) < 0).any()))     # ... and so is what the memo's records cannot name
        return LiveIdentifier(self, self.engine.open_monitor(int(n), **how), trace=trace, memo_slots=slots)

    # ------------------------------------------------------------------ after the sync: the walk of one scan, in stages
    def _keyring(self):
        if self._ring is None or self._ring.ring.device != self.engine.device:
            self._ring = self.engine.keyring(self.keys)
        return self._ring

    def _hop_table(self, C: int):
        """uint8 [N, C] on the device: band of (key, counter) for the counters 0 .. C - 1."""
        import torch
        eng, N = self.engine, len(self.keys)
        kk = torch.arange(N, dtype=torch.int32, device=eng.device).repeat_interleave(C)
        cc = torch.arange(C, dtype=torch.int64, device=eng.device).repeat(N)
        return eng.schedule_keyed(self._keyring(), kk, cc, want_pn=False)[1].reshape(N, C)

    def _walk(self, scan, out, traces, live: "_LiveWalk | None" = None, origins=None) -> None:
        """Everything after the sync, for the clips of one SyncScan: header decode per (key, fitting peak), hop table, plan, rank loop,
        final check.  live: the scan is a monitor tick's (SyncScan.from_monitor) -- frames are read in place in the history rows, row
        lengths are the windows', and candidates the memo knows to fail are not decoded again.  origins: per clip its counter origin
        or None (a tick's are live.origin): with any, the plan is es_plan_at_batch's over one hop row per distinct window base."""
        N, g = len(self.keys), len(scan.sizes)
        self._keyring()
        if not scan.rows.size:                                              # no peak can hold a frame: nothing to try for any key
            return
        if live is not None:
            origin, tracing = live.origin, live.trace
        else:
            origin, tracing = np.array([-1 if o is None else o for o in origins or [None] * g], np.int64), self.trace
        pl = self._plan(scan, self._headers(scan), origin, live, tracing)
        alive = np.ones((N, g), bool)
        found: list = []                                                    # (key, clip, ctr, band, start, variant, blob row)
        for rank in range(NB):
            ks, cs = np.nonzero(alive)                                      # key-major: candidates arrive sorted by key
            if not ks.size:
                break
            c = self._candidates(scan, pl, ks, cs, rank)
            first = np.full(ks.size, -1, np.int64)                          # per pair: its first validated candidate (index into the flat list)
            if c.total:
                todo, keys = (np.arange(c.total), None) if live is None else self._unknown(c, origin, live)      # a tick decodes what its memo does not know
                ok, blobs = self._decode(scan.sy.y, c, todo)
                if keys is not None and todo.size:
                    # what was decoded and failed in all four variants is remembered: ONE insert per rank, the rest masked out
                    self.engine.memo_insert(live.memo, np.where((ok[todo] == 0).all(axis=1), keys[0][todo], memo.EMPTY), keys[1][todo])
                hits = np.flatnonzero((ok == 1).any(axis=1))
                if hits.size:
                    pairs, where = np.unique(c.pair_of[hits], return_index=True)    # hits ascend: the first hit of each pair
                    first[pairs] = hits[where]
                for p in np.flatnonzero(first >= 0):
                    i = int(first[p])
                    found.append((int(ks[p]), int(cs[p]), int(c.ctr_h[i]), int(pl.order[ks[p], rank]), int(c.start_h[i]), *blobs[i]))
            if tracing:
                self._trace_rank(pl, c, first, rank, traces)
            alive[ks[first >= 0], cs[first >= 0]] = False                   # keys that matched leave before the next rank
        self._confirm(found, out)

    def _headers(self, scan):
        """One header decode over (key, fitting peak), key-major, each key with its own header PN -> (ok, low 16 bits, score) [N * P]."""
        eng, N = self.engine, len(self.keys)
        return eng.header(scan.sy.y, dev(eng, np.tile(scan.rows % NB, N), np.uint8), self._keyring().hdr_pn.repeat_interleave(scan.rows.size, dim=0),
                          rows=dev(eng, np.tile(scan.frame_rows, N), np.int32), start=dev(eng, np.tile(scan.frame_cols, N), np.int32))

    def _plan(self, scan, hdr, origin, live, tracing) -> _Planned:
        """The tries of every (key, row), planned on the device from the header results `hdr`, with their counts on the host."""
        import torch
        eng, ring, sy = self.engine, self._keyring(), scan.sy
        N, g, P = len(self.keys), len(scan.sizes), scan.rows.size
        R = g * NB                                                          # sync rows: row = clip * 4 + band index
        sizes = np.array(scan.sizes, np.int32)
        M = int(sizes.max())                                                # the longest clip: row length of the sync call
        M_rows = np.repeat(sizes, NB)                                       # samples of each sync row's own clip
        base = np.searchsorted(scan.rows, np.arange(R)).astype(np.int32)
        rowband = np.tile(np.arange(NB, dtype=np.uint8), g)
        hdr_at = (hdr[0].reshape(N, P), hdr[1].reshape(N, P))
        absolute = origin >= 0                                              # per clip
        if live is None:            # a clip starts at sample 0; hop tables for the longest clip, built here
            span, w0, table, row0 = M, np.zeros(g, np.int64), lambda: self._hop_table(hop_width(M)), None
            T = M if int(sizes.min()) == M else M_rows                      # (equally long rows have a planning kernel of their own)
        else:                       # a window starts at w0; hop tables for the monitor's window, built once by the live identifier
            span, w0, table, row0, T = live.window, live.w0[::NB], lambda: live.hop, live.hop_at, M_rows
        if not absolute.any():      # counters from 0: the hop table of the relative estimates
            plan = eng.plan(sy.peaks, sy.npeaks, rowband, base, T, *hdr_at, table())
        else:
            # a clip with an origin starts at sample pos0 (a window's w0; 0 for a clip) of a stream marked from that
            # counter; one without keeps estimates relative to its first sample, which is origin 0 at pos0 0.  One hop row per
            # distinct base, filled on the device; the row of base 0 is the hop table of clips without origins.
            pos0, ctr0 = np.where(absolute, w0, 0).astype(np.int64), np.where(absolute, origin, 0)
            row_base = np.maximum(0, ctr0 + (2 * pos0 + FRAME_LEN) // (2 * FRAME_LEN) - WIDE_DELTA)
            bases, hop_row = np.unique(row_base, return_inverse=True)
            if row0 is not None and bases[0] == 0:                          # counters from 0: the window's own table, built once
                hop = torch.cat((row0(), eng.hop_window(ring, bases[1:], hop_at_width(span))), dim=1)
            else:
                hop = eng.hop_window(ring, bases, hop_at_width(span))
            plan = eng.plan(sy.peaks, sy.npeaks, rowband, base, M_rows, *hdr_at, hop, pos0=np.repeat(pos0, NB), ctr0=np.repeat(ctr0, NB),
                            hop_row=np.repeat(hop_row.reshape(-1), NB), hop_base=bases)
        count = plan.count.cpu().numpy().astype(np.int64).reshape(N, R)
        hop0 = ring.hop0.cpu().numpy().astype(np.int64)
        order = np.array([[h] + [b for b in range(NB) if b != h] for h in range(NB)], np.int64)[hop0]      # [N, 4]: rtwm/detector.py:46-52
        pl, pk_h = _Planned(plan, count, order), sy.peaks.cpu().numpy()             # (the peaks' copy is made with or without traces)
        if tracing:
            looked = plan.looked.cpu().numpy().reshape(N, R)
            hdr_h = (hdr[0].cpu().numpy().reshape(N, P), hdr[1].cpu().numpy().reshape(N, P), hdr[2].cpu().numpy().astype(np.float64).reshape(N, P))
            fit = (pk_h >= 0) & (pk_h + FRAME_LEN <= M_rows[:, None]) & (np.arange(ES_MAX_PEAKS)[None, :] < np.minimum(sy.npeaks.cpu().numpy() & 0xFFFF, PEAK_LIMIT)[:, None])
            pl.log = (base, looked, hdr_h, np.cumsum(fit, axis=1) - 1)
        return pl

    def _candidates(self, scan, pl: _Planned, ks, cs, rank: int) -> _Rank:
        """The candidates of band rank `rank` for the pairs (ks[p], cs[p]), gathered from the plan on the device."""
        import torch
        eng, R = self.engine, pl.count.shape[1]
        rs = cs * NB + pl.order[ks, rank]
        cnt = pl.count[ks, rs]
        pair_of = np.repeat(np.arange(ks.size), cnt)
        c = _Rank(ks, cs, rs, cnt, pair_of, rs[pair_of])
        if c.total:
            pos = np.arange(c.total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            flat = dev(eng, (ks[pair_of] * R + c.row_h) * ES_MAX_TRIES + pos, np.int64)
            c.ctr_d = pl.plan.ctr.reshape(-1)[flat]
            c.slot_d = pl.plan.slot.reshape(-1)[flat].to(torch.int64)
            row_d = dev(eng, c.row_h, np.int64)
            start_d = scan.sy.peaks.reshape(-1)[row_d * ES_MAX_PEAKS + c.slot_d]
            c.key_d = dev(eng, ks[pair_of], np.int32)
            c.ctr_h = c.ctr_d.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            c.start_h = start_d.cpu().numpy().astype(np.int64)
            if scan.yrows is None:                                          # frames at sy.y[row, start] ...
                c.yrow_d, c.col_d = row_d.to(torch.int32), start_d
            else:                                                           # ... or in place in a tick's history: row 4 s + j, column offset + start
                c.yrow_h = scan.sy.rows[c.row_h]
                c.yrow_d, c.col_d = dev(eng, c.yrow_h, np.int32), dev(eng, scan.sy.offset[c.row_h] + c.start_h, np.int32)
        return c

    def _unknown(self, c: _Rank, origin, live: _LiveWalk):
        """The memo filter -> (the candidates no earlier push is known to have decoded in vain, the memo records (k0, k1) of all of
        them or None without a memo); counted in live.stats."""
        todo, keys = np.arange(c.total), None
        if live.memo is not None:
            a_h = live.w0[c.row_h] + c.start_h                              # absolute start
            org = origin[c.row_h // NB]                                     # a stream with an origin: counter relative to its peak's estimate
            field = np.where(org >= 0, c.ctr_h - (org + (2 * a_h + FRAME_LEN) // (2 * FRAME_LEN)) + WIDE_DELTA, c.ctr_h)
            k0, k1 = np.empty(c.total, np.uint64), np.empty(c.total, np.uint64)
            for sel, pack in ((org < 0, memo.pack), (org >= 0, memo.pack_abs)):
                if sel.any():
                    k0[sel], k1[sel] = pack(c.ks[c.pair_of][sel], c.yrow_h[sel], live.epoch[c.row_h][sel], a_h[sel], field[sel])
            keys = (k0, k1)
            k0_d, k1_d = dev(self.engine, k0.view(np.int64), np.int64), dev(self.engine, k1.view(np.int64), np.int64)
            todo = np.flatnonzero(self.engine.memo_probe(live.memo, k0_d, k1_d).cpu().numpy() == 0)
        for what, n in (("planned", c.total), ("decoded", todo.size), ("skipped", c.total - todo.size)):
            live.stats[what] += int(n)
        return todo, keys

    def _decode(self, y, c: _Rank, todo: np.ndarray):
        """Decode candidates `todo` of a rank in chunks of _pair_cap() -> (int8 [total, 4]: 1 where a variant validated under the
        candidate's key -- a candidate that is not decoded is a known failure --, {candidate: (first such variant, its blob)})."""
        eng, ring, cap = self.engine, self._keyring(), max(1, int(self._pair_cap()))
        ok_all, blobs = np.zeros((c.total, 4), np.int8), {}
        for a in range(0, todo.size, cap):
            sel = todo[a:a + cap]
            n = sel.size
            sel_d = dev(eng, sel, np.int64)
            rows, cols, key, ctr = c.yrow_d[sel_d], c.col_d[sel_d], c.key_d[sel_d], c.ctr_d[sel_d]
            pn, bands = eng.schedule_keyed(ring, key, ctr)
            res = decode_four(eng, y, rows, cols, pn, bands, self._list_size)
            payload, ok, _which = eng.select(res, ring=ring, key_idx=key.repeat(4), ctrs=ctr.repeat(4))
            okc = check_decoded(ok.cpu().numpy()).reshape(4, n).T
            ok_all[sel] = okc
            hit = np.flatnonzero((okc == 1).any(axis=1))
            if hit.size:
                v = np.argmax(okc[hit] == 1, axis=1)                        # the first of +llr0, -llr0, +llr1, -llr1 that validates
                got = payload[dev(eng, v * n + hit, np.int64)].cpu().numpy()
                for i, vv, row in zip(hit, v, got):
                    blobs[int(sel[i])] = (int(vv), row)
        return ok_all, blobs

    def _trace_rank(self, pl: _Planned, c: _Rank, first, rank: int, traces) -> None:
        """traces[clip][key] += what a fresh detector of the key records on this band: tries up to the accepted one, headers looked at."""
        base, looked, hdr_h, fit_rank = pl.log
        off = np.cumsum(c.cnt) - c.cnt
        slot_h = c.slot_d.cpu().numpy() if c.total else None
        for p in range(c.ks.size):
            k, r = int(c.ks[p]), int(c.rs[p])
            tr, ht = traces[int(c.cs[p])][k]
            lo = int(BAND_PLAN[pl.order[k, rank]][0])
            end = int(first[p]) + 1 if first[p] >= 0 else int(off[p] + c.cnt[p])
            tr.extend((lo, int(c.start_h[i]), int(c.ctr_h[i])) for i in range(int(off[p]), end))
            # the reference decodes a peak's header when it reaches the peak: peaks after the accepted one were never looked at
            n = int(fit_rank[r, slot_h[first[p]]]) + 1 if first[p] >= 0 else int(looked[k, r])
            j = k, slice(int(base[r]), int(base[r]) + n)
            ht.extend((float(bool(a)), float(b), float(s)) for a, b, s in zip(hdr_h[0][j], hdr_h[1][j], hdr_h[2][j]))

    def _confirm(self, found: list, out) -> None:
        """The final check: the plaintexts of the accepted candidates from ONE keyed AEAD call -> out[clip][key] = the KeyMatch."""
        import torch
        if not found:
            return
        eng = self.engine
        ok, plain = eng.aead_check_keyed(self._keyring(), dev(eng, [f[0] for f in found], np.int64), dev(eng, np.stack([f[6] for f in found]), np.uint8),
                                         torch.tensor([f[2] for f in found], dtype=torch.int64), want_plain=True)
        for f, o, pt in zip(found, ok.cpu().numpy(), plain.cpu().numpy()):
            if o != 1:
                raise NativeError("es_select_keyed_batch accepted a blob that es_aead_check_keyed_batch rejects")
            out[f[1]][f[0]] = KeyMatch(f[0], f[2], f[3], f[4], f[5], f[6].tobytes(), pt.tobytes())


class LiveIdentifier(LiveTable):
    """The monitored streams of a WatermarkIdentifier (WatermarkIdentifier.open_streams); stream ids are the slots of `table`.

    After a push, entry k of stream s is what WatermarkIdentifier.identify gives for key k on the stream's window [w0, n): while
    w0 == 0 exactly identify(everything received so far, fs_target), afterwards the identifier's walk over the scan of the contiguous
    slice y_whole[:, w0 : n] of the whole stream's band-pass -- same boolean, same tries in the same order, same accepted blob, with
    KeyMatch.start relative to the window.  Every push is stateless per key, as identify is.  A stream opened at another rate is
    conditioned on the device first, as for LiveMonitor.

    What differs is the work.  The band-pass and the correlation are continued from push to push by the monitor table,
    and a candidate (key, band row, absolute position, counter) that failed once is remembered in a memo on the device: its verdict
    depends on nothing else, and the history it read is bit-identical from push to push, so a tick decodes only candidates it has never
    decoded.  `stats` counts the candidates of the last push: planned = decoded + skipped."""

    def __init__(self, identifier: WatermarkIdentifier, table, *, trace: bool = False, memo_slots: int = 0) -> None:
        self._id, self.table, self._trace = identifier, table, bool(trace)
        self.check_memo(memo_slots, len(identifier.keys), table.window, bool((table.origin_host < 0).any()))
        self.memo_slots = int(memo_slots)
        self._memo = None                                                   # engine.Memo, opened by the first push that needs it
        self._hop = None                                                    # the window's hop table, built by the first push
        self._hop_at = None                                                 # the same as a hop row of es_plan_at_batch, built when first needed
        self._epoch = np.zeros(table.n, np.int64)                           # times each stream slot has been closed, mod 2^16
        self.stats = {"planned": 0, "decoded": 0, "skipped": 0}

    @staticmethod
    def check_memo(slots: int, n_keys: int, window: int, relative: bool = True) -> None:
        """Refuse what the memo's records cannot name: they hold 20 bits of key index and 16 of counter.  relative: some stream has
        no counter origin -- its records hold the counter itself; one with an origin holds 0 .. 400 whatever the window."""
        if not slots:
            return
        memo.check_slots(slots)
        if n_keys > memo.MAX_KEYS:
            raise ValueError(f"{n_keys} keys: a live identifier with a memo takes at most {memo.MAX_KEYS} keys (memo_slots=0 takes any number)")
        C = hop_width(window)
        if relative and C > memo.MAX_COUNTERS:
            raise ValueError(f"window of {int(window)} samples: its candidates reach counter ceil(window / 1215) + 200 = {C - 1}, the memo's records "
                             f"hold counters below {memo.MAX_COUNTERS} (use a shorter window_s, memo_slots=0, or give every stream its counter origin ctr0)")

    @property
    def fs_target(self) -> int:
        return self._id.fs_target

    @property
    def engine(self):
        return self._id.engine

    def push(self, chunks, streams=None, *, fs: int | None = None):
        """chunks[i], 1-D int16 or float32 at the rate its stream was opened with, continues stream streams[i] (None: one chunk per open
        stream, in order) -> per chunk a list of len(keys) entries, a KeyMatch or None; with trace=True (matches, traces) as
        identify_batch returns them.  Streams not named are not touched.  Raises ValueError before any GPU work for what
        LiveMonitor.push refuses, and for a stream that would pass 2^48 samples while the memo is on.  A stream with a counter origin
        (origin(stream)) is planned from absolute positions: pos0 = w0 and its origin; its hop row is rebuilt on the device each push."""
        from .monitor import push_arguments
        tab, N = self.table, len(self._id.keys)
        ids, arrs, lengths = push_arguments(tab, self.fs_target, chunks, streams, fs)
        if self.memo_slots and ids.size and (tab.n_host[ids] + lengths).max() > memo.MAX_POSITION:
            bad = int(ids[int((tab.n_host[ids] + lengths).argmax())])
            raise ValueError(f"stream {bad} would pass 2^48 samples: the memo's records hold absolute positions below that (close the stream "
                             "and open it again, or use memo_slots=0)")
        out = [[None] * N for _ in ids]
        traces = [[([], []) for _ in range(N)] for _ in ids]
        self.stats = {"planned": 0, "decoded": 0, "skipped": 0}
        if ids.size and N:
            eng = self.engine
            if self.memo_slots and self._memo is None:
                self._memo = eng.open_memo(self.memo_slots)
            if self._hop is None and (tab.origin_host[ids] < 0).any():      # depends on the keys and the window alone (streams without an origin)
                self._hop = self._id._hop_table(hop_width(tab.window))
            tick = eng.monitor_step(tab, ids, arrs)
            per_call = max(1, PAIR_BUDGET // (N * NB))                      # cut as identify_batch cuts its clips
            for a in range(0, ids.size, per_call):
                part = tick.part(a, a + per_call)
                s_rows = np.repeat(part.sid, NB)                            # the stream of each scan row
                live = _LiveWalk(tab.base_host[s_rows] + part.offset, self._epoch[s_rows], tab.origin_host[part.sid], tab.window,
                                 self._hop, self._hop_row0, self._memo, self.stats, self._trace)
                self._id._walk(SyncScan.from_monitor(part), out[a:a + per_call], traces[a:a + per_call], live)
        elif ids.size:
            self.engine.monitor_step(tab, ids, arrs)                        # no key: the streams still move on
        return (out, traces) if self._trace else out

    def presence(self, streams=None, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0) -> list:
        """LiveMonitor.presence under every key at once -> per stream None (no whole slot in its window) or a list with one
        presence.Presence per key: entry k is field for field what a LiveMonitor of key k gives on the same table.  The ring is
        keys + decoys, entry k has score = key row k and null = the decoy rows; one fold launch and one score launch per group of
        equal span width cover all streams and all keys.  With N keys the chance that SOME key is flagged on unmarked
        audio is bounded by N / (decoys + 1), not 1 / (decoys + 1): ask for decoys accordingly.  Nothing is pushed, and neither the
        table, the memo, the stats nor any origin is touched: the verdict is statistical and never sets a stream's origin.
        ValueError before any GPU work, as for LiveMonitor.presence."""
        return self._presence(self._id._det, self._id.keys, streams, span, phases, decoys, drift_ppm)

    def _hop_row0(self):
        """The window's hop table (counters from 0) at the width es_plan_at_batch asks for, as its hop row: depends on the keys and the
        window alone, built by the first push that mixes streams with and without an origin."""
        if self._hop_at is None:
            self._hop_at = self.engine.hop_window(self._id._keyring(), [0], hop_at_width(self.table.window))
        return self._hop_at

    def forget(self) -> None:
        """Empty the memo: the next push of every stream decodes its whole window again."""
        if self._memo is not None:
            self._memo.table.fill_(-1)

    def add(self, n: int = 1, fs=None, ctr0=None) -> np.ndarray:
        """LiveTable.add; streams without an origin (ctr0 None) are refused where the memo's records cannot hold the window's counters."""
        from .monitor import origin_words
        self.check_memo(self.memo_slots, len(self._id.keys), self.table.window, bool((origin_words(ctr0, int(n)) < 0).any()))
        return super().add(n, fs, ctr0)

    def _slots_changed(self, ids, closed: bool) -> None:
        """Slots the table grew by start at epoch 0; a closed slot's moves on, so that whoever opens it next never meets this stream's
        verdicts, and when an epoch wraps the whole memo is emptied."""
        self._epoch = np.concatenate((self._epoch, np.zeros(self.table.n - self._epoch.size, np.int64)))
        if closed and memo.bump_epochs(self._epoch, ids):
            self.forget()


__all__ = ["KeyMatch", "LiveIdentifier", "WatermarkIdentifier", "plan_reference"]
