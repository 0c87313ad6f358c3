"""The receive side of live streams: a monitor table on the device and one tick of it.

A monitor holds S stream slots at the engine's rate, a window of W samples and a longest chunk.  Stream s has received n samples X
since it was opened; per band y = lfilter(b, a, X) from zero state at the opening, never restarted, and corr is the normalised
correlation of that y at absolute lags 0 <= i < n - 62.  The table keeps the recent part of both in linear rows of H columns (absolute
index a at column a - base, base a multiple of 1216) together with the band-pass's eight delay elements per (stream, band).  After a
push the window is [w0, n), w0 = 1216 * ceil(max(0, n - W) / 1216): 1216 = 64 * 19 is the correlation kernel's segment, and a window that
starts at a multiple of 19 sees exactly the correlation values the stream already has, so nothing is ever computed twice.

`monitor_layout` (where a tick's chunks go, and when rows are moved down) and the argument checks are host functions that need no
engine; `MonitorChain` is the part of RxEngine that owns the table and launches a tick (es_bpf_stream_batch -> es_xcorr_stream_batch ->
es_pick_at_batch).

Streams at other rates: a slot has a rate of its own, fixed when it is opened; its chunks are conditioned on the device
(es_resample_stream_batch) to the finalized prefix of resample_poly over the whole stream, and everything above holds with that
conditioned stream in place of X.  `ResamplerTable` is that state (rates, filters, tails, samples received), usable on its own.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native as nat

SEG = nat.ES_XC_SEG                  # 1216: lags per segment of the correlation kernel; windows and row bases lie on this grid
PRE_L = nat.ES_PRE_L
MIN_WINDOW = 2 * SEG


def window_start(n, window: int):
    """w0 of the window [w0, n) of a stream that has received n samples: 1216 * ceil(max(0, n - W) / 1216) (scalars or arrays)."""
    over = np.maximum(np.asarray(n, dtype=np.int64) - int(window), 0)
    return (over + SEG - 1) // SEG * SEG


def history_columns(window: int, chunk_max: int) -> int:
    """The fewest columns a history row needs: the window, a segment of slack for its grid and one longest chunk."""
    return int(window) + SEG + int(chunk_max)


def check_geometry(window: int, chunk_max: int, hist: int | None = None) -> int:
    """Refuse a monitor that cannot work -> H, the columns of a history row."""
    window, chunk_max = int(window), int(chunk_max)
    if window < MIN_WINDOW:
        raise ValueError(f"window of {window} samples: a monitor window holds at least {MIN_WINDOW} samples (two correlation segments, "
                         "so that a whole 1215-sample frame always fits behind the window's start grid); use a longer window_s")
    if chunk_max < 1:
        raise ValueError("chunk_max must be at least 1 sample")
    need = history_columns(window, chunk_max)
    hist = need if hist is None else int(hist)
    if hist < need:
        raise ValueError(f"history rows of {hist} columns: window + 1216 + chunk_max = {need} are needed")
    if 4 * hist >= 2 ** 31:
        raise ValueError("history rows of 2^29 columns or more are not supported")
    return hist


@dataclass
class ResamplerTable:
    """The resampling state of S live streams (RxEngine.open_resampler; a MonitorTable with rates holds one as `rs`).  Stream s arrives at
    fs[s] and is conditioned to fs_target: rate_host[s] = (up, down, offset of its filter in the pool, taps per phase, y0), the words
    es_resample_stream_batch reads; a stream at fs_target has (1, 1, 0, 0, 0) and is copied.  In a monitor the chunks of streams at
    fs_target go straight to the band-pass, never through the resampling kernels: there the device `tail` and `nin` are kept for the
    other-rate slots only (an at-rate slot's stay +0.0 and 0; n_in_host counts for every slot).  A table of RxEngine.open_resampler
    keeps them for every stream."""
    fs_target: int
    fs: np.ndarray             # [S] int64 rate of each stream
    rate_host: np.ndarray      # [S, 5] int64
    filters: np.ndarray        # float32 pool, one copy per distinct rate
    n_in_host: np.ndarray      # [S] int64 samples received at the stream's own rate (host mirror of nin)
    offsets: dict              # rate -> (up, down, filter offset, hpp, y0)
    rate: object = None        # [S, 5] int64 device
    filt: object = None        # float32 device
    tail: object = None        # [S, 256] float32 device: the last 256 samples received, newest last (the kernel reads the newest 255)
    nin: object = None         # [S] int64 device

    @property
    def n(self) -> int:
        return int(self.fs.size)


def stream_rates(n_streams: int, fs, fs_target: int) -> np.ndarray:
    """`fs` (None: every stream at fs_target; one rate; or one per stream) as int64 [n_streams], each rate checked by
    utils.stream_geometry (integers only, no filter is designed).  A ValueError names what is refused; nothing is changed."""
    S, fs_target = int(n_streams), int(fs_target)
    if fs is None:
        return np.full(S, fs_target, np.int64)
    if np.ndim(fs) == 0:
        fs = [fs] * S
    rates = [int(f) for f in fs]
    if len(rates) != S:
        raise ValueError(f"fs names {len(rates)} rates for {S} streams: give one rate, or one per stream")
    from .utils import stream_geometry
    for f in sorted(set(rates)):
        stream_geometry(f, fs_target)
    return np.asarray(rates, np.int64).reshape(S)


def resampler_extend(rt: ResamplerTable, fs) -> None:
    """Append streams at rates `fs` to the host half of rt: a rate not seen before adds its filter to the pool (designed once)."""
    from .utils import stream_resample_plan
    rows = []
    for f in (int(v) for v in fs):
        if f not in rt.offsets:
            pl = stream_resample_plan(f, rt.fs_target)                      # refuses by name
            rt.offsets[f] = (pl.up, pl.down, int(rt.filters.size) if pl.hpp else 0, pl.hpp, pl.y0)
            rt.filters = np.concatenate((rt.filters, pl.h_tf))
        rows.append(rt.offsets[f])
    rt.rate_host = np.concatenate((rt.rate_host, np.asarray(rows, np.int64).reshape(-1, nat.ES_RSTREAM_RATE_WORDS)))
    rt.fs = np.concatenate((rt.fs, np.asarray(list(fs), np.int64).reshape(-1)))
    rt.n_in_host = np.concatenate((rt.n_in_host, np.zeros(len(rows), np.int64)))


def resampler_host(fs_list, fs_target: int) -> ResamplerTable:
    """The host half of a resampler table for streams at rates fs_list, checked; RxEngine.open_resampler adds the device arrays."""
    fs_target = int(fs_target)
    if fs_target < 1:
        raise ValueError("fs_target must be positive")
    rt = ResamplerTable(fs_target, np.zeros(0, np.int64), np.zeros((0, nat.ES_RSTREAM_RATE_WORDS), np.int64), np.zeros(0, np.float32),
                        np.zeros(0, np.int64), {})
    resampler_extend(rt, np.asarray(fs_list, np.int64).reshape(-1))
    return rt


def resample_counts(rt: ResamplerTable, ids: np.ndarray, lengths: np.ndarray):
    """-> (F(n_old), outputs finalized) int64 per chunk of `lengths` samples pushed to streams `ids`, from the host mirror alone.  A
    position at which n * up would pass 2^62 is refused."""
    from .utils import finalized, stream_position_limit
    f_old, cnt = np.zeros(ids.size, np.int64), np.zeros(ids.size, np.int64)
    for i, (s, ln) in enumerate(zip(ids.tolist(), lengths.tolist())):
        up, down, _, _, y0 = (int(v) for v in rt.rate_host[s])
        n_old = int(rt.n_in_host[s])
        if n_old + ln > stream_position_limit(up):
            raise ValueError(f"stream {s} at {int(rt.fs[s])} Hz: position {n_old + ln} times up = {up} passes 2^62")
        f_old[i] = finalized(n_old, up, down, y0) if up != down else n_old
        cnt[i] = (finalized(n_old + ln, up, down, y0) if up != down else n_old + ln) - f_old[i]
    return f_old, cnt


@dataclass
class MonitorLayout:
    """Where one tick's chunks go (monitor_layout); one entry per pushed stream."""
    move: np.ndarray           # int64 columns the stream's rows are moved down before the chunk is appended (0, or a multiple of 1216)
    base: np.ndarray           # int64 absolute index of column 0 after that move
    col: np.ndarray            # int64 column the chunk is appended at: n_old - base
    n: np.ndarray              # int64 samples received after the chunk
    w0: np.ndarray             # int64 start of the window after the chunk (absolute)


def monitor_layout(n_old, base, lengths, window: int, hist: int) -> MonitorLayout:
    """Lay out one tick.  A chunk is appended at column n_old - base.  Only when it would not fit (column + length > hist) are the rows
    moved down first, to the new base min(w0, 1216 * floor(max(0, n_old - 62) / 1216)) with w0 the window start AFTER the chunk: the
    window's samples and lags stay, and so do the 62 samples before the chunk that its first new lags read.  hist >= window + 1216 +
    chunk_max makes that room for any chunk, and leaves hist - window room after a move, so moves are rare.  A pure host function."""
    n_old = np.asarray(n_old, dtype=np.int64).reshape(-1)
    base = np.asarray(base, dtype=np.int64).reshape(-1)
    ln = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if not (n_old.shape == base.shape == ln.shape):
        raise ValueError("n_old, base, lengths: one entry per chunk")
    if ln.size and ln.min() < 0:
        raise ValueError("negative chunk length")
    n = n_old + ln
    w0 = window_start(n, window)
    full = (n_old - base) + ln > hist
    keep_from = np.minimum(w0, np.maximum(n_old - (PRE_L - 1), 0) // SEG * SEG)
    new_base = np.where(full, np.maximum(base, keep_from), base)
    if ln.size and (n - new_base).max() > hist:
        raise ValueError(f"a chunk does not fit its history row of {hist} columns (longer than the chunk_max the monitor was opened with?)")
    return MonitorLayout(new_base - base, new_base, n_old - new_base, n, w0)


@dataclass
class MonitorTable:
    """The state of S monitored streams (RxEngine.open_monitor); RxEngine.monitor_step pushes chunks to any of them.  Row 4 s + j of
    the device arrays belongs to stream s and band bands[j]."""
    window: int
    chunk_max: int
    hist: int                  # H, columns of a history row
    bands: np.ndarray          # [4] uint8 band of row j of every stream
    n_host: np.ndarray         # [S] int64 samples received (host mirror of pos[:, 0])
    base_host: np.ndarray      # [S] int64 absolute index of column 0 (host mirror of pos[:, 1])
    live: np.ndarray           # [S] bool; False: a closed slot, free for add_monitor_streams
    band: object = None        # [4 S] uint8 device
    z: object = None           # [4 S, 8] float64 device: the band-pass's delay elements
    pos: object = None         # [S, 2] int64 device: (n, base)
    y_hist: object = None      # [4 S, H] float64 device
    corr_hist: object = None   # [4 S, H] float64 device
    fs_target: int = 0         # the rate the streams are conditioned to (0: not stated -- every stream arrives at it)
    rs: ResamplerTable | None = None        # rates, filters, tails and samples received of streams at other rates (None: all at fs_target)
    origin_host: np.ndarray | None = None   # [S] int64 counter origin of each stream; -1: none, counters relative to the window

    @property
    def fs(self) -> np.ndarray:
        """[S] int64 rate of each stream (fs_target where none was given)."""
        return np.full(self.n, self.fs_target, np.int64) if self.rs is None else self.rs.fs

    @property
    def n_in_host(self) -> np.ndarray:
        """[S] int64 samples received at the stream's own rate (n_host is the conditioned position)."""
        return self.n_host if self.rs is None else self.rs.n_in_host

    @property
    def n(self) -> int:
        return int(self.live.size)


def origin_words(ctr0, n: int) -> np.ndarray:
    """Counter origins (scan.counter_origins: None, one, or one per stream; checked) as the table holds them: int64 [n], -1 for None."""
    from .scan import counter_origins
    return np.array([-1 if v is None else v for v in counter_origins(ctr0, n, "stream")], np.int64).reshape(int(n))


def origin_keywords(ctr0) -> dict:           # ctr0 as the keyword of open_monitor / add_monitor_streams; no origin: the call as it always was
    return {} if ctr0 is None else {"ctr0": ctr0}


def open_arguments(n: int, fs_target: int, *, bands, fs=None, window_s: float = 5.0, chunk_max: int | None = None, ctr0=None) -> dict:
    """What both open_streams do before an engine is touched: window_s and chunk_max (default half a second) in samples at fs_target,
    then by name a geometry that cannot work, a rate that cannot be served, an origin that is no counter -> RxEngine.open_monitor's keywords."""
    window = int(round(float(window_s) * fs_target))
    chunk_max = fs_target // 2 if chunk_max is None else int(chunk_max)
    check_geometry(window, chunk_max)
    stream_rates(int(n), fs, fs_target)
    origin_words(ctr0, int(n))
    return dict(window=window, chunk_max=chunk_max, bands=bands, fs=fs, **origin_keywords(ctr0))


def host_table(n_streams: int, window: int, chunk_max: int, hist: int | None = None, bands=(0, 1, 2, 3), *, fs=None,
               fs_target: int | None = None, ctr0=None) -> MonitorTable:
    """The host half of a monitor table, checked; RxEngine.open_monitor adds the device arrays.  fs: the rate of every stream, or one per
    stream (None: all at fs_target, which then need not be stated).  ctr0: the counter origin of every stream, or one per stream (None, or
    a None entry: no origin)."""
    hist = check_geometry(window, chunk_max, hist)
    S = int(n_streams)
    if S < 0:
        raise ValueError("negative number of streams")
    origins = origin_words(ctr0, S)
    b = np.asarray(bands, dtype=np.int64).reshape(-1)
    if b.size != nat.ES_NBANDS or sorted(b.tolist()) != list(range(nat.ES_NBANDS)):
        raise ValueError("bands: the four band indices, each once")
    t = MonitorTable(int(window), int(chunk_max), hist, b.astype(np.uint8), np.zeros(S, np.int64), np.zeros(S, np.int64), np.ones(S, bool),
                     fs_target=int(fs_target or 0), origin_host=origins)
    if fs is not None:
        if not fs_target:
            raise ValueError("fs needs fs_target, the rate the streams are conditioned to")
        rates = stream_rates(S, fs, fs_target)
        if (rates != t.fs_target).any():
            t.rs = resampler_host(rates, fs_target)
    return t


def monitor_ids(table: MonitorTable, sid) -> np.ndarray:
    """Stream ids as int64, each inside the table, open and named once."""
    ids = np.asarray(sid, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= table.n):
        raise ValueError(f"stream id outside [0, {table.n})")
    if np.unique(ids).size != ids.size:
        raise ValueError("a stream is named twice in one push: give each stream one chunk per tick (concatenate its chunks)")
    if not table.live[ids].all():
        raise ValueError("a closed stream")
    return ids


def monitor_chunks(chunks, chunk_max: int, at_rate=None) -> list:
    """The chunks of a tick as 1-D int16 or float32 host arrays (other sample types are converted to float32, as verify() does).
    chunk_max counts samples at fs_target (None: any length): at_rate[i] False marks a chunk at another rate, whose finalized outputs
    monitor_conditioned holds to it instead."""
    out = []
    for i, c in enumerate(chunks):
        a = np.asarray(c.cpu().numpy() if hasattr(c, "cpu") else c)
        if a.ndim != 1:
            raise ValueError(f"a chunk of {a.ndim} dimensions: chunks are 1-D sample arrays, one channel per stream")
        if chunk_max is not None and a.size > chunk_max and (at_rate is None or at_rate[i]):
            raise ValueError(f"a chunk of {a.size} samples is longer than chunk_max = {chunk_max}: push it in pieces, or open the monitor "
                             "with a larger chunk_max")
        out.append(np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32, copy=False)))
    return out


def monitor_conditioned(table: MonitorTable, ids: np.ndarray, arrs: list):
    """-> (lengths at fs_target, other-rate mask, F(n_old)) int64 / bool / int64 per chunk: a chunk at fs_target counts as it is, one at
    another rate as the outputs it finalizes, refused where they exceed chunk_max.  Host mirror only."""
    lengths = np.array([a.size for a in arrs], np.int64)
    other = np.zeros(ids.size, bool) if table.rs is None else table.rs.rate_host[ids, 0] != table.rs.rate_host[ids, 1]
    f_old = np.zeros(ids.size, np.int64)
    if other.any():
        f_old[other], cnt = resample_counts(table.rs, ids[other], lengths[other])
        if cnt.size and cnt.max() > table.chunk_max:
            i = int(np.flatnonzero(other)[int(cnt.argmax())])
            raise ValueError(f"a chunk of {arrs[i].size} samples at {int(table.rs.fs[ids[i]])} Hz finalizes {int(cnt.max())} samples at "
                             f"{table.fs_target} Hz, more than chunk_max = {table.chunk_max}: push it in pieces, or open the monitor with "
                             "a larger chunk_max")
        lengths = lengths.copy()
        lengths[other] = cnt
    return lengths, other, f_old


def pack_chunks(arrs: list, order):
    """The staging buffer of one upload -> (buf uint8, stride, k32): the float32 chunks of `arrs` in the order `order` visits them, then the
    int16 chunks in the order `order` visits them, each a zero-filled row of stride = max(4, the longest chunk rounded up to 4) samples; the
    k32 float32 rows are the first k32 * stride * 4 bytes.  A pure host function."""
    rows = [i for i in order if arrs[i].dtype != np.int16]
    k32 = len(rows)
    rows += [i for i in order if arrs[i].dtype == np.int16]
    stride = max(4, (max((a.size for a in arrs), default=0) + 3) // 4 * 4)
    buf = np.zeros(k32 * stride * 4 + (len(rows) - k32) * stride * 2, np.uint8)
    x32 = buf[:k32 * stride * 4].view(np.float32).reshape(k32, stride)
    x16 = buf[k32 * stride * 4:].view(np.int16).reshape(len(rows) - k32, stride)
    for k, i in enumerate(rows):
        (x32[k] if k < k32 else x16[k - k32])[:arrs[i].size] = arrs[i]
    return buf, stride, k32


def push_arguments(table: MonitorTable, target: int, chunks, streams=None, fs=None):
    """The arguments of a push of live streams (LiveMonitor.push, LiveIdentifier.push), checked without an engine -> (ids int64, chunks as
    1-D int16 / float32 host arrays, their lengths at fs_target).  streams None: one chunk per open stream, in order.  fs= is a check,
    not a conversion: every named stream must have been opened at that rate.  A ValueError names what is refused: that, a chunk that is
    not 1-D, longer than chunk_max or (at another rate) finalizing more than chunk_max samples, a stream named twice, outside the table
    or closed, and a stream with a counter origin whose samples would reach the end of the counter range."""
    chunks = list(chunks)
    if fs is not None and table.rs is None and int(fs) != target:
        raise ValueError(f"chunks at {fs} Hz: this monitor's streams arrive at fs_target = {target} Hz (open a stream with fs={fs} "
                         "to have it conditioned on the device; push(fs=) only checks the rate)")
    if streams is None:
        streams = np.flatnonzero(table.live)
    ids = monitor_ids(table, streams)
    if fs is not None and table.rs is not None and (table.rs.fs[ids] != int(fs)).any():
        bad = int(ids[table.rs.fs[ids] != int(fs)][0])
        raise ValueError(f"chunks at {fs} Hz: stream {bad} was opened at {int(table.rs.fs[bad])} Hz (fs_target = {target} Hz); push(fs=) "
                         "only checks the rate, a stream's rate is fixed when it is opened")
    if len(chunks) != ids.size:
        raise ValueError("one chunk per stream is required")
    arrs = monitor_chunks(chunks, table.chunk_max, None if table.rs is None else table.rs.fs[ids] == target)
    lengths, _, _ = monitor_conditioned(table, ids, arrs)                   # a chunk that finalizes more than chunk_max: refused here
    from .scan import check_counter_reach
    for s, n in zip(ids.tolist(), (table.n_host[ids] + lengths).tolist()):
        if table.origin_host[s] >= 0:
            check_counter_reach(int(table.origin_host[s]), n, "stream")
    return ids, arrs, lengths


class LiveTable:
    """What LiveMonitor and LiveIdentifier say about their streams: both hold a MonitorTable as `table` and the rate the streams are
    conditioned to as `fs_target`; stream ids are the table's slots.  Both also name their `engine`, and hear of slots that were
    opened or closed through `_slots_changed`."""

    def __len__(self) -> int:
        return int(np.count_nonzero(self.table.live))

    def add(self, n: int = 1, fs=None, ctr0=None) -> np.ndarray:
        """n more fresh streams -> their ids; slots of closed streams are used first.  fs: their rate, one or one per stream (None:
        fs_target); ctr0: their counter origins, one or one per stream (None: no origin)."""
        origin_words(ctr0, int(n))                                          # refused by name before the engine is asked
        ids = self.engine.add_monitor_streams(self.table, n, fs, **origin_keywords(ctr0))
        self._slots_changed(ids, closed=False)
        return ids

    def close(self, streams) -> None:
        """Free the slots of `streams` (state, history and what the owner kept per stream are dropped); a push to a closed stream raises."""
        ids = monitor_ids(self.table, streams)
        self.engine.close_monitor_streams(self.table, ids)
        self._slots_changed(ids, closed=True)

    def _slots_changed(self, ids: np.ndarray, closed: bool) -> None:
        """Slots `ids` were just opened as fresh streams, or closed."""

    def _presence(self, det, keys, streams, span, phases, decoys, drift_ppm) -> list:
        """The presence test on the current window [w0, n) of each named stream (None: every open stream), read in
        place in the table's correlation history, under each of `keys` (None: the key of `det` alone) -> per stream None (no whole
        slot) or one Presence per key.  det: the WatermarkDetector whose engine and decoy ring are used.  Everything is checked on the
        host before any GPU work; the table is only read."""
        from . import presence as pr
        from .acquire import check_span
        from .presence_search import search
        tab = self.table
        P, R, drift = pr.check_phases(phases), pr.check_decoys(decoys), pr.check_drift(drift_ppm)
        span = check_span(span)
        ids = np.flatnonzero(tab.live) if streams is None else monitor_ids(tab, streams)
        n, base = tab.n_host[ids], tab.base_host[ids]
        w0 = window_start(n, tab.window)
        nlag = n - (PRE_L - 1) - w0                                         # the window's lags: column w0 - base onwards of the stream's rows
        spans = []
        for s, nl, w in zip(ids.tolist(), nlag.tolist(), w0.tolist()):
            J = max(nl, 0) // nat.ES_FRAME_LEN
            if J and drift > 0:
                pr.skew_table(nl, drift)                                    # a skew of a whole frame, or no slot left: refused by name
            o = int(tab.origin_host[s])
            spans.append(pr.live_span(o, w, J) if o >= 0 else pr.check_reach(span, nl + PRE_L - 1))
        out: list = [None] * int(ids.size)
        some = np.flatnonzero(nlag >= nat.ES_FRAME_LEN)
        n_own = 1 if keys is None else len(keys)
        if some.size and n_own:
            rows4 = np.array([pr.table_rows(tab.bands, s) for s in ids[some].tolist()], np.int64)
            res = search(det.engine, det._presence_ring(R, keys), n_own, tab.corr_hist, nlag[some], [spans[i] for i in some.tolist()], drift, P,
                         at=(rows4, (w0 - base)[some]), pos0=w0[some])
            for i, r in zip(some.tolist(), res):
                out[i] = r
        return out


    def position(self, stream: int) -> int:
        """Samples at fs_target stream `stream` has been verified over since it was opened: the samples received, for a stream at
        another rate the conditioned samples that are final."""
        return int(self.table.n_host[int(stream)])

    def received(self, stream: int) -> int:
        """Samples stream `stream` has received since it was opened, at its own rate."""
        return int(self.table.n_in_host[int(stream)])

    def rate(self, stream: int) -> int:
        """The rate stream `stream` was opened at."""
        return int(self.table.fs[int(stream)]) or int(self.fs_target)

    def origin(self, stream: int) -> int | None:
        """The counter origin stream `stream` was opened with: its frame k carries counter origin + k (None: no origin, counters are
        estimated relative to the window)."""
        o = int(self.table.origin_host[int(stream)])
        return None if o < 0 else o

    def window(self, stream: int) -> tuple[int, int]:
        """(w0, n): the samples of the stream, counted from its opening, that its last push looked at."""
        n = self.position(stream)
        return int(window_start(n, self.table.window)), n


@dataclass
class MonitorTick:
    """What one tick found (RxEngine.monitor_step).  Record q = 4 i + j is band row j of the i-th pushed stream; its window is
    y[rows[q], offset[q] : offset[q] + length[q]] and its peaks are relative to that window."""
    y: object                  # the table's y_hist [4 S, H] float64 (in place: valid until the stream's next push)
    thr: object                # [4 R] float64
    peaks: object              # [4 R, 32] int32, window-relative
    npeaks: object             # [4 R] int32 (count; bit 30 = fallback branch)
    sid: np.ndarray            # [R] int64 the pushed streams, in input order
    rows: np.ndarray           # [4 R] int64 history row of each record
    offset: np.ndarray         # [4 R] int64 column of the window's first sample: w0 - base
    length: np.ndarray         # [4 R] int64 samples of the window: n - w0
    nb: int = nat.ES_NBANDS

    def part(self, a: int, b: int) -> "MonitorTick":
        """The records of pushed streams a .. b - 1 as a tick of their own."""
        q = slice(self.nb * a, self.nb * b)
        return MonitorTick(self.y, self.thr[q], self.peaks[q], self.npeaks[q], self.sid[a:b], self.rows[q], self.offset[q], self.length[q], self.nb)


class MonitorChain:
    """The monitor methods of RxEngine (a mixin without state of its own).  From the engine it uses _call, device and _peak_out."""

    # ---- chunked resampling on its own
    def _resampler_device(self, rt: ResamplerTable) -> None:
        """(Re)build the device half of rt from its host half, keeping the tails and counts of the streams it already has."""
        import torch
        dev, S = self.device, rt.n
        rt.rate = torch.from_numpy(np.ascontiguousarray(rt.rate_host)).to(dev)
        rt.filt = torch.from_numpy(rt.filters if rt.filters.size else np.zeros(1, np.float32)).to(dev)
        old = 0 if rt.tail is None else int(rt.tail.shape[0])
        tail = torch.zeros((S, nat.ES_RSTREAM_TAIL), dtype=torch.float32, device=dev)
        nin = torch.zeros(S, dtype=torch.int64, device=dev)
        if old:
            tail[:old], nin[:old] = rt.tail, rt.nin
        rt.tail, rt.nin = tail, nin

    def open_resampler(self, fs_list, fs_target: int) -> ResamplerTable:
        """A table of fresh streams at rates fs_list, conditioned to fs_target chunk by chunk (any target, not only the engine's)."""
        rt = resampler_host(fs_list, fs_target)
        self._resampler_device(rt)
        return rt

    def _resample_enqueue(self, rt: ResamplerTable, ids, lengths, f_old, counts, x_ptr: int, dtype: int, n_stride: int, sid_ptr: int, len_ptr: int,
                          out_ptr: int, out_stride: int) -> None:
        """One es_resample_stream_batch over records that already lie on the device; the host mirror moves on."""
        rec = np.ascontiguousarray(np.concatenate((np.stack((ids, lengths, rt.n_in_host[ids], f_old, counts), axis=1), rt.rate_host[ids][:, [0, 1, 4]]),
                                                  axis=1).astype(np.int64))                                        # [R, 8], as the C ABI checks it
        self._call("es_resample_stream_batch", x_ptr, dtype, ids.size, n_stride, sid_ptr, len_ptr, rec.ctypes.data, rt.n, rt.rate, rt.filt,
                   int(rt.filters.size), rt.tail, rt.nin, out_ptr, out_stride)
        rt.n_in_host[ids] += lengths

    def resample_step(self, table: ResamplerTable, sid, chunks, *, out=None):
        """chunks[i] (1-D int16 or float32, any length) continues stream sid[i] -> (float32 rows [R, stride] on the device, counts int64 [R]):
        row i holds the counts[i] samples the chunk finalizes, r[F(n_old) : F(n_new)] of r = resample_poly(whole stream, up, down) -- bit
        for bit, possibly none; the rest of a row is not written (out: the rows the kernels write into, float32 [>= R, >= max count],
        float32 chunks first; what is returned is those rows in input order).  One upload, one launch per sample type present."""
        import torch
        ids = np.asarray(sid, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= table.n):
            raise ValueError(f"stream id outside [0, {table.n})")
        if np.unique(ids).size != ids.size:
            raise ValueError("a stream is named twice in one step: give each stream one chunk per step (concatenate its chunks)")
        arrs = monitor_chunks(chunks, None)
        if ids.size != len(arrs):
            raise ValueError("one stream id per chunk is required")
        R = ids.size
        lengths = np.array([a.size for a in arrs], np.int64)
        f_old, counts = resample_counts(table, ids, lengths)
        if out is None:
            out = torch.empty((R, max(4, (int(counts.max()) + 3) // 4 * 4) if R else 4), dtype=torch.float32, device=self.device)
        elif out.dtype != torch.float32 or out.dim() != 2 or not out.is_contiguous() or out.shape[0] < R or (R and out.shape[1] < counts.max()):
            raise ValueError("out: contiguous float32 rows, one per chunk, as long as the most outputs a chunk finalizes")
        ostride = int(out.shape[1])
        if R == 0:
            return out[:0], counts
        order = np.argsort([a.dtype == np.int16 for a in arrs], kind="stable")
        buf, stride, k32 = pack_chunks(arrs, order)
        xd = torch.from_numpy(buf).to(self.device, non_blocking=True)
        rec_d = torch.from_numpy(np.ascontiguousarray(np.stack((ids[order], lengths[order])))).to(self.device, non_blocking=True)      # [2, R]
        for a, b, dt, byte0 in ((0, k32, nat.ES_DTYPE_F32, 0), (k32, R, nat.ES_DTYPE_I16, k32 * stride * 4)):
            if b > a:
                sel = order[a:b]
                self._resample_enqueue(table, ids[sel], lengths[sel], f_old[sel], counts[sel], xd.data_ptr() + byte0, dt, stride,
                                       rec_d[0].data_ptr() + 8 * a, rec_d[1].data_ptr() + 8 * a, out.data_ptr() + 4 * a * ostride, ostride)
        xd.record_stream(torch.cuda.current_stream(self.device))
        if (order == np.arange(R)).all():
            return out[:R], counts
        inv = np.empty(R, np.int64)
        inv[order] = np.arange(R)                                           # rows lie in launch order: back to input order, unwritten columns with them
        return out[torch.from_numpy(inv).to(self.device)], counts

    def open_monitor(self, n_streams: int, *, window: int, chunk_max: int, hist: int | None = None, bands=(0, 1, 2, 3), fs=None,
                     ctr0=None) -> MonitorTable:
        """A table of n_streams fresh streams: windows of `window` samples (>= 2 * 1216), chunks of at most chunk_max samples, history
        rows of `hist` columns (default and minimum window + 1216 + chunk_max), row j of every stream on band bands[j]; fs: the rate
        the streams arrive at, one or one per stream (None: the engine's); ctr0: their counter origins, one or one per stream (None: no
        origin; a host record, read by whoever plans the streams' candidates).  Everything is allocated here; monitor_step only enqueues."""
        import torch
        t = host_table(n_streams, window, chunk_max, hist, bands, fs=fs, fs_target=self.fs, ctr0=ctr0)
        if t.rs is not None:
            self._resampler_device(t.rs)
        S, dev = t.n, self.device
        t.band = torch.from_numpy(np.tile(t.bands, S)).to(dev)
        t.z = torch.zeros((4 * S, 8), dtype=torch.float64, device=dev)
        t.pos = torch.zeros((S, 2), dtype=torch.int64, device=dev)
        t.y_hist = torch.zeros((4 * S, t.hist), dtype=torch.float64, device=dev)
        t.corr_hist = torch.zeros((4 * S, t.hist), dtype=torch.float64, device=dev)
        return t

    def add_monitor_streams(self, table: MonitorTable, n: int, fs=None, ctr0=None) -> np.ndarray:
        """n more fresh streams: closed slots are used first, lowest first, then the table grows (an allocation).  fs: their rate, one or
        one per stream (None: the engine's); ctr0: their counter origins, one or one per stream (None: no origin).  -> their ids."""
        import torch
        n, S = int(n), table.n
        target = table.fs_target or int(self.fs)
        rates = stream_rates(n, fs, target)                                # a rate that cannot be served: refused by name before anything changes
        origins = origin_words(ctr0, n)                                    # ... and so is an origin that is no counter
        table.fs_target = target
        if table.rs is None and (rates != target).any():
            table.rs = resampler_host(np.full(S, target, np.int64), target)
            table.rs.n_in_host[:] = table.n_host                            # at-rate streams: received = conditioned
        ids = np.concatenate((np.flatnonzero(~table.live)[:n], np.arange(S, S + n, dtype=np.int64)))[:n]
        grow = int(np.count_nonzero(ids >= S))
        if grow:
            ext = lambda t, rows: torch.cat((t, torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)))
            table.z, table.y_hist, table.corr_hist = ext(table.z, 4 * grow), ext(table.y_hist, 4 * grow), ext(table.corr_hist, 4 * grow)
            table.pos = ext(table.pos, grow)
            table.band = torch.from_numpy(np.tile(table.bands, S + grow)).to(self.device)
            table.n_host, table.base_host = (np.concatenate((a, np.zeros(grow, np.int64))) for a in (table.n_host, table.base_host))
            table.live = np.concatenate((table.live, np.zeros(grow, bool)))
            table.origin_host = np.concatenate((table.origin_host, np.full(grow, -1, np.int64)))
        table.live[ids] = True
        table.origin_host[ids] = origins
        if table.rs is not None:
            rt = table.rs
            reuse = ids < rt.n
            resampler_extend(rt, rates[~reuse])                              # (ids beyond the table are ascending: rates[~reuse] in their order)
            for s_, f in zip(ids[reuse].tolist(), rates[reuse].tolist()):
                if f not in rt.offsets:
                    resampler_extend(rt, [f])                               # designs the filter; the row it appended is dropped again
                    rt.fs, rt.rate_host, rt.n_in_host = rt.fs[:-1], rt.rate_host[:-1], rt.n_in_host[:-1]
                rt.fs[s_], rt.rate_host[s_], rt.n_in_host[s_] = f, rt.offsets[f], 0
            self._resampler_device(rt)
        return ids

    def close_monitor_streams(self, table: MonitorTable, sid) -> None:
        """Free the slots of streams `sid` and reset them (zero state, empty history): add_monitor_streams hands them out as fresh
        streams, monitor_step refuses them until then."""
        import torch
        ids = monitor_ids(table, sid)
        if ids.size:
            rows = torch.from_numpy((4 * ids[:, None] + np.arange(4)).reshape(-1)).to(self.device)
            table.z[rows] = 0.0
            table.y_hist[rows] = 0.0
            table.corr_hist[rows] = 0.0
            table.pos[torch.from_numpy(ids).to(self.device)] = 0
            if table.rs is not None:
                table.rs.tail[torch.from_numpy(ids).to(self.device)] = 0.0
                table.rs.nin[torch.from_numpy(ids).to(self.device)] = 0
        table.n_host[ids], table.base_host[ids], table.live[ids], table.origin_host[ids] = 0, 0, False, -1
        if table.rs is not None:
            table.rs.n_in_host[ids] = 0

    def monitor_step(self, table: MonitorTable, sid, chunks) -> MonitorTick:
        """One tick: chunks[i] (1-D int16 or float32, 0 .. chunk_max samples) continues stream sid[i]; streams not named are not
        touched.  One upload of the chunks and one launch sequence -- band-pass continued from the stored delay elements (one launch
        per sample type present), the lags the chunks complete, threshold and peaks of every pushed row's window -- whatever the
        number of streams.  Per pushed (stream, band) row, thr / peaks / npeaks are bit for bit those of pick(xcorr(.)) on the
        contiguous slice y[w0 : n] of the whole stream's band-pass output.  A stream at another rate is first conditioned
        on the device, in the same upload (es_resample_stream_batch, one launch per sample type present among them); the samples its
        chunk finalizes (at most chunk_max, possibly none) are its chunk in all of the above, a third band-pass group in float32."""
        import torch
        ids, chunks = monitor_ids(table, sid), list(chunks)
        other_s = None if table.rs is None else table.rs.rate_host[:, 0] != table.rs.rate_host[:, 1]
        arrs = monitor_chunks(chunks, table.chunk_max, None if other_s is None or ids.size != len(chunks) else ~other_s[ids])
        if ids.size != len(arrs):
            raise ValueError("one stream id per chunk is required")
        R = ids.size
        raw = np.array([a.size for a in arrs], np.int64)
        lengths, other, f_old = monitor_conditioned(table, ids, arrs)      # at fs_target: what the band-pass appends
        lay = monitor_layout(table.n_host[ids], table.base_host[ids], lengths, table.window, table.hist)
        q_rows = (4 * ids[:, None] + np.arange(4)).reshape(-1)
        offset, length = np.repeat(lay.w0 - lay.base, 4), np.repeat(lay.n - lay.w0, 4)
        thr, peaks, npeaks, _ = self._peak_out(4 * R, flags=False)
        if R == 0:
            return MonitorTick(table.y_hist, thr, peaks, npeaks, ids, q_rows, offset, length)
        # ONE host buffer, one upload: float32 chunks first (streams at the table's rate, then the others), then int16 likewise; the
        # records in launch order: at-rate float32, at-rate int16, other-rate float32, other-rate int16
        i16 = np.array([a.dtype == np.int16 for a in arrs], bool)
        order = np.argsort(2 * other + i16, kind="stable")
        nA, nB, nC = (int(np.count_nonzero(m)) for m in (~other & ~i16, ~other & i16, other & ~i16))
        nD = R - nA - nB - nC
        buf, stride, k32 = pack_chunks(arrs, order)                         # k32 = nA + nC
        xd = torch.from_numpy(buf).to(self.device, non_blocking=True)
        rec = np.ascontiguousarray(np.stack((ids, lengths, lay.col, lay.move, lay.base), axis=1)[order])          # [R, 5], as the C ABI checks it
        rec_d = torch.from_numpy(np.ascontiguousarray(np.concatenate((rec.T, raw[order][None])))).to(self.device, non_blocking=True)    # [6, R]: + the chunks' own lengths
        pk = np.stack((q_rows, offset, length - (PRE_L - 1))).astype(np.int32)                                      # [3, 4 R], input order
        pk_d = torch.from_numpy(pk).to(self.device, non_blocking=True)
        S, H = table.n, table.hist
        byte16 = k32 * stride * 4
        nE, ostride, cond = nC + nD, 4, None
        if nE:                                                              # condition the other-rate chunks: row e of `cond` = record nA + nB + e
            ostride = max(4, (int(lengths[other].max()) + 3) // 4 * 4)
            cond = torch.empty((nE, ostride), dtype=torch.float32, device=self.device)
            for a, b, dt, x_ptr in ((nA + nB, nA + nB + nC, nat.ES_DTYPE_F32, xd.data_ptr() + 4 * nA * stride),
                                    (nA + nB + nC, R, nat.ES_DTYPE_I16, xd.data_ptr() + byte16 + 2 * nB * stride)):
                if b > a:
                    sel = order[a:b]
                    self._resample_enqueue(table.rs, ids[sel], raw[sel], f_old[sel], lengths[sel], x_ptr, dt, stride, rec_d[0].data_ptr() + 8 * a,
                                           rec_d[5].data_ptr() + 8 * a, cond.data_ptr() + 4 * (a - nA - nB) * ostride, ostride)
        for a, b, dt, x_ptr, n_stride in ((0, nA, nat.ES_DTYPE_F32, xd.data_ptr(), stride), (nA, nA + nB, nat.ES_DTYPE_I16, xd.data_ptr() + byte16, stride),
                                          (nA + nB, R, nat.ES_DTYPE_F32, cond.data_ptr() if nE else 0, ostride)):
            if b > a:
                cols = [rec_d[w].data_ptr() + 8 * a for w in range(5)]
                self._call("es_bpf_stream_batch", x_ptr, dt, b - a, n_stride, *cols, rec[a:].ctypes.data, S, H, table.band, table.z, table.pos,
                           table.y_hist, table.corr_hist)
        self._call("es_xcorr_stream_batch", table.y_hist, R, max(stride, ostride), rec_d[0], rec_d[1], rec_d[2], rec.ctypes.data, S, H, table.band,
                   table.corr_hist)
        self._call("es_pick_at_batch", table.corr_hist, 4 * S, H, 4 * R, pk_d[0], pk_d[1], pk_d[2], thr, peaks, npeaks)
        xd.record_stream(torch.cuda.current_stream(self.device))
        if cond is not None:
            cond.record_stream(torch.cuda.current_stream(self.device))
        table.n_host[ids], table.base_host[ids] = lay.n, lay.base
        if table.rs is not None:
            table.rs.n_in_host[ids[~other]] += raw[~other]                  # (the other-rate streams' were moved on by _resample_enqueue)
        return MonitorTick(table.y_hist, thr, peaks, npeaks, ids, q_rows, offset, length)


__all__ = ["SEG", "MIN_WINDOW", "LiveTable", "MonitorChain", "MonitorLayout", "MonitorTable", "MonitorTick", "ResamplerTable", "check_geometry",
           "history_columns", "host_table", "monitor_chunks", "monitor_conditioned", "monitor_ids", "monitor_layout", "pack_chunks", "push_arguments",
           "resample_counts", "resampler_host", "stream_rates", "window_start"]
