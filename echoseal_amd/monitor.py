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

    @property
    def n(self) -> int:
        return int(self.live.size)


def host_table(n_streams: int, window: int, chunk_max: int, hist: int | None = None, bands=(0, 1, 2, 3)) -> MonitorTable:
    """The host half of a monitor table, checked; RxEngine.open_monitor adds the device arrays."""
    hist = check_geometry(window, chunk_max, hist)
    S = int(n_streams)
    if S < 0:
        raise ValueError("negative number of streams")
    b = np.asarray(bands, dtype=np.int64).reshape(-1)
    if b.size != nat.ES_NBANDS or sorted(b.tolist()) != list(range(nat.ES_NBANDS)):
        raise ValueError("bands: the four band indices, each once")
    return MonitorTable(int(window), int(chunk_max), hist, b.astype(np.uint8), np.zeros(S, np.int64), np.zeros(S, np.int64), np.ones(S, bool))


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


def monitor_chunks(chunks, chunk_max: int) -> list:
    """The chunks of a tick as 1-D int16 or float32 host arrays (other sample types are converted to float32, as verify() does)."""
    out = []
    for c in chunks:
        a = np.asarray(c.cpu().numpy() if hasattr(c, "cpu") else c)
        if a.ndim != 1:
            raise ValueError(f"a chunk of {a.ndim} dimensions: chunks are 1-D sample arrays, one channel per stream")
        if a.size > chunk_max:
            raise ValueError(f"a chunk of {a.size} samples is longer than chunk_max = {chunk_max}: push it in pieces, or open the monitor "
                             "with a larger chunk_max")
        out.append(np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32, copy=False)))
    return out


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


class MonitorChain:
    """The monitor methods of RxEngine (a mixin without state of its own).  From the engine it uses _ctx, _lib, device, _stream and
    _peak_out."""

    def open_monitor(self, n_streams: int, *, window: int, chunk_max: int, hist: int | None = None, bands=(0, 1, 2, 3)) -> MonitorTable:
        """A table of n_streams fresh streams at the engine's rate: windows of `window` samples (>= 2 * 1216), chunks of at most
        chunk_max samples, history rows of `hist` columns (default and minimum window + 1216 + chunk_max), row j of every stream on
        band bands[j].  Everything is allocated here; monitor_step only enqueues."""
        import torch
        t = host_table(n_streams, window, chunk_max, hist, bands)
        S, dev = t.n, self.device
        t.band = torch.from_numpy(np.tile(t.bands, S)).to(dev)
        t.z = torch.zeros((4 * S, 8), dtype=torch.float64, device=dev)
        t.pos = torch.zeros((S, 2), dtype=torch.int64, device=dev)
        t.y_hist = torch.zeros((4 * S, t.hist), dtype=torch.float64, device=dev)
        t.corr_hist = torch.zeros((4 * S, t.hist), dtype=torch.float64, device=dev)
        return t

    def add_monitor_streams(self, table: MonitorTable, n: int) -> np.ndarray:
        """n more fresh streams: closed slots are used first, lowest first, then the table grows (an allocation).  -> their ids."""
        import torch
        n, S = int(n), table.n
        ids = np.concatenate((np.flatnonzero(~table.live)[:n], np.arange(S, S + n, dtype=np.int64)))[:n]
        grow = int(np.count_nonzero(ids >= S))
        if grow:
            ext = lambda t, rows: torch.cat((t, torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)))
            table.z, table.y_hist, table.corr_hist = ext(table.z, 4 * grow), ext(table.y_hist, 4 * grow), ext(table.corr_hist, 4 * grow)
            table.pos = ext(table.pos, grow)
            table.band = torch.from_numpy(np.tile(table.bands, S + grow)).to(self.device)
            table.n_host, table.base_host = (np.concatenate((a, np.zeros(grow, np.int64))) for a in (table.n_host, table.base_host))
            table.live = np.concatenate((table.live, np.zeros(grow, bool)))
        table.live[ids] = True
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
        table.n_host[ids], table.base_host[ids], table.live[ids] = 0, 0, False

    def monitor_step(self, table: MonitorTable, sid, chunks) -> MonitorTick:
        """One tick: chunks[i] (1-D int16 or float32, 0 .. chunk_max samples) continues stream sid[i]; streams not named are not
        touched.  One upload of the chunks and one launch sequence -- band-pass continued from the stored delay elements (one launch
        per sample type present), the lags the chunks complete, threshold and peaks of every pushed row's window -- whatever the
        number of streams.  Per pushed (stream, band) row, thr / peaks / npeaks are bit for bit those of pick(xcorr(.)) on the
        contiguous slice y[w0 : n] of the whole stream's band-pass output."""
        import torch
        ids = monitor_ids(table, sid)
        arrs = monitor_chunks(chunks, table.chunk_max)
        if ids.size != len(arrs):
            raise ValueError("one stream id per chunk is required")
        R = ids.size
        lengths = np.array([a.size for a in arrs], np.int64)
        lay = monitor_layout(table.n_host[ids], table.base_host[ids], lengths, table.window, table.hist)
        q_rows = (4 * ids[:, None] + np.arange(4)).reshape(-1)
        offset, length = np.repeat(lay.w0 - lay.base, 4), np.repeat(lay.n - lay.w0, 4)
        thr, peaks, npeaks, _ = self._peak_out(4 * R, flags=False)
        if R == 0:
            return MonitorTick(table.y_hist, thr, peaks, npeaks, ids, q_rows, offset, length)
        # float32 chunks first, then int16: ONE host buffer, one upload, a launch per sample type over its slice of the records
        order = np.argsort([a.dtype == np.int16 for a in arrs], kind="stable")
        k32 = int(sum(a.dtype != np.int16 for a in arrs))
        stride = max(4, (int(lengths.max()) + 3) // 4 * 4)
        buf = np.zeros(k32 * stride * 4 + (R - k32) * stride * 2, np.uint8)
        x32 = buf[:k32 * stride * 4].view(np.float32).reshape(k32, stride)
        x16 = buf[k32 * stride * 4:].view(np.int16).reshape(R - k32, stride)
        for k, i in enumerate(order):
            (x32 if k < k32 else x16)[k if k < k32 else k - k32, :arrs[i].size] = arrs[i]
        xd = torch.from_numpy(buf).to(self.device, non_blocking=True)
        rec = np.ascontiguousarray(np.stack((ids, lengths, lay.col, lay.move, lay.base), axis=1)[order])          # [R, 5], as the C ABI checks it
        rec_d = torch.from_numpy(np.ascontiguousarray(rec.T)).to(self.device, non_blocking=True)                    # [5, R]
        pk = np.stack((q_rows, offset, length - (PRE_L - 1))).astype(np.int32)                                      # [3, 4 R], input order
        pk_d = torch.from_numpy(pk).to(self.device, non_blocking=True)
        S, H, st = table.n, table.hist, self._stream()
        for a, b, dt, byte0 in ((0, k32, nat.ES_DTYPE_F32, 0), (k32, R, nat.ES_DTYPE_I16, k32 * stride * 4)):
            if b > a:
                cols = [rec_d[w].data_ptr() + 8 * a for w in range(5)]
                nat.check(self._ctx, self._lib.es_bpf_stream_batch(self._ctx, xd.data_ptr() + byte0, dt, b - a, stride, *cols, rec[a:].ctypes.data, S, H,
                                                                   table.band.data_ptr(), table.z.data_ptr(), table.pos.data_ptr(),
                                                                   table.y_hist.data_ptr(), table.corr_hist.data_ptr(), st), "es_bpf_stream_batch")
        nat.check(self._ctx, self._lib.es_xcorr_stream_batch(self._ctx, table.y_hist.data_ptr(), R, stride, rec_d[0].data_ptr(), rec_d[1].data_ptr(),
                                                             rec_d[2].data_ptr(), rec.ctypes.data, S, H, table.band.data_ptr(),
                                                             table.corr_hist.data_ptr(), st), "es_xcorr_stream_batch")
        nat.check(self._ctx, self._lib.es_pick_at_batch(self._ctx, table.corr_hist.data_ptr(), 4 * S, H, 4 * R, pk_d[0].data_ptr(), pk_d[1].data_ptr(),
                                                        pk_d[2].data_ptr(), thr.data_ptr(), peaks.data_ptr(), npeaks.data_ptr(), st), "es_pick_at_batch")
        xd.record_stream(torch.cuda.current_stream(self.device))
        table.n_host[ids], table.base_host[ids] = lay.n, lay.base
        return MonitorTick(table.y_hist, thr, peaks, npeaks, ids, q_rows, offset, length)


__all__ = ["SEG", "MIN_WINDOW", "MonitorChain", "MonitorLayout", "MonitorTable", "MonitorTick", "check_geometry", "history_columns", "host_table",
           "monitor_chunks", "monitor_ids", "monitor_layout", "window_start"]
