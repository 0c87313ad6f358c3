"""RxEngine: batched EchoSeal receive hot path on one MI355X.

Thin host layer over the C ABI (include/echoseal_hip.h).  torch is used only to own device
buffers and to name the HIP stream; every computation is a hand-written HIP kernel.  Each method
mirrors one stage of the reference detector:

    bpf / xcorr / pick / sync   rtwm/detector.py:59-99   (band-pass, NCC, threshold, NMS)
    open_monitor / monitor_step the same three stages continued chunk by chunk for live streams (monitor.py)
    llr                         rtwm/detector.py:296-416 (_llr)
    scl                         rtwm/fastpolar.py:254-359 (PolarCode.decode, pre-validator)
    polar_encode                rtwm/fastpolar.py:237-252

`decode_batch` strings them together for the throughput metric: one frame record ->
sync + LLR (variant 0, known start/counter) + SCL-L.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from .monitor import MonitorChain, MonitorLayout, MonitorTable, MonitorTick, monitor_layout      # the live monitor's public names stay importable from here
from .tables import pack_tables
from .transmit import (EMBED_ROW_SAMPLES, EmbedClip, EmbedLayout, EmbedResult, StreamLayout, StreamTable, TxChain, embed_launches, embed_layout,
                       stream_layout)      # the transmit chain's public names stay importable from here

_FRAME_DTYPES = {torch.int16: nat.ES_DTYPE_I16, torch.float32: nat.ES_DTYPE_F32}     # what the band-pass reads
_RESAMPLE_DTYPES = {torch.int16: (nat.ES_DTYPE_I16, np.int16), torch.float32: (nat.ES_DTYPE_F32, np.float32),
                    torch.float64: (nat.ES_DTYPE_F64, np.float64)}              # what es_resample_ragged_batch reads
RESAMPLE_TILE = nat.ES_RESAMPLE_TILE                                           # outputs per workgroup of es_resample_ragged_kernel


def _peak_start(start: str) -> None:
    if start != "peak":
        raise ValueError(f'start must be a tensor, None or "peak", not {start!r}')


@dataclass
class SclResult:
    hard_info: torch.Tensor    # [B,55] uint8 (engines of another code: [B, ceil((K - 8) / 8)])
    hard_ok: torch.Tensor      # [B] uint8
    cand_info: torch.Tensor    # [B,L,55] uint8, ascending metric
    cand_metric: torch.Tensor  # [B,L] float64
    cand_ok: torch.Tensor      # [B,L] uint8
    ncand: torch.Tensor        # [B] int32 (0 = list loop skipped; < 0 = the kernel could not decode the record: see check())

    def check(self) -> "SclResult":
        """Raise if the list decoder reported records it could not decode (ncand < 0: a block found no free slot of the scratch
        slab -- cannot happen while resident blocks <= slots, and must never pass silently).  Synchronises on the result."""
        bad = int((self.ncand < 0).sum().item())
        if bad:
            raise nat.NativeError(f"es_scl_batch: {bad} record(s) were not decoded (no free scratch-slab slot); the candidate rows of those records are undefined")
        return self


@dataclass
class SyncResult:
    y: torch.Tensor            # [B,T] float64 band-passed records
    corr: torch.Tensor | None  # [B,T-62] float64
    thr: torch.Tensor          # [B] float64
    peaks: torch.Tensor        # [B,32] int32
    npeaks: torch.Tensor       # [B] int32 (count; bit 30 = fallback branch)
    corr32: torch.Tensor | None = None   # float32 screen (sync_fast only)
    flags: torch.Tensor | None = None    # reason code 1..5 of records settled from float64 values alone, else 0 (sync_fast only)
    y32: torch.Tensor | None = None


@dataclass
class KeyRing:
    """Keys as device data (es_keyring_derive_batch): row k of `ring` holds what the keyed kernels need of key k (layout:
    include/echoseal_hip.h)."""
    ring: torch.Tensor         # [N, ES_KEYRING_BYTES] uint8
    n: int

    @property
    def aead_key(self) -> torch.Tensor:      # [N, 32] uint8
        return self.ring[:, 0:32]

    @property
    def hdr_pn(self) -> torch.Tensor:        # [N, 16] uint8 = np.packbits(pn_bits(0, 128)) of each key
        return self.ring[:, 272:288]

    @property
    def hop0(self) -> torch.Tensor:          # [N] uint8: band index of counter 0
        return self.ring[:, 288]


@dataclass
class DevicePlan:
    """A utils.ConditionPlan whose filter pool and descriptors are on the device (RxEngine.condition_upload)."""
    plan: object               # utils.ConditionPlan (host)
    filt: torch.Tensor         # filter pool, float32 or float64 (never empty: one zero where no record has a filter)
    desc: torch.Tensor         # [R, 8] int64


@dataclass
class PlanResult:
    slot: torch.Tensor         # [N * rows, 400] uint8: index into the row's peaks, try order (entries past `count` undefined)
    ctr: torch.Tensor          # [N * rows, 400] int32 (the counters' 32-bit words)
    count: torch.Tensor        # [N * rows] int32
    looked: torch.Tensor       # [N * rows] int32: fitting peaks looked at


@dataclass
class Memo:
    """A verdict memo on the device (RxEngine.open_memo; layout and rules: include/echoseal_hip.h, host model: memo.MemoModel).  The
    uint64 words are held in int64 tensors, bit for bit."""
    table: torch.Tensor        # [slots, 2] int64: the records themselves, -1 / -1 (all ones) where empty
    claim: torch.Tensor        # [slots] int32: es_memo_insert_batch's claim words, -1 (0xFFFFFFFF) between calls
    slots: int


class RxEngine(TxChain, MonitorChain):
    def __init__(self, device: int | torch.device = 0, *, list_size_max: int = 32, fs: int = 48_000, code_k: int = 448):
        """code_k: information positions of the polar code (data bits + CRC-8).  448 is the reference's own code (rtwm/polar_fast.py:8-9);
        any other 9 <= K <= 1024 (PolarCode(1024, K), rtwm/fastpolar.py:209-234) makes an engine whose `scl` is the only FEC entry point
        (rows of ceil((K - 8) / 8) bytes = np.packbits of the information bits), on the lane-per-path kernel: it needs list_size_max > 32
        or the "scl_lane_slab" option.
        list_size_max: the largest list `scl` will be asked for (sizes the list decoder's scratch: 0.4 GB, above 32 another 1.6 GB);
        0 = a front-end engine (everything but `scl`, no list-decoder scratch): what a pipeline's band-pass / sync / demodulator streams use."""
        if not torch.cuda.is_available():
            raise nat.NativeError("RxEngine needs a ROCm GPU: torch.cuda.is_available() is False")
        self.device = torch.device("cuda", device if isinstance(device, int) else (device.index or 0))
        self._lib = nat.load()
        self._ctx = self._lib.es_create(self.device.index, int(list_size_max))
        if not self._ctx:
            raise nat.NativeError("es_create failed: " + (self._lib.es_last_error(None) or b"?").decode())
        self.list_size_max = int(list_size_max)
        self.fs = fs
        self.code_k = int(code_k)
        self.set_tables(*pack_tables(fs, self.code_k))
        self.info_bytes = int(self._lib.es_info_bytes(self._ctx))

    def tables(self):
        """The host arrays last installed: (ba [4, 18] float64, tpl, taps [4, ES_MAX_TAPS] float32, ntaps int32 [4], frozen)."""
        return self._tables

    def set_tables(self, ba, tpl, taps, ntaps, frozen) -> None:
        """Install band-pass coefficients, sync templates, matched filters and the frozen set (es_set_tables): what __init__ does with
        pack_tables(fs, code_k).  Arrays in pack_tables' shapes and types; work enqueued under the previous tables is waited for.  For
        tests and experiments that need tables the band plan never produces, such as a one-tap matched filter."""
        torch.cuda.synchronize(self.device)
        self._tables = (ba, tpl, taps, ntaps, frozen)       # keep host arrays alive
        self._call("es_set_tables", ba.ctypes.data, tpl.ctypes.data, taps.ctypes.data, ntaps.ctypes.data, frozen.ctypes.data)

    def set_option(self, name: str, value: int) -> None:
        """Tuning knobs of the native library (results never depend on them); see include/echoseal_hip.h."""
        self._call("es_set_option", name.encode(), int(value))

    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.es_destroy(self._ctx)
            self._ctx = None

    def __del__(self):  # pragma: no cover
        try:
            if not sys.is_finalizing():            # at interpreter shutdown the HIP runtime may already be gone; the OS reclaims the rest
                self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _call(self, name: str, *args) -> None:
        """The one place the C ABI is called (include/echoseal_hip.h): entry point `name`, looked up on _lib at every call (tests replace
        _lib), with the context first, every tensor as its data_ptr() and everything else as it is -- None (a NULL pointer), sizes, addresses
        already formed, floats, bytes --, and the current stream last exactly when the name ends in _batch: the header's own rule, held by
        tests/test_binding_call.py.  Nothing is checked here.  A return code raises nat.check's NativeError.
        A tensor is an object whose type is torch.Tensor itself: one of a subclass (an nn.Parameter) is handed through unconverted and
        ctypes refuses it -- no caller passes one; hand its .data instead."""
        args = [a.data_ptr() if type(a) is torch.Tensor else a for a in args]
        if name.endswith("_batch"):
            args.append(self._stream())
        rc = getattr(self._lib, name)(self._ctx, *args)
        if rc:
            nat.check(self._ctx, rc, name)

    def _dev(self, x, dtype) -> torch.Tensor:
        t = torch.as_tensor(x)
        if t.dtype != dtype:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=True).contiguous()

    def _frames(self, frames: torch.Tensor):
        """The records of a band-pass call, checked: -> (contiguous frames, their native dtype code, B, T)."""
        if frames.dim() != 2:
            raise ValueError("frames must be [B, T]")
        dt = _FRAME_DTYPES.get(frames.dtype)
        if dt is None:
            raise ValueError("frames must be float32 or int16")
        return frames.contiguous(), dt, frames.shape[0], frames.shape[1]

    def _peak_out(self, B: int, flags: bool = True):
        """Outputs of a peak picker: thr, peaks (the kernels write whole rows, -1 = unused), npeaks, flags (None unless asked for)."""
        dev = self.device
        return (torch.empty(B, dtype=torch.float64, device=dev), torch.empty((B, nat.ES_MAX_PEAKS), dtype=torch.int32, device=dev),
                torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev) if flags else None)

    def _llr_out(self, out: torch.Tensor | None, B: int) -> torch.Tensor:
        """The demodulator's output rows: the caller's, checked, or new ones."""
        if out is None:
            return torch.empty((B, 1024), dtype=torch.float32, device=self.device)
        if out.shape != (B, 1024) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 [B, 1024] tensor")
        return out

    # ------------------------------------------------------------------ sync stage
    def bpf(self, frames: torch.Tensor, band: torch.Tensor) -> torch.Tensor:
        frames, dt, B, T = self._frames(frames)
        y = torch.empty((B, T), dtype=torch.float64, device=self.device)
        self._call("es_bpf_batch", frames, dt, B, T, band, y)
        return y

    def bpf2(self, frames: torch.Tensor, band: torch.Tensor):
        """Band-pass with both outputs: y (float64) and y32 = (float)y."""
        frames, dt, B, T = self._frames(frames)
        y = torch.empty((B, T), dtype=torch.float64, device=self.device)
        y32 = torch.empty((B, T), dtype=torch.float32, device=self.device)
        self._call("es_bpf2_batch", frames, dt, B, T, band, y, y32)
        return y, y32

    def xcorr32(self, y32: torch.Tensor, band: torch.Tensor) -> torch.Tensor:
        B, T = y32.shape
        corr = torch.empty((B, T - 62), dtype=torch.float32, device=self.device)
        self._call("es_xcorr32_batch", y32, B, T, band, corr)
        return corr

    def pick_exact(self, corr32: torch.Tensor, y: torch.Tensor, band: torch.Tensor):
        """thr / peaks / npeaks identical to pick(xcorr(y)); also returns the per-record flags (reason codes 1..5, 0 = settled from the screen)."""
        B, T = y.shape
        thr, peaks, npeaks, flags = self._peak_out(B)
        self._call("es_pick_exact_batch", corr32, y, B, T, band, thr, peaks, npeaks, flags)
        return thr, peaks, npeaks, flags

    def sync_fused(self, y: torch.Tensor, y32: torch.Tensor, band: torch.Tensor):
        """Correlation screen + exact threshold / peak picking in ONE kernel (the screen row never leaves LDS):
        -> (thr, peaks, npeaks, flags), identical to pick(xcorr(y))."""
        B, T = y.shape
        thr, peaks, npeaks, flags = self._peak_out(B)
        self._call("es_sync_fused_batch", y32, y, B, T, band, thr, peaks, npeaks, flags)
        return thr, peaks, npeaks, flags

    def front(self, frames: torch.Tensor, band: torch.Tensor, pn_rows: torch.Tensor, *, start: torch.Tensor | str | None = None,
              out: torch.Tensor | None = None):
        """bpf2 -> sync_fused -> llr (variant 0) in one library call (es_front_batch): -> (y, thr, peaks, npeaks, flags, llr).
        start="peak": the demodulator reads each record at its first detected peak (es_front_peak_batch; no peak = 0)."""
        frames, dt, B, T = self._frames(frames)
        y = torch.empty((B, T), dtype=torch.float64, device=self.device)
        y32 = torch.empty((B, T), dtype=torch.float32, device=self.device)
        thr, peaks, npeaks, flags = self._peak_out(B)
        out = self._llr_out(out, B)
        if isinstance(start, str):
            _peak_start(start)
            self._call("es_front_peak_batch", frames, dt, B, T, band, pn_rows, y, y32, thr, peaks, npeaks, flags, out)
        else:
            self._call("es_front_batch", frames, dt, B, T, band, pn_rows, start, y, y32, thr, peaks, npeaks, flags, out)
        return y, thr, peaks, npeaks, flags, out

    def front_steps(self, frames: torch.Tensor, band: torch.Tensor, pn_rows: torch.Tensor, *, start: torch.Tensor | str | None = None,
                    out: torch.Tensor | None = None, events=None, side: torch.cuda.Stream | None = None):
        """The same sequence as three library calls on the current stream, -> what `front` returns: the one place it is written out
        (decode_batch and every DecodePipeline arrangement run it).  events: two timing events, recorded before and after the sync.
        out: the rows the demodulator writes.  side: a stream the demodulator runs on beside the sync -- both only need y --, forked
        after the band-pass and joined before returning (the current stream itself: no fork, the demodulator still ahead of the sync)."""
        y, y32 = self.bpf2(frames, band)
        peak = isinstance(start, str)
        beside = side is not None and not peak
        if beside:
            cur = torch.cuda.current_stream(self.device)
            if side != cur:
                side.wait_stream(cur)
            with torch.cuda.stream(side):
                llr = self.llr(y, band, pn_rows, start=start, variant=0, out=out)
        if events is not None:
            events[0].record()
        thr, peaks, npeaks, flags = self.sync_fused(y, y32, band)        # correlation screen + exact picking, one kernel
        if events is not None:
            events[1].record()
        if not beside:                  # (start="peak": at the first detected peak, read in place from the peaks, so behind the sync)
            llr = self.llr(y, band, pn_rows, start=start, peaks=peaks if peak else None, variant=0, out=out)
        elif side != cur:
            cur.wait_stream(side)
        return y, thr, peaks, npeaks, flags, llr

    def reserve(self, B_max: int, T_max: int) -> None:
        """Size the context's workspaces once (es_reserve): afterwards the sync entry points only enqueue."""
        self._call("es_reserve", int(B_max), int(T_max))

    FAST_MAX_LAGS = 4096

    def sync_fast(self, frames: torch.Tensor, band: torch.Tensor, *, fused: bool = True) -> SyncResult:
        """Band-pass + float32 correlation screen + exact peak picking (results identical to sync()).  fused: screen and
        picking in one kernel (the default); otherwise es_xcorr32_batch -> es_pick_exact_batch with the screen in HBM."""
        y, y32 = self.bpf2(frames, band)
        if fused:
            corr32 = None
            thr, peaks, npeaks, flags = self.sync_fused(y, y32, band)
        else:
            corr32 = self.xcorr32(y32, band)
            thr, peaks, npeaks, flags = self.pick_exact(corr32, y, band)
        res = SyncResult(y, None, thr, peaks, npeaks)
        res.corr32, res.flags, res.y32 = corr32, flags, y32
        return res

    def xcorr(self, y: torch.Tensor, band: torch.Tensor) -> torch.Tensor:
        B, T = y.shape
        corr = torch.empty((B, T - 62), dtype=torch.float64, device=self.device)
        self._call("es_xcorr_batch", y, B, T, band, corr)
        return corr

    def pick(self, corr: torch.Tensor):
        B, n = corr.shape
        thr, peaks, npeaks, _ = self._peak_out(B, flags=False)
        self._call("es_pick_batch", corr, B, n, thr, peaks, npeaks)
        return thr, peaks, npeaks

    def sync(self, frames: torch.Tensor, band: torch.Tensor, *, keep_corr: bool = True) -> SyncResult:
        y = self.bpf(frames, band)
        corr = self.xcorr(y, band)
        thr, peaks, npeaks = self.pick(corr)
        return SyncResult(y, corr if keep_corr else None, thr, peaks, npeaks)

    def _lens(self, lens, rows: int) -> torch.Tensor:
        """Per-row sample counts as the int32 [rows] device tensor the ragged entry points read."""
        lens = self._dev(lens, torch.int32).reshape(-1)
        if lens.numel() != rows:
            raise ValueError("lens: one sample count per row")
        return lens

    def sync_ragged(self, frames: torch.Tensor, lens, band: torch.Tensor, *, keep_corr: bool = False) -> SyncResult:
        """sync() for records of unequal length in one batch (es_sync_ragged_batch): record i = frames[i, :lens[i]], the rest of the
        row is padding that may hold anything.  thr / peaks / npeaks, y[i, :lens[i]] and corr[i, :lens[i] - 62] are those of
        sync(frames[i:i+1, :lens[i]]), bit for bit; a record shorter than 63 samples has no peak (npeaks 0, thr 0).  y and corr past a
        record's end are unspecified."""
        frames, dt, B, T = self._frames(frames)
        lens = self._lens(lens, B)
        y = torch.empty((B, T), dtype=torch.float64, device=self.device)
        corr = torch.empty((B, max(T - 62, 0)), dtype=torch.float64, device=self.device) if keep_corr else None
        thr, peaks, npeaks, _ = self._peak_out(B, flags=False)
        self._call("es_sync_ragged_batch", frames, dt, B, T, lens, band, y, corr, thr, peaks, npeaks)
        return SyncResult(y, corr, thr, peaks, npeaks)

    # ------------------------------------------------------------------ soft demod
    def _at(self, y: torch.Tensor, start, rows, peaks):
        """Record addressing of the peak-addressed entry points: -> (B, row int32 [B] or None, start int32 or None, stride)."""
        if isinstance(start, str):
            _peak_start(start)
            if peaks is None or peaks.dim() != 2 or peaks.shape[1] != nat.ES_MAX_PEAKS or peaks.dtype != torch.int32 or not peaks.is_contiguous():
                raise ValueError('start="peak" needs peaks=: the contiguous int32 [B, 32] peaks of a sync call')
            start, stride = peaks, nat.ES_MAX_PEAKS
        elif peaks is not None:
            raise ValueError('peaks= goes with start="peak"')
        else:
            stride = 1
            if start is not None:
                start = self._dev(start, torch.int32).reshape(-1)
        if rows is not None:
            rows = self._dev(rows, torch.int32).reshape(-1)
            B = rows.numel()
        else:
            B = y.shape[0]
        if start is not None and start.numel() < (B - 1) * stride + 1 and B > 0:
            raise ValueError("start: one entry per record")
        return B, rows, start, stride

    def llr(self, y: torch.Tensor, band: torch.Tensor, pn_rows: torch.Tensor, *, start: torch.Tensor | str | None = None,
            variant: int = 0, want_diag: bool = False, out: torch.Tensor | None = None, rows: torch.Tensor | None = None,
            peaks: torch.Tensor | None = None):
        """Batched _llr (rtwm/detector.py:296-416).  Record i = y[i] from start[i] (None = 0): es_llr_batch.
        In place, without gathering frames (es_llr_at_batch): rows= reads record i from y[rows[i]]; start="peak" with peaks= (the
        [B, 32] peaks of a sync call) starts it at the first detected peak (none: 0).  band, pn_rows and the outputs follow i."""
        T = y.shape[1]
        at = rows is not None or peaks is not None or isinstance(start, str)
        if at:
            B, rows, st, stride = self._at(y, start, rows, peaks)
        else:
            B = y.shape[0]
        out = self._llr_out(out, B)
        best_s = torch.empty(B, dtype=torch.int32, device=self.device) if want_diag else None
        score = torch.empty((B, 2), dtype=torch.float32, device=self.device) if want_diag else None
        if at:
            self._call("es_llr_at_batch", y, y.shape[0], T, B, rows, st, stride, band, pn_rows, int(variant), out, best_s, score)
        else:
            self._call("es_llr_batch", y, B, T, start, band, pn_rows, int(variant), out, best_s, score)
        return (out, best_s, score) if want_diag else out

    def header(self, y: torch.Tensor, band: torch.Tensor, hdr_pn: torch.Tensor, *, start: torch.Tensor | str | None = None,
               want_diag: bool = False, rows: torch.Tensor | None = None, peaks: torch.Tensor | None = None):
        """Batched _decode_header (rtwm/detector.py:452-515) -> (ok uint8[B], val int32[B], score float32[B]);
        want_diag: also the chosen shift, (ok, val, score, best_s int32[B]).  rows= / start="peak" with peaks=: in place, as for llr
        (es_header_at_batch)."""
        T = y.shape[1]
        at = rows is not None or peaks is not None or isinstance(start, str)
        if at:
            B, rows, st, stride = self._at(y, start, rows, peaks)
        else:
            B = y.shape[0]
        if hdr_pn.shape[0] == 1 and B > 1:
            hdr_pn = hdr_pn.expand(B, 16)
        hdr_pn = hdr_pn.contiguous()
        ok = torch.empty(B, dtype=torch.uint8, device=self.device)
        val = torch.empty(B, dtype=torch.int32, device=self.device)
        score = torch.empty(B, dtype=torch.float32, device=self.device)
        best_s = torch.empty(B, dtype=torch.int32, device=self.device) if want_diag else None
        if at:
            self._call("es_header_at_batch", y, y.shape[0], T, B, rows, st, stride, band, hdr_pn, ok, val, score, best_s)
        else:
            self._call("es_header_batch", y, B, T, start, band, hdr_pn, ok, val, score, best_s)
        return (ok, val, score, best_s) if want_diag else (ok, val, score)

    # ------------------------------------------------------------------ FEC
    def scl(self, llr: torch.Tensor, *, list_size: int = 8, skip_if_hard_ok: bool = True) -> SclResult:
        if llr.dim() != 2 or llr.shape[1] != 1024:
            raise ValueError("llr must be [B, 1024]")
        if llr.dtype == torch.float32:
            dt = nat.ES_DTYPE_F32
        elif llr.dtype == torch.float64:
            dt = nat.ES_DTYPE_F64
        else:
            raise ValueError("llr must be float32 or float64")
        llr = llr.contiguous()
        B, L = llr.shape[0], int(list_size)
        dev = self.device
        res = SclResult(
            torch.empty((B, self.info_bytes), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.uint8, device=dev),
            torch.empty((B, L, self.info_bytes), dtype=torch.uint8, device=dev), torch.empty((B, L), dtype=torch.float64, device=dev),
            torch.empty((B, L), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev))   # every row is written by the kernel
        self._call("es_scl_batch", llr, dt, B, L, int(bool(skip_if_hard_ok)), res.hard_info, res.hard_ok, res.cand_info, res.cand_metric, res.cand_ok,
                   res.ncand)
        return res

    def softplus(self, t: torch.Tensor) -> torch.Tensor:
        """Diagnostic: log1p(exp(t)) for t <= 0 as the list decoder evaluates it on the device (float64 in, float64 out)."""
        t = t.contiguous()
        out = torch.empty_like(t)
        self._call("es_softplus_batch", t, t.numel(), out)
        return out

    def polar_f(self, a: torch.Tensor, b: torch.Tensor):
        """Diagnostic: f(a, b) and its two softplus terms as the lane-per-path list decoder's hot loops evaluate them on the device
        (float64 in; returns float64 [3, n] and the int32 out-of-range flag [n])."""
        a = a.contiguous(); b = b.contiguous()
        out = torch.empty((3, a.numel()), dtype=torch.float64, device=a.device)
        bad = torch.empty(a.numel(), dtype=torch.int32, device=a.device)
        self._call("es_polar_f_batch", a, b, a.numel(), out, bad)
        return out, bad

    def polar_encode(self, info: torch.Tensor) -> torch.Tensor:
        info = info.contiguous()
        B = info.shape[0]
        code = torch.empty((B, 1024), dtype=torch.uint8, device=self.device)
        self._call("es_polar_encode_batch", info, B, code)
        return code

    # ------------------------------------------------------------------ input conditioning
    def resample(self, audio, fs_orig: int, fs_target: int) -> torch.Tensor:
        """resample_to (rtwm/utils.py:58-66) on the device: 1-D or [B,n] signal -> the same values
        scipy.signal.resample_poly(audio, fs_target/g, fs_orig/g) returns (float32 for float32 input, else float64),
        bit for bit.  Equal rates return the input as a device tensor."""
        from .utils import resample_plan
        x = audio if torch.is_tensor(audio) else torch.as_tensor(np.asarray(audio))
        one_d = x.dim() == 1
        if one_d:
            x = x.reshape(1, -1)
        np_dtype = np.dtype(str(x.dtype).replace("torch.", ""))
        plan = resample_plan(x.shape[1], fs_target, fs_orig, np_dtype)
        if plan is None:
            out = x.to(self.device)
            return out[0] if one_d else out
        h_tf, hpp, up, down, y0, n_out, ctype = plan
        tdt = torch.float32 if ctype == np.float32 else torch.float64
        xd = self._dev(x, tdt)
        hd = torch.from_numpy(h_tf).to(self.device)
        out = torch.empty((x.shape[0], n_out), dtype=tdt, device=self.device)
        self._call("es_resample_batch", xd, nat.ES_DTYPE_F32 if tdt == torch.float32 else nat.ES_DTYPE_F64, x.shape[0], x.shape[1], hd, hpp, up, down, y0,
                   n_out, out)
        return out[0] if one_d else out

    def condition_upload(self, lengths, fs_list, fs_target: int, dtype) -> "DevicePlan":
        """utils.condition_plan with its descriptors and filter pool on the device: made once for a queue shape, it lets resample_ragged
        run without any host copy (device clips, plan=), e.g. inside a stream capture."""
        from .utils import condition_plan
        plan = condition_plan(lengths, fs_list, fs_target, dtype)
        filt = torch.from_numpy(plan.filters if plan.filters.size else np.zeros(1, plan.filters.dtype)).to(self.device, non_blocking=True)
        return DevicePlan(plan, filt, torch.from_numpy(plan.desc).to(self.device, non_blocking=True))

    def resample_ragged(self, clips, fs_list, fs_target: int, *, rep: int = 1, out: torch.Tensor | None = None, plan: "DevicePlan | None" = None):
        """resample_to for a group of clips of any lengths and rates in ONE launch (es_resample_ragged_batch): clips = 1-D host arrays
        or device tensors of ONE sample type (int16, float32 or float64), fs_list one rate or one per clip.  -> (rows float32
        [len(clips) * rep, stride], lens int64 host array): rows i * rep .. i * rep + rep - 1 all hold clip i conditioned to fs_target in
        their first lens[i] samples -- scipy.signal.resample_poly(x).astype(float32) bit for bit (int16 as x / 32768 first; equal rates:
        the samples themselves) --, the rest of a row is never written (new rows: zeros).  stride = the longest output rounded up to 4:
        the padded rows sync_ragged reads.  Host clips are uploaded once, unpadded; nothing comes back to the host.  plan = the
        condition_upload of these lengths, rates and sample type: fs_list and fs_target are then not looked at."""
        clips = list(clips)
        rep = int(rep)
        if rep < 1:
            raise ValueError("rep must be >= 1")
        ts = [c if torch.is_tensor(c) else torch.from_numpy(np.require(c, requirements=["C", "W"])) for c in clips]      # (a read-only array is copied)
        if any(t.dim() != 1 for t in ts):
            raise ValueError("resample_ragged takes 1-D clips")
        dtypes = {t.dtype for t in ts}
        if len(dtypes) > 1 or (dtypes and next(iter(dtypes)) not in _RESAMPLE_DTYPES):
            raise ValueError("resample_ragged: clips of one sample type, int16, float32 or float64")
        tdt = next(iter(dtypes)) if dtypes else torch.float32
        dt, np_dt = _RESAMPLE_DTYPES[tdt]
        if plan is None:
            plan = self.condition_upload([t.numel() for t in ts], fs_list, fs_target, np_dt)
        elif plan.plan.desc[:, 1].tolist() != [t.numel() for t in ts] or plan.filt.dtype != (torch.float64 if tdt == torch.float64 else torch.float32):
            raise ValueError("plan: made for other lengths or another sample type")
        filt, desc, plan = plan.filt, plan.desc, plan.plan
        lens = plan.n_out
        R = len(ts)
        longest = int(lens.max()) if R else 0
        stride = (longest + 3) // 4 * 4
        if out is None:
            out = torch.zeros((R * rep, stride), dtype=torch.float32, device=self.device)
        elif out.shape != (R * rep, stride) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out must be a contiguous float32 [{R * rep}, {stride}] tensor on the engine's device")
        if R == 0 or longest == 0:
            return out, lens
        if all(t.device == self.device for t in ts):
            pool = torch.cat(ts)                                            # device clips: gathered on the device
        else:
            pool = torch.cat([t.cpu() for t in ts]).to(self.device, non_blocking=True)      # ONE upload, unpadded
        self._call("es_resample_ragged_batch", pool, dt, pool.numel(), filt, filt.numel(), desc, R, rep, out, stride, longest)
        return out, lens

    # ------------------------------------------------------------------ key / PN / hop schedule
    def schedule(self, aes_key16: bytes, band_key32: bytes, ctrs=None, *, ctr0: int = 0, n: int | None = None):
        """PN rows and band indices of frame counters, derived on the device: -> (pn [n,152] uint8, band [n] uint8).
        `ctrs` (any integer sequence / tensor) or the range ctr0 .. ctr0+n-1.  aes_key16 = StreamPRNG.sub_key,
        band_key32 = the hop key (rtwm/utils.py:27-36, 115-132)."""
        if len(aes_key16) != 16 or len(band_key32) != 32:
            raise ValueError("schedule needs a 16-byte AES key and a 32-byte band key")
        if ctrs is not None:
            cd = self._ctr_dev(ctrs); n = cd.numel()
        elif n is None:
            raise ValueError("give ctrs or (ctr0, n)")
        else:
            cd = None
        pn = torch.empty((n, 152), dtype=torch.uint8, device=self.device)
        band = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call("es_schedule_batch", bytes(aes_key16), bytes(band_key32), cd, int(ctr0) & 0xFFFFFFFF, n, pn, band)
        return pn, band

    # ------------------------------------------------------------------ many keys at once (es_keyring.hip)
    def keyring(self, keys) -> KeyRing:
        """The key ring of 32-byte master keys (a sequence of bytes objects, or uint8 [N, 32]), derived on the device (a KeyRing: itself)."""
        if isinstance(keys, KeyRing):
            return keys
        if torch.is_tensor(keys):
            mk = keys
        else:
            keys = [bytes(k) for k in keys]
            if any(len(k) != 32 for k in keys):
                raise ValueError("master_key must be 32 bytes (256 bit)")
            mk = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 32).copy())
        mk = self._dev(mk, torch.uint8)
        if mk.dim() != 2 or mk.shape[1] != 32:
            raise ValueError("keys must be 32 bytes each")
        N = mk.shape[0]
        ring = torch.empty((N, nat.ES_KEYRING_BYTES), dtype=torch.uint8, device=self.device)
        self._call("es_keyring_derive_batch", mk, N, ring)
        return KeyRing(ring, N)

    @staticmethod
    def _key_host(ring: KeyRing, key_idx) -> np.ndarray:
        """Key indices as int64 on the host (a device tensor is copied), each a row of the ring."""
        h = np.asarray(key_idx.cpu().numpy() if torch.is_tensor(key_idx) else key_idx, dtype=np.int64).reshape(-1)
        if h.size and (h.min() < 0 or h.max() >= ring.n):
            raise ValueError(f"key index outside [0, {ring.n})")
        return h

    def _key_dev(self, ring: KeyRing, key_idx, n: int) -> torch.Tensor:
        """Key indices as int32 on the device; indices the host can see (anything but a device tensor) are range-checked here."""
        if not (torch.is_tensor(key_idx) and key_idx.is_cuda):
            key_idx = torch.from_numpy(self._key_host(ring, key_idx))
        kd = self._dev(key_idx, torch.int32).reshape(-1)
        if kd.numel() != n:
            raise ValueError("one key index per record is required")
        return kd

    def schedule_keyed(self, ring: KeyRing, key_idx, ctrs, *, want_pn: bool = True, want_band: bool = True):
        """`schedule` for records of several keys (es_schedule_keyed_batch): record i = (ring row key_idx[i], counter ctrs[i])
        -> (pn [n,152] uint8 or None, band [n] uint8 or None).  want_pn=False skips the AES blocks (bands only)."""
        cd = self._ctr_dev(ctrs).reshape(-1)
        n = cd.numel()
        kd = self._key_dev(ring, key_idx, n)
        pn = torch.empty((n, 152), dtype=torch.uint8, device=self.device) if want_pn else None
        band = torch.empty(n, dtype=torch.uint8, device=self.device) if want_band else None
        if n and ring.n == 0:
            raise ValueError("records but an empty key ring")
        self._call("es_schedule_keyed_batch", ring.ring, ring.n, kd, cd, n, pn, band)
        return pn, band

    def aead_check_keyed(self, ring: KeyRing, key_idx, blobs: torch.Tensor, ctrs, *, want_plain: bool = False):
        """`aead_check` with the AEAD key of ring row key_idx[r] per row (per frame for [B,L,55]) (es_aead_check_keyed_batch)."""
        if blobs.dtype != torch.uint8 or blobs.shape[-1] != 55 or blobs.dim() not in (2, 3):
            raise ValueError("blobs must be uint8 [n,55] or [B,L,55]")
        blobs = self._dev(blobs, torch.uint8)
        group = blobs.shape[1] if blobs.dim() == 3 else 1
        n = blobs.numel() // 55
        ctrs = self._ctr_dev(ctrs).reshape(-1)
        if ctrs.numel() * group != n:
            raise ValueError("one expected counter per blob row (or per frame for [B,L,55]) is required")
        kd = self._key_dev(ring, key_idx, ctrs.numel())
        ok = torch.empty(blobs.shape[:-1], dtype=torch.uint8, device=self.device)
        plain = torch.empty(blobs.shape[:-1] + (27,), dtype=torch.uint8, device=self.device) if want_plain else None
        self._call("es_aead_check_keyed_batch", ring.ring, ring.n, kd, blobs, n, group, ctrs, ok, plain)
        return (ok, plain) if want_plain else ok

    def hop_window(self, ring: KeyRing, hop_base, C: int) -> torch.Tensor:
        """Hop rows filled on the device (es_hop_window_batch): -> uint8 [N, HR, C], entry (k, h, col) = band of counter hop_base[h] + col
        under key k of the ring, 0xFF where that counter lies past 2^32 - 1.  hop_base: HR counters in [0, 2^32) (host values or a
        tensor); nothing but them is uploaded."""
        base = self._ctr_dev(hop_base).reshape(-1)
        HR, C = base.numel(), int(C)
        if C < 0:
            raise ValueError("C: a column count")
        hop = torch.empty((ring.n, HR, C), dtype=torch.uint8, device=self.device)
        self._call("es_hop_window_batch", ring.ring, ring.n, base, HR, C, hop)
        return hop

    # ------------------------------------------------------------------ presence (include/echoseal_presence.h)
    def _presence_rows(self, corr: torch.Tensor, nlag):
        """The correlation rows of a presence call, checked: -> (corr, rows, stride, nlag int32 [B] on the device, B)."""
        if corr.dim() != 2 or corr.dtype != torch.float64 or not corr.is_contiguous() or corr.device != self.device:
            raise ValueError("corr must be a contiguous float64 [rows, stride] tensor on the engine's device")
        nlag = self._dev(nlag, torch.int32).reshape(-1)
        if 4 * nlag.numel() > corr.shape[0]:
            raise ValueError("corr: four rows per clip, row 4 * clip + band")
        return corr, corr.shape[0], corr.shape[1], nlag, nlag.numel()

    def _score_io(self, hop: torch.Tensor, B: int, n_origins):
        """The hop rows of a score call, checked, and what the call writes: -> (hop uint8 [K, Ccols], K, n_origins, score, origin, rank,
        scratch)."""
        if hop.dim() == 3 and hop.shape[1] == 1:
            hop = hop[:, 0, :]
        if hop.dim() != 2 or hop.dtype != torch.uint8:
            raise ValueError("hop must be uint8 [K, Ccols]")
        hop = hop.contiguous()
        K, n_origins = hop.shape[0], int(n_origins)
        score = torch.empty((B, K), dtype=torch.float64, device=self.device)
        origin = torch.empty((B, K), dtype=torch.int64, device=self.device)
        rank = torch.empty((B, K), dtype=torch.int32, device=self.device)
        chunks = -(-max(n_origins, 0) // nat.ES_HOP_ORIGINS)
        scratch = torch.empty(3 * B * K * chunks, dtype=torch.int64, device=self.device)      # the workgroups' bests: 24 bytes each
        return hop, K, n_origins, score, origin, rank, scratch

    def phase_fold(self, corr: torch.Tensor, nlag) -> torch.Tensor:
        """The keyless fold of a presence test (es_phase_fold_batch; presence.fold_model is the host twin): corr float64 [rows, stride],
        row 4 * clip + band the correlation row of BAND_PLAN band `band`, nlag [B] the lags of each clip (clamped to [0, stride]; columns
        past them are never read) -> fold float64 [B, 1215], fold[b, phi] = sum over the clip's whole slots j of the largest of its four
        rows at lag phi + 1215 j."""
        corr, rows, stride, nlag, B = self._presence_rows(corr, nlag)
        fold = torch.empty((B, nat.ES_FRAME_LEN), dtype=torch.float64, device=self.device)
        self._call("es_phase_fold_batch", corr, rows, stride, nlag, B, fold)
        return fold

    def hop_score(self, corr: torch.Tensor, nlag, phases, hop: torch.Tensor, n_origins: int):
        """The keyed score of a presence test (es_hop_score_batch; presence.score_model is the host twin).  corr, nlag as for phase_fold;
        phases int [B, P], 1 <= P <= 1215: each clip's phase list; hop uint8 [K, Ccols] (or hop_window's [K, 1, Ccols]): column i = the
        band of counter lo + i under key row k, Ccols >= n_origins + stride // 1215 - 1; origins 0 .. n_origins - 1 are searched
        -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K]): per (clip, key) the largest mean of the rows the key hops
        through, the origin (counter - lo) and the list entry it was found at; (-inf, -1, -1) where nothing was scored."""
        corr, rows, stride, nlag, B = self._presence_rows(corr, nlag)
        phases = self._dev(phases, torch.int32)
        if phases.dim() != 2 or phases.shape[0] != B:
            raise ValueError("phases: int [B, P], one list per clip")
        hop, K, n_origins, score, origin, rank, scratch = self._score_io(hop, B, n_origins)
        self._call("es_hop_score_batch", corr, rows, stride, nlag, B, phases, phases.shape[1], hop, K, hop.shape[1], n_origins, score, origin, rank,
                   scratch if scratch.numel() else None)
        return score, origin, rank

    # ------------------------------------------------------------------ the coherent presence test (include/echoseal_coherent.h)
    def mf_rows(self, y: torch.Tensor, lens, bands, *, out=None):
        """The keyless rows of the coherent presence test (es_mf_rows_batch; presence.mf_rows_model is the host twin): y float64
        [rows, T] band-passed records (bpf, or sync_ragged's y), lens [rows] the samples of each (clamped to [0, T]; nothing at or past
        them is read), bands [rows] their BAND_PLAN indices -> (M, A, D) float64 [rows, T]: the matched-filter row, the preamble sum at
        every start and its normaliser, written where they are defined (M: t + L <= len; A, D: s + 190 + L <= len) and nowhere else.
        out: three tensors to write into (what is not defined keeps its value); new ones are zero-filled."""
        if y.dim() != 2 or y.dtype != torch.float64 or not y.is_contiguous() or y.device != self.device:
            raise ValueError("y must be a contiguous float64 [rows, T] tensor on the engine's device")
        rows, T = y.shape
        lens, bands = self._lens(lens, rows), self._dev(bands, torch.uint8).reshape(-1)
        if bands.numel() != rows:
            raise ValueError("bands: one band index per row")
        M, A, D = out if out is not None else (torch.zeros((rows, T), dtype=torch.float64, device=self.device) for _ in range(3))
        if any(t.shape != (rows, T) or t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device for t in (M, A, D)):
            raise ValueError("out: three contiguous float64 [rows, T] tensors on the engine's device")
        self._call("es_mf_rows_batch", y, rows, T, lens, bands, M, A, D)
        return M, A, D

    def coherent_score(self, M: torch.Tensor, A: torch.Tensor, D: torch.Tensor, nslot, phases, ring: KeyRing, hop: torch.Tensor, lo: int,
                       n_origins: int):
        """The keyed score of the coherent presence test (es_coherent_score_batch; presence.coherent_score_model is the host twin).
        M, A, D: mf_rows' three [rows, T] tensors, clip b in rows 4 b .. 4 b + 3 in BAND_PLAN order; nslot [B] the slots J of each clip
        (presence.coherent_slots; clamped to (T - 190) // 1215); phases int [B, P], 1 <= P <= 1215; ring: the K keys, whose header PN
        signs the header sums; hop uint8 [K, Ccols] (or hop_window's [K, 1, Ccols]): column i = the band of counter lo + i under key row
        k, Ccols >= n_origins + max(0, T - 190) // 1215 - 1; lo: the counter of column 0; origins 0 .. n_origins - 1 are searched
        -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K]) as hop_score gives them."""
        for t in (M, A, D):
            if t.dim() != 2 or t.shape != M.shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("M, A, D must be contiguous float64 [rows, T] tensors of one shape on the engine's device")
        nslot = self._dev(nslot, torch.int32).reshape(-1)
        B = nslot.numel()
        if 4 * B > M.shape[0]:
            raise ValueError("M, A, D: four rows per clip, row 4 * clip + band")
        phases = self._dev(phases, torch.int32)
        if phases.dim() != 2 or phases.shape[0] != B:
            raise ValueError("phases: int [B, P], one list per clip")
        if not 0 <= int(lo) < 1 << 32:
            raise ValueError("lo: the counter of hop column 0, in [0, 2^32)")
        hop, K, n_origins, score, origin, rank, scratch = self._score_io(hop, B, n_origins)
        if K != ring.n:
            raise ValueError("hop: one row per key of the ring")
        self._call("es_coherent_score_batch", M, A, D, M.shape[0], M.shape[1], nslot, B, phases, phases.shape[1], ring.ring, hop, K, hop.shape[1],
                   int(lo), n_origins, score, origin, rank, scratch if scratch.numel() else None)
        return score, origin, rank

    def coherent_score_at(self, M: torch.Tensor, A: torch.Tensor, D: torch.Tensor, rows4, col, nslot, phases, ring: KeyRing, hop: torch.Tensor,
                          hop_row, lo, n_origins: int):
        """coherent_score over records that lie anywhere in the three tables (es_coherent_score_at_batch, include/echoseal_coherent_at.h;
        presence.coherent_score_at_model is the host twin).  M, A, D: mf_rows' three [rows, stride] tensors; rows4 int
        [B, 4]: rows4[b, band] the row that holds BAND_PLAN band `band` of record b; col [B] the column of its sample 0; nslot [B] its
        slots (clamped to (stride - col - 190) // 1215; a record with a row or a column outside the tables has none; Jw is the largest
        of them).  Nothing outside columns [col, col + 1215 J + 190) of a record's own rows is read; records may share rows and overlap.
        phases int [B, P]; ring: the K keys; hop uint8 [K, HR, Ccols] as hop_window gives it ([K, Ccols]: one hop row),
        Ccols >= n_origins + Jw - 1; hop_row int [B]: record b reads hop row hop_row[b] of every key, one outside [0, HR) scores
        nothing; lo [B]: the counter of column 0 of that hop row, in [0, 2^32) -> (score float64 [B, K], origin int64 [B, K], rank
        int32 [B, K]) as coherent_score gives them."""
        for t in (M, A, D):
            if t.dim() != 2 or t.shape != M.shape or t.dtype != torch.float64 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("M, A, D must be contiguous float64 [rows, stride] tensors of one shape on the engine's device")
        rows4 = self._dev(rows4, torch.int64)
        nslot = torch.as_tensor(nslot).reshape(-1)
        Jw = max(int(nslot.max()), 0) if nslot.numel() else 0               # read where the values are: host values cost no sync
        col, nslot = self._dev(col, torch.int64).reshape(-1), self._dev(nslot, torch.int32)
        B = nslot.numel()
        if rows4.dim() != 2 or tuple(rows4.shape) != (B, 4) or col.numel() != B:
            raise ValueError("rows4: int [B, 4], the row of each band of each record; col, nslot: one value per record")
        phases = self._dev(phases, torch.int32)
        if phases.dim() != 2 or phases.shape[0] != B:
            raise ValueError("phases: int [B, P], one list per record")
        if hop.dim() == 2:
            hop = hop[:, None, :]
        if hop.dim() != 3 or hop.dtype != torch.uint8:
            raise ValueError("hop must be uint8 [K, HR, Ccols]")
        HR, Ccols = hop.shape[1], hop.shape[2]
        hop_row, lo = self._dev(hop_row, torch.int32).reshape(-1), self._ctr_dev(lo).reshape(-1)
        if hop_row.numel() != B or lo.numel() != B:
            raise ValueError("hop_row, lo: one hop row index and one counter per record")
        hop, K, n_origins, score, origin, rank, scratch = self._score_io(hop.reshape(hop.shape[0], HR * Ccols), B, n_origins)
        if K != ring.n:
            raise ValueError("hop: one row per key of the ring")
        self._call("es_coherent_score_at_batch", M, A, D, M.shape[0], M.shape[1], rows4, col, nslot, B, Jw, phases, phases.shape[1], ring.ring, hop,
                   K, HR, Ccols, hop_row, lo, n_origins, score, origin, rank, scratch if scratch.numel() else None)
        return score, origin, rank

    # ------------------------------------------------------------------ presence under clock drift (include/echoseal_warp.h)
    def _warp_table(self, warp, nwarp, nslot, B: int):
        """The table of per-slot offsets of a warp call, checked: -> (warp int32 [B, D, Jw], nwarp int32 [B], nslot int32 [B], D, Jw)."""
        warp = self._dev(warp, torch.int32)
        nwarp, nslot = self._dev(nwarp, torch.int32).reshape(-1), self._dev(nslot, torch.int32).reshape(-1)
        if warp.dim() != 3 or warp.shape[0] != B or nwarp.numel() != B or nslot.numel() != B:
            raise ValueError("warp: int [B, D, Jw] with nwarp [B] rows and nslot [B] slots per clip")
        return warp, nwarp, nslot, warp.shape[1], warp.shape[2]

    def warp_fold(self, corr: torch.Tensor, nlag, warp, nwarp, nslot) -> torch.Tensor:
        """phase_fold along a table of per-slot offsets (es_warp_fold_batch; presence.warp_fold_model is the host twin).  corr, nlag as
        for phase_fold; warp int [B, D, Jw]: slot j of row d of clip b starts warp[b, d, j] samples after 1215 j; nwarp [B] the rows
        and nslot [B] the slots of each clip (clamped to [0, min(Jw, nlag // 1215)]) -> fold float64 [B, D, 1215]; a row at or past
        nwarp, or one with a slot that does not lie whole inside the clip's lags, is all -inf and is never read."""
        corr, rows, stride, nlag, B = self._presence_rows(corr, nlag)
        warp, nwarp, nslot, D, Jw = self._warp_table(warp, nwarp, nslot, B)
        fold = torch.empty((B, D, nat.ES_FRAME_LEN), dtype=torch.float64, device=self.device)
        self._call("es_warp_fold_batch", corr, rows, stride, nlag, B, warp if warp.numel() else None, nwarp, nslot, D, Jw, fold)
        return fold

    def warp_score(self, corr: torch.Tensor, nlag, warp, nwarp, nslot, hyp, hop: torch.Tensor, n_origins: int):
        """hop_score along a table of per-slot offsets (es_warp_score_batch; presence.warp_score_model is the host twin).  corr, nlag,
        warp, nwarp, nslot as for warp_fold; hyp int [B, H, 2], H >= 1: entry h of clip b is (row d, phase phi); hop uint8 [K, Ccols]
        (or hop_window's [K, 1, Ccols]) with Ccols >= n_origins + Jw - 1 -> (score float64 [B, K], origin int64 [B, K], rank int32
        [B, K]) as hop_score gives them, rank the list entry; an entry that names no usable row or no phase is not scored."""
        corr, rows, stride, nlag, B = self._presence_rows(corr, nlag)
        warp, nwarp, nslot, D, Jw = self._warp_table(warp, nwarp, nslot, B)
        hyp = self._dev(hyp, torch.int32)
        if hyp.dim() != 3 or hyp.shape[0] != B or hyp.shape[2] != 2:
            raise ValueError("hyp: int [B, H, 2], a list of (row, phase) per clip")
        hop, K, n_origins, score, origin, rank, scratch = self._score_io(hop, B, n_origins)
        self._call("es_warp_score_batch", corr, rows, stride, nlag, B, warp if warp.numel() else None, nwarp, nslot, D, Jw, hyp, hyp.shape[1],
                   hop, K, hop.shape[1], n_origins, score, origin, rank, scratch if scratch.numel() else None)
        return score, origin, rank

    # ------------------------------------------------------------------ presence of records anywhere in a table of rows (DESIGN 4.25;
    # include/echoseal_live_presence.h)
    def _presence_records(self, corr: torch.Tensor, rows4, col, nlag):
        """The table of rows and the records of an _at call, checked: -> (corr, rows, stride, rows4 int64 [B, 4], col int64 [B], nlag int32
        [B], B).  What the arrays hold is the kernels' to judge: a record that names a row or a column outside the table has no lags."""
        if corr.dim() != 2 or corr.dtype != torch.float64 or not corr.is_contiguous() or corr.device != self.device:
            raise ValueError("corr must be a contiguous float64 [rows, stride] tensor on the engine's device")
        rows4 = self._dev(rows4, torch.int64)
        col, nlag = self._dev(col, torch.int64).reshape(-1), self._dev(nlag, torch.int32).reshape(-1)
        B = nlag.numel()
        if rows4.dim() != 2 or tuple(rows4.shape) != (B, 4) or col.numel() != B:
            raise ValueError("rows4: int [B, 4], the row of each band of each record; col, nlag: one value per record")
        return corr, corr.shape[0], corr.shape[1], rows4, col, nlag, B

    def warp_fold_at(self, corr: torch.Tensor, rows4, col, nlag, warp, nwarp, nslot) -> torch.Tensor:
        """warp_fold over records that lie anywhere in a table of rows (es_warp_fold_at_batch; presence.window_rows + warp_fold_model is the
        host twin).  corr float64 [rows, stride]; rows4 int [B, 4]: rows4[b, band] the row that holds BAND_PLAN band `band` of record b;
        col [B] the column of its lag 0; nlag [B] its lags (clamped to [0, stride - col]; a record with a row or a column outside the table
        has none).  Nothing outside columns [col, col + nlag) of a record's own rows is read; records may share rows and overlap.  warp,
        nwarp, nslot as for warp_fold -> fold float64 [B, D, 1215]."""
        corr, rows, stride, rows4, col, nlag, B = self._presence_records(corr, rows4, col, nlag)
        warp, nwarp, nslot, D, Jw = self._warp_table(warp, nwarp, nslot, B)
        fold = torch.empty((B, D, nat.ES_FRAME_LEN), dtype=torch.float64, device=self.device)
        self._call("es_warp_fold_at_batch", corr, rows, stride, rows4, col, nlag, B, warp if warp.numel() else None, nwarp, nslot, D, Jw, fold)
        return fold

    def warp_score_at(self, corr: torch.Tensor, rows4, col, nlag, warp, nwarp, nslot, hyp, hop: torch.Tensor, hop_row, n_origins: int):
        """warp_score over records that lie anywhere in a table of rows (es_warp_score_at_batch; presence.window_rows + warp_score_model on
        the record's hop row is the host twin).  corr, rows4, col, nlag as for warp_fold_at; warp, nwarp, nslot, hyp as for warp_score; hop
        uint8 [K, HR, Ccols] as hop_window gives it ([K, Ccols]: one hop row), Ccols >= n_origins + Jw - 1; hop_row int [B]: record b
        reads hop row hop_row[b] of every key, one outside [0, HR) scores nothing -> (score float64 [B, K], origin int64 [B, K], rank
        int32 [B, K])."""
        corr, rows, stride, rows4, col, nlag, B = self._presence_records(corr, rows4, col, nlag)
        warp, nwarp, nslot, D, Jw = self._warp_table(warp, nwarp, nslot, B)
        hyp = self._dev(hyp, torch.int32)
        if hyp.dim() != 3 or hyp.shape[0] != B or hyp.shape[2] != 2:
            raise ValueError("hyp: int [B, H, 2], a list of (row, phase) per record")
        if hop.dim() == 2:
            hop = hop[:, None, :]
        if hop.dim() != 3 or hop.dtype != torch.uint8:
            raise ValueError("hop must be uint8 [K, HR, Ccols]")
        HR, Ccols = hop.shape[1], hop.shape[2]
        hop_row = self._dev(hop_row, torch.int32).reshape(-1)
        if hop_row.numel() != B:
            raise ValueError("hop_row: one hop row index per record")
        hop, K, n_origins, score, origin, rank, scratch = self._score_io(hop.reshape(hop.shape[0], HR * Ccols), B, n_origins)
        self._call("es_warp_score_at_batch", corr, rows, stride, rows4, col, nlag, B, warp if warp.numel() else None, nwarp, nslot, D, Jw, hyp,
                   hyp.shape[1], hop, K, HR, Ccols, hop_row, n_origins, score, origin, rank, scratch if scratch.numel() else None)
        return score, origin, rank

    # ------------------------------------------------------------------ the hypothesis list on the device (include/echoseal_pick.h)
    def fold_pick(self, fold: torch.Tensor, nwarp=None, H: int = 8, *, want_val: bool = True):
        """The hypothesis list of each record of a fold, picked on the device (es_fold_pick_batch; presence.pick_model is the host twin).
        fold float64 [B, D, 1215] as warp_fold / warp_fold_at give it ([B, 1215], phase_fold's: D = 1); nwarp [B] the rows of each
        record (None: D; clamped to [0, D]; rows past them are never read); 1 <= H <= ES_PICK_MAX_H -> (hyp int32 [B, H, 2], val float64
        [B, H]): entry h the (row, phase) of h-th largest value, equal values by the lower row, then the lower phase; -inf and NaN are
        never picked; (-1, -1) and -inf from the first entry past a record's last candidate -- the form warp_score / warp_score_at take
        for "an entry that names nothing".  want_val=False: val is None and is not written.  B * D == 0 enqueues nothing: every list is
        empty, and the outputs are filled here."""
        if fold.dim() == 2:
            fold = fold[:, None, :]
        if fold.dim() != 3 or fold.shape[2] != nat.ES_FRAME_LEN or fold.dtype != torch.float64 or not fold.is_contiguous() or fold.device != self.device:
            raise ValueError("fold must be a contiguous float64 [B, D, 1215] tensor on the engine's device")
        B, D, H = fold.shape[0], fold.shape[1], int(H)
        if not 1 <= H <= nat.ES_PICK_MAX_H:
            raise ValueError(f"H = {H}: a list of 1 .. {nat.ES_PICK_MAX_H} entries")
        if nwarp is not None:
            nwarp = self._dev(nwarp, torch.int32).reshape(-1)
            if nwarp.numel() != B:
                raise ValueError("nwarp: one row count per record")
        if B * D == 0:
            return (torch.full((B, H, 2), -1, dtype=torch.int32, device=self.device),
                    torch.full((B, H), float("-inf"), dtype=torch.float64, device=self.device) if want_val else None)
        hyp = torch.empty((B, H, 2), dtype=torch.int32, device=self.device)
        val = torch.empty((B, H), dtype=torch.float64, device=self.device) if want_val else None
        self._call("es_fold_pick_batch", fold, B, D, nwarp, H, hyp, val)
        return hyp, val

    def acquire_mask(self, ring: KeyRing, key_idx, ok, lo16, band, span):
        """Which counters of `span` each header record may belong to (es_acquire_mask_batch; acquire.mask_model is the host twin).
        Record p = (ring row key_idx[p] int32, ok[p] uint8, lo16[p] int32, band[p] uint8), as one header call gives them
        -> (mask int32 [P, W] holding the uint32 words, count int32 [P]); bit h - h0 of row p: (h << 16) | lo16[p] is a candidate."""
        from .acquire import span_words
        lo, hi = span
        _, _, W = span_words(span)
        kd, okd = self._dev(key_idx, torch.int32).reshape(-1), self._dev(ok, torch.uint8).reshape(-1)
        lod, bd = self._dev(lo16, torch.int32).reshape(-1), self._dev(band, torch.uint8).reshape(-1)
        P = kd.numel()
        if not (okd.numel() == lod.numel() == bd.numel() == P):
            raise ValueError("key_idx, ok, lo16, band: one entry per record")
        mask = torch.empty((P, W), dtype=torch.int32, device=self.device)
        count = torch.empty(P, dtype=torch.int32, device=self.device)
        self._call("es_acquire_mask_batch", ring.ring, ring.n, kd, okd, lod, bd, P, int(lo), int(hi), mask, count)
        return mask, count

    def acquire_list(self, mask: torch.Tensor, lo16, span, base, total: int):
        """The set bits of acquire_mask's rows as a flat list (es_acquire_list_batch): record p with base[p] >= 0 fills entries base[p] ..
        of -> (cand_rec int32 [total], cand_ctr int32 [total] holding the uint32 counters), its counters ascending; base[p] < 0 skips
        the record.  base (int64 [P]) and total are the host's choice, made from acquire_mask's counts."""
        lo, hi = span
        P, total = mask.shape[0], int(total)
        from .acquire import span_words
        if mask.dim() != 2 or mask.dtype != torch.int32 or mask.shape[1] != span_words(span)[2]:
            raise ValueError("mask: the int32 [P, W] output of acquire_mask over the same span")
        mask, lod, based = mask.contiguous(), self._dev(lo16, torch.int32).reshape(-1), self._dev(base, torch.int64).reshape(-1)
        if lod.numel() != P or based.numel() != P or total < 0:
            raise ValueError("lo16, base: one entry per record; total: an entry count")
        rec = torch.empty(total, dtype=torch.int32, device=self.device)
        ctr = torch.empty(total, dtype=torch.int32, device=self.device)
        self._call("es_acquire_list_batch", mask, lod, P, int(lo), int(hi), based, total, rec, ctr)
        return rec, ctr

    def plan(self, peaks: torch.Tensor, npeaks: torch.Tensor, rowband, hdr_base, T, hdr_ok: torch.Tensor, hdr_lo16: torch.Tensor,
             hop: torch.Tensor, *, pos0=None, ctr0=None, hop_row=None, hop_base=None) -> PlanResult:
        """Counter candidates of every (key, row) in try order (es_plan_batch; the rules of _scan_band_multi_frame,
        rtwm/detector.py:105-142).  peaks int32 [rows, 32] / npeaks int32 [rows] of a sync call over records of T samples -- an int, or
        for the rows of a sync_ragged call their sample counts, an integer tensor / array [rows] (es_plan_ragged_batch) --, rowband
        uint8 [rows] their bands, hdr_base int32 [rows] = index of the row's first fitting peak among the P fitting peaks of all
        rows, hdr_ok uint8 / hdr_lo16 int32 [N, P] header results per (key, fitting peak), hop uint8 [N, C] band of (key, counter).
        With any of pos0 / ctr0 / hop_row / hop_base (es_plan_at_batch): row r starts at absolute sample pos0[r] (default 0) of a
        stream whose counters start at ctr0[r] (default 0), hop is uint8 [N, HR, C] (hop_window), the row reads hop row hop_row[r]
        (default 0), whose column 0 is counter hop_base[hop_row[r]] (default 0); T may be an int or per row."""
        rows = peaks.shape[0]
        if peaks.dim() != 2 or peaks.shape[1] != nat.ES_MAX_PEAKS or peaks.dtype != torch.int32 or npeaks.dtype != torch.int32 or npeaks.numel() != rows:
            raise ValueError("peaks / npeaks: the int32 [rows, 32] / [rows] outputs of a sync call")
        at = not (pos0 is None and ctr0 is None and hop_row is None and hop_base is None)
        if at and hop.dim() == 2:
            hop = hop[:, None, :]
        if hop.dim() != (3 if at else 2) or hop.dtype != torch.uint8:
            raise ValueError("hop must be uint8 [N, HR, C]" if at else "hop must be uint8 [N, C]")
        N, C = hop.shape[0], hop.shape[-1]
        if hdr_ok.dtype != torch.uint8 or hdr_lo16.dtype != torch.int32 or hdr_ok.shape != hdr_lo16.shape or hdr_ok.dim() != 2 or hdr_ok.shape[0] != N:
            raise ValueError("hdr_ok uint8 / hdr_lo16 int32 must be [N, P]")
        P = hdr_ok.shape[1]
        peaks = peaks.contiguous(); npeaks = npeaks.contiguous(); hop = hop.contiguous()
        hdr_ok = hdr_ok.contiguous(); hdr_lo16 = hdr_lo16.contiguous()
        rowband = self._dev(rowband, torch.uint8).reshape(-1)
        hdr_base = self._dev(hdr_base, torch.int32).reshape(-1)
        if rowband.numel() != rows or hdr_base.numel() != rows:
            raise ValueError("rowband / hdr_base: one entry per row")
        pairs = N * rows
        res = PlanResult(torch.empty((pairs, nat.ES_MAX_TRIES), dtype=torch.uint8, device=self.device),
                         torch.empty((pairs, nat.ES_MAX_TRIES), dtype=torch.int32, device=self.device),
                         torch.empty(pairs, dtype=torch.int32, device=self.device), torch.empty(pairs, dtype=torch.int32, device=self.device))
        row_args = (peaks, npeaks, rowband, hdr_base, rows)         # the three argument groups every arm passes, in the header's order
        key_args = (hdr_ok, hdr_lo16, P, hop, N, C)
        out = (res.slot, res.ctr, res.count, res.looked)
        if at:
            HR = hop.shape[1]
            def per_row(v, n, what, counter=False):                 # one value, or one per row / hop row; None: zeros
                v = np.zeros(n, np.int64) if v is None else v
                t = (self._ctr_dev(v) if counter else self._dev(v, torch.int64)).reshape(-1)
                if t.numel() == 1 and n != 1:
                    t = t.expand(n)
                if t.numel() != n:
                    raise ValueError(f"{what}: one entry, or {n}")
                return t.contiguous()
            pos0_d, ctr0_d = per_row(pos0, rows, "pos0"), per_row(ctr0, rows, "ctr0", True)
            hrow_d, hbase_d = per_row(hop_row, rows, "hop_row").to(torch.int32), per_row(hop_base, HR, "hop_base", True)
        ragged = torch.is_tensor(T) or isinstance(T, np.ndarray)
        if ragged:
            t_max, lens = (int(T.max()) if rows else 0), self._lens(T, rows)      # (t_max: the bound on the hop table's width)
        elif at:
            t_max, lens = int(T), torch.full((rows,), int(T), dtype=torch.int32, device=self.device)
        if at:
            self._call("es_plan_at_batch", *row_args, lens, t_max, *key_args, pos0_d, ctr0_d, hrow_d, hbase_d, HR, *out)
        elif ragged:
            self._call("es_plan_ragged_batch", *row_args, lens, t_max, *key_args, *out)
        else:
            self._call("es_plan_batch", *row_args, int(T), *key_args, *out)
        return res

    # ------------------------------------------------------------------ the verdict memo (es_memo.hip)
    def open_memo(self, slots: int) -> Memo:
        """An empty memo of `slots` entries (a power of two): 16 bytes of table and 4 of claim word per entry."""
        from .memo import check_slots
        slots = check_slots(slots)
        return Memo(torch.full((slots, 2), -1, dtype=torch.int64, device=self.device), torch.full((slots,), -1, dtype=torch.int32, device=self.device), slots)

    def _memo_words(self, k0, k1):
        """Packed records as int64 device tensors: uint64 host arrays (memo.pack) are reinterpreted, device tensors are taken as they are."""
        w = [t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint64).view(np.int64)) for t in (k0, k1)]
        w = [self._dev(t, torch.int64).reshape(-1) for t in w]
        if w[0].numel() != w[1].numel():
            raise ValueError("memo records: one k0 and one k1 word per record")
        return w[0], w[1], w[0].numel()

    def memo_probe(self, memo: Memo, k0, k1) -> torch.Tensor:
        """-> uint8 [n]: record i is in the memo (es_memo_probe_batch)."""
        k0, k1, n = self._memo_words(k0, k1)
        hit = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call("es_memo_probe_batch", memo.table, memo.slots, k0, k1, n, hit)
        return hit

    def memo_insert(self, memo: Memo, k0, k1) -> None:
        """Store the records of one call (es_memo_insert_batch): per entry the record of the lowest index wins, a record whose k0 is all
        ones is ignored."""
        k0, k1, n = self._memo_words(k0, k1)
        self._call("es_memo_insert_batch", memo.table, memo.claim, memo.slots, k0, k1, n)

    # ------------------------------------------------------------------ after the list decoder
    def _ctr_dev(self, ctrs) -> torch.Tensor:
        """Frame counters as the 32-bit words the kernels compare against (stored in an int32 tensor)."""
        t = self._dev(ctrs, torch.int64) & 0xFFFFFFFF
        return torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32).contiguous()

    def aead_check(self, key32: bytes, blobs: torch.Tensor, ctrs: torch.Tensor, *, want_plain: bool = False):
        """The detector's validator (rtwm/detector.py:168-176) on 55-byte blobs: [n,55] or [B,L,55] uint8 with
        one expected counter per row / per B.  -> ok uint8 (same leading shape), optionally plaintext [...,27]."""
        if len(key32) != 32:
            raise ValueError("AEAD key must be 32 bytes")
        if blobs.dtype != torch.uint8 or blobs.shape[-1] != 55 or blobs.dim() not in (2, 3):
            raise ValueError("blobs must be uint8 [n,55] or [B,L,55]")
        blobs = blobs.contiguous()
        group = blobs.shape[1] if blobs.dim() == 3 else 1
        n = blobs.numel() // 55
        ctrs = self._ctr_dev(ctrs)
        if ctrs.numel() * group != n:
            raise ValueError("one expected counter per blob row (or per frame for [B,L,55]) is required")
        ok = torch.empty(blobs.shape[:-1], dtype=torch.uint8, device=self.device)
        plain = torch.empty(blobs.shape[:-1] + (27,), dtype=torch.uint8, device=self.device) if want_plain else None
        self._call("es_aead_check_batch", bytes(key32), blobs, n, group, ctrs, ok, plain)
        return (ok, plain) if want_plain else ok

    def select(self, scl: SclResult, *, key32: bytes | None = None, ctrs: torch.Tensor | None = None, ring: KeyRing | None = None,
               key_idx=None):
        """Tail of PolarCode.decode (rtwm/fastpolar.py:268-276, 332-359) for every record of an SclResult, on the
        GPU: -> (payload [B,55] uint8, ok [B] int8, which [B] int32).  key32=None is validator=None; with a key the
        validator is `aead_check` against ctrs [B].  ok = -1 marks records whose list loop had been skipped.
        ring= with key_idx= [B]: the validator of record i uses the AEAD key of ring row key_idx[i] (es_select_keyed_batch)."""
        B, L = scl.cand_metric.shape
        if ring is not None:
            if key32 is not None or key_idx is None or ctrs is None:
                raise ValueError("ring= goes with key_idx= and ctrs=, and without key32=")
        elif key_idx is not None:
            raise ValueError("key_idx= goes with ring=")
        elif key32 is not None:
            if len(key32) != 32:
                raise ValueError("AEAD key must be 32 bytes")
            if ctrs is None:
                raise ValueError("one expected counter per record is required with a key")
        keyed = ring is not None or key32 is not None
        if keyed:
            ctrs = self._ctr_dev(ctrs)
            if ctrs.numel() != B:
                raise ValueError("one expected counter per record is required with a key")
        kd = self._key_dev(ring, key_idx, B) if ring is not None else None
        payload = torch.empty((B, 55), dtype=torch.uint8, device=self.device)
        ok = torch.empty(B, dtype=torch.int8, device=self.device)
        which = torch.empty(B, dtype=torch.int32, device=self.device)
        lists = (B, L, scl.hard_info, scl.hard_ok, scl.cand_info, scl.cand_metric, scl.cand_ok, scl.ncand, payload, ok, which)
        if ring is not None:
            self._call("es_select_keyed_batch", ring.ring, ring.n, kd, ctrs, *lists)
        else:
            self._call("es_select_batch", bytes(key32) if keyed else None, ctrs if keyed else None, *lists)
        return payload, ok, which

    # ------------------------------------------------------------------ metric unit
    def decode_batch(self, frames: torch.Tensor, band: torch.Tensor, pn_rows: torch.Tensor, *,
                     start: torch.Tensor | str | None = None, list_size: int = 8, keep_corr: bool = False):
        """sync + LLR(variant 0 at `start`, default 0; "peak" = each record's first detected peak) + SCL-L for every record.

        After the band-pass the chain forks: correlation + peak picking and the demodulator (frame
        start known) both only need `y`, so the LLR kernel runs on a side HIP stream beside them;
        the branches are joined before the list decoder starts.  With start="peak" the demodulator
        needs the peaks: it runs after sync, on the caller's stream, reading them in place."""
        main = torch.cuda.current_stream(self.device)
        peak = isinstance(start, str)
        if peak:
            _peak_start(start)
        elif getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(self.device)
        if (not keep_corr) and frames.shape[1] - 62 <= self.FAST_MAX_LAGS:
            corr = None      # float32 correlation screen + exact float64 fix-ups (identical thr / peaks)
            y, thr, peaks, npeaks, _flags, llr = self.front_steps(frames, band, pn_rows, start=start, side=None if peak else self._side)
        else:
            y = self.bpf(frames, band)
            if not peak:
                self._side.wait_stream(main)
                with torch.cuda.stream(self._side):      # the demodulator only needs y: it runs beside sync
                    llr = self.llr(y, band, pn_rows, start=start, variant=0)
            corr = self.xcorr(y, band)
            thr, peaks, npeaks = self.pick(corr)
            if peak:
                llr = self.llr(y, band, pn_rows, start="peak", peaks=peaks, variant=0)
            else:
                main.wait_stream(self._side)             # join before SCL, which wants the chip to itself
        if not peak:
            llr.record_stream(main)                          # (allocated on the side stream, read on the caller's from here on)
        scl = self.scl(llr, list_size=list_size, skip_if_hard_ok=True)
        return SyncResult(y, corr if keep_corr else None, thr, peaks, npeaks), llr, scl


def select_payload(scl: SclResult, row: int = 0, validator=None):
    """Host-side tail of PolarCode.decode (rtwm/fastpolar.py:268-276, 332-359) for one record:
    apply CRC / validator rules to the hard candidate and the metric-ordered list."""
    hard = bytes(scl.hard_info[row].cpu().numpy().tobytes())
    hard_ok = bool(scl.hard_ok[row].item())

    def _valid(payload: bytes) -> bool:
        try:
            return bool(validator(payload))
        except Exception:
            return False

    if hard_ok and (validator is None or _valid(hard)):
        return hard, True
    n = int(scl.ncand[row].item())
    if n < 0:
        raise nat.NativeError("es_scl_batch: this record was not decoded (no free scratch-slab slot)")
    if n == 0:      # list loop skipped although the shortcut did not return: only when validator is set
        raise RuntimeError("list decode was skipped; call scl(..., skip_if_hard_ok=False) when using a validator")
    infos = scl.cand_info[row].cpu().numpy()
    oks = scl.cand_ok[row].cpu().numpy()
    metrics = scl.cand_metric[row].cpu().numpy()
    best_crc = None
    best_any = (np.inf, hard)
    for r in range(n):
        payload = infos[r].tobytes()
        if oks[r]:
            if validator is None or _valid(payload):
                return payload, True
            if best_crc is None or metrics[r] < best_crc[0]:
                best_crc = (metrics[r], payload)
        elif metrics[r] < best_any[0]:
            best_any = (metrics[r], payload)
    if best_crc is not None:
        return best_crc[1], False
    return best_any[1], False


def __getattr__(name: str):      # the pipeline's public names stay importable from here (on first use: pipeline.py imports this module, so not at import)
    if name in ("DecodePipeline", "GroupTicket", "hw_queue_budget", "pipeline_streams"):
        from . import pipeline
        return getattr(pipeline, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
