"""DecodePipeline: the streaming form of `RxEngine.decode_batch`, several batches in flight on several HIP streams.  Batches are
independent; per batch the kernels' inputs and results are those of decode_batch in each of the three arrangements, which differ in
the stream and context every call goes to.  The receive sequence itself is `RxEngine.front_steps`, shared with decode_batch."""
from __future__ import annotations

import os
import warnings

import torch

from .engine import RxEngine, SclResult, SyncResult

# The streaming pipelines run on up to eight HIP streams.  The HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues
# (default 4) and streams that share a queue serialise, silently.  The variable belongs to the process's environment: this module reads
# it and never sets it; DecodePipeline warns when more streams are alive than the budget it names.
_HWQ_ENV_AT_IMPORT = os.environ.get("GPU_MAX_HW_QUEUES")      # None: the runtime's default
_LIVE_STREAMS = [0]                                            # streams made through pipeline_streams and not yet given back (a plain count:
                                                               # weak references to torch.cuda.Stream objects crash the interpreter's final GC)


def hw_queue_budget() -> int:
    """Hardware queues the process's HIP streams are spread over, as far as this module can tell: GPU_MAX_HW_QUEUES as it stood
    when the module was imported, else the runtime's default of 4."""
    try:
        return max(1, int(_HWQ_ENV_AT_IMPORT)) if _HWQ_ENV_AT_IMPORT is not None else 4
    except ValueError:
        return 4


def pipeline_streams(device, n: int, priority: int = 0) -> list:
    """n new HIP streams, counted against the hardware-queue budget (DecodePipeline makes its own through this; a process that builds
    several pipelines makes the streams once and hands them to each: DecodePipeline(streams=...))."""
    out = [torch.cuda.Stream(device, priority=priority) for _ in range(n)]
    _LIVE_STREAMS[0] += n
    if _LIVE_STREAMS[0] > hw_queue_budget():
        import gc
        gc.collect()                                # (pipelines that are garbage but not yet collected still count their streams)
    if _LIVE_STREAMS[0] > hw_queue_budget():
        warnings.warn(f"DecodePipeline: {_LIVE_STREAMS[0]} pipeline streams are alive but the HIP runtime has {hw_queue_budget()} hardware queues "
                      f"(GPU_MAX_HW_QUEUES{'=' + _HWQ_ENV_AT_IMPORT if _HWQ_ENV_AT_IMPORT else ' not set'}): streams that share a "
                      "queue serialise.  Hand existing streams to further pipelines (streams=...).", RuntimeWarning, stacklevel=3)
    return out


def DecodePipeline(eng: RxEngine, *, list_size: int = 8, scl_streams: int = 2, depth: int | None = None, lanes: int = 0,
                   side_stream: bool = True, group: int = 0, streams=None):
    """The pipeline these keywords ask for: group=G > 0 a GroupedPipeline (the throughput arrangement, bench.py's headline), else
    lanes=K > 0 a LanePipeline, else a StagedPipeline.  Results are complete after `wait(result)` / `synchronize()`.  More live
    pipeline streams than hardware queues raises a RuntimeWarning (hw_queue_budget): they share queues and serialise.  `streams=`
    (lanes: a list; grouped: (front-end streams, list-decoder streams)) builds a further pipeline on existing streams instead."""
    if int(group) > 0:
        return GroupedPipeline(eng, list_size, group, lanes, scl_streams, streams)
    if int(lanes) > 0:
        return LanePipeline(eng, list_size, lanes, streams)
    return StagedPipeline(eng, list_size, scl_streams, depth, side_stream)


class _Pipeline:
    """What the arrangements share.  Each has submit(frames, band, pn_rows, *, start, xcorr_events, select, inputs_ready) ->
    (SyncResult, llr, scl, done), which enqueues one batch.  start: frame starts [B] (None = 0; "peak" = the first detected peak of
    each record, read in place by the demodulator).  xcorr_events: two timing events, recorded around the sync.  select: also run
    the candidate selection (es_select_batch, validator None) behind the list decoder and attach it to the SclResult as `.selected =
    (payload, ok, which)`: lanes and grouped; the staged arrangement accepts and ignores it.  inputs_ready: grouped only."""

    def __init__(self, eng: RxEngine, list_size: int):
        self.eng = eng
        self.list_size = int(list_size)
        self._own_streams = 0                     # streams this pipeline made itself (given back to the budget when it is collected)

    def _mk(self, n: int, priority: int = 0) -> list:
        self._own_streams += n
        return pipeline_streams(self.eng.device, n, priority)

    def __del__(self):  # pragma: no cover
        try:
            _LIVE_STREAMS[0] -= self._own_streams
        except Exception:
            pass

    def _check(self, frames: torch.Tensor) -> None:
        if frames.shape[1] - 62 > self.eng.FAST_MAX_LAGS:
            raise ValueError("DecodePipeline serves frame-sized records (use RxEngine.decode_batch for long captures)")

    @staticmethod
    def wait(result) -> None:
        result[3].synchronize()


class StagedPipeline(_Pipeline):
    """The front end on one stream (the demodulator on a side stream unless side_stream=False), the list decoder on one of
    `scl_streams` further streams, at most `depth` batches in flight."""

    def __init__(self, eng, list_size, scl_streams, depth, side_stream):
        super().__init__(eng, list_size)
        self.front = self._mk(1, priority=-1)[0]                                 # the short front-end kernels get dispatch priority over the long-running list decoders
        self.side = self._mk(1, priority=-1)[0] if side_stream else self.front   # one hardware queue less without it
        self.backs = self._mk(max(1, int(scl_streams)))
        self.scl_engs = [eng] + [RxEngine(eng.device, list_size_max=max(8, self.list_size)) for _ in self.backs[1:]]
        # Batches in flight = list-decoder streams: the front end of batch k waits for batch k-2 to leave, so it runs while only ONE list
        # decoder is resident (two of them fill every SIMD's register file and would starve the short front-end kernels of wave
        # slots), and its own list decoder then starts beside the one still running.
        self.depth = len(self.backs) if depth is None else max(1, int(depth))
        self._inflight: list = []            # `done` events of the most recent batches
        self._k = 0

    def submit(self, frames, band, pn_rows, *, start=None, xcorr_events=None, select=False, inputs_ready=False):
        self._check(frames)
        self.front.wait_stream(torch.cuda.current_stream(self.eng.device))   # inputs were produced on the caller's stream
        if len(self._inflight) >= self.depth:                                # at most `depth` batches in flight
            self.front.wait_event(self._inflight.pop(0))
        with torch.cuda.stream(self.front):
            y, thr, peaks, npeaks, flags, llr = self.eng.front_steps(frames, band, pn_rows, start=start, events=xcorr_events, side=self.side)
            ready = self.front.record_event()
        j = self._k % len(self.backs)
        self._k += 1
        back = self.backs[j]
        back.wait_event(ready)
        llr.record_stream(back)
        with torch.cuda.stream(back):
            scl = self.scl_engs[j].scl(llr, list_size=self.list_size, skip_if_hard_ok=True)
            done = back.record_event()
        self._inflight.append(done)
        return SyncResult(y, None, thr, peaks, npeaks, flags=flags), llr, scl, done

    def synchronize(self) -> None:
        for st in (self.front, self.side, *self.backs):
            st.synchronize()


class LanePipeline(_Pipeline):
    """K independent lanes, each one HIP stream (= one hardware queue) with its own context that runs the WHOLE chain, band-pass ..
    list decoder, of its batches (k, k+K, ...) in order: no cross-stream events at all, rows of a batch within a few milliseconds."""

    def __init__(self, eng, list_size, lanes, streams):
        super().__init__(eng, list_size)
        self.lanes = int(lanes)
        # (lane 0 on the caller's own stream was measured slower: 1.29 M against 1.43 M frames/s at 7 lanes)
        self.lane_streams = list(streams)[:self.lanes] if streams is not None else self._mk(self.lanes)
        if len(self.lane_streams) != self.lanes:
            raise ValueError("streams: one per lane")
        self.lane_engs = [eng] + [RxEngine(eng.device, list_size_max=max(8, self.list_size)) for _ in range(self.lanes - 1)]
        self.scl_engs, self.backs = self.lane_engs, self.lane_streams       # a lane decodes too: callers set list-decoder options through these
        self._k = 0

    def submit(self, frames, band, pn_rows, *, start=None, xcorr_events=None, select=False, inputs_ready=False):
        self._check(frames)
        j = self._k % self.lanes
        self._k += 1
        st, e = self.lane_streams[j], self.lane_engs[j]
        st.wait_stream(torch.cuda.current_stream(self.eng.device))
        with torch.cuda.stream(st):
            y, thr, peaks, npeaks, flags, llr = e.front_steps(frames, band, pn_rows, start=start, events=xcorr_events)
            scl = e.scl(llr, list_size=self.list_size, skip_if_hard_ok=True)
            if select:
                scl.selected = e.select(scl)
            done = st.record_event()
        for t in (frames, band, pn_rows):
            t.record_stream(st)
        return SyncResult(y, None, thr, peaks, npeaks, flags=flags), llr, scl, done

    def synchronize(self) -> None:
        for st in self.lane_streams:
            st.synchronize()


class GroupedPipeline(_Pipeline):
    """The front ends (band-pass .. demodulator) of `group` consecutive batches run on `lanes` high-priority streams and write
    their LLR rows into ONE buffer, and ONE list-decoder launch (on one of `scl_streams` streams, own context, one lane per path:
    es_set_option "scl_lanes" = 1, the mapping with the fewest instructions per frame) decodes the whole group: that mapping
    needs tens of thousands of frames per launch to fill the chip, which a 1 024-frame batch cannot give it.  A batch's rows are a
    slice of its group's result (`GroupTicket.result()`), complete when the group's launch is; `synchronize()` / `wait` decode an incomplete group."""

    def __init__(self, eng, list_size, group, lanes, scl_streams, streams):
        super().__init__(eng, list_size)
        self.group = int(group)
        self.lanes = max(1, int(lanes) or 4)
        nb = max(1, int(scl_streams))
        # (priority: the short front-end kernels must slip in whenever list-decoder waves leave)
        self.lane_streams = list(streams[0])[:self.lanes] if streams is not None else self._mk(self.lanes, priority=-1)
        if len(self.lane_streams) != self.lanes:
            raise ValueError("streams: one front-end stream per lane")
        self.lane_engs = [eng] + [RxEngine(eng.device, list_size_max=0) for _ in range(self.lanes - 1)]     # front-end contexts: no list-decoder scratch
        self.backs = list(streams[1])[:nb] if streams is not None else self._mk(nb)
        if len(self.backs) != nb:
            raise ValueError("streams: one list-decoder stream per scl_streams")
        self.scl_engs = [RxEngine(eng.device, list_size_max=max(8, self.list_size)) for _ in range(nb)]
        for e in self.scl_engs:                   # kernel by launch size: a full group runs one lane per path, a lone batch one frame per wave
            e.set_option("scl_multi", -1); e.set_option("scl_lanes", 0); e.set_option("scl_lane_slab", 1)
        self._ring: list = [None] * (nb + 1)      # the most recent groups: a new group's front ends wait for the decoder of the group nb + 1 before it
        self._open = None
        self._k = self._g = 0
        self._flush_lanes = 0                     # (tests: 1 = one lane per path whatever the group's size)

    def submit(self, frames, band, pn_rows, *, start=None, xcorr_events=None, select=False, inputs_ready=False):
        self._check(frames)
        B = frames.shape[0]
        g = self._open
        if g is not None and (g.B != B or g.select != bool(select)):
            self._flush(g); g = None
        if g is None:
            r = self._g % len(self._ring)
            g = _Group(self, B, bool(select), self._ring[r])
            self._ring[r] = g                         # (only its `done` event is looked at again: the throttle of the group opened R groups later)
            self._open = g
            self._g += 1
        j = self._k % self.lanes
        self._k += 1
        st, e = self.lane_streams[j], self.lane_engs[j]
        if not inputs_ready:      # (inputs_ready: the caller vouches that frames / band / pn_rows are complete on the device: 10 us of host time per batch)
            st.wait_stream(torch.cuda.current_stream(self.eng.device))
        if g.throttle is not None:
            st.wait_event(g.throttle)                                         # at most len(ring) groups in flight on the GPU
        if g.llr is None:                                                     # on THIS lane's stream: the block's earlier life is ordered before its writes
            with torch.cuda.stream(st):
                g.llr = torch.empty((self.group * B, 1024), dtype=torch.float32, device=self.eng.device)
            g.alloc_ev = st.record_event()
            g.lanes_used.add(j)
        elif j not in g.lanes_used:
            g.lanes_used.add(j)
            st.wait_event(g.alloc_ev)                                         # (a recycled block may still be in use by work queued on the allocating stream)
            g.llr.record_stream(st)
        slot = g.count
        rows = g.llr[slot * B:(slot + 1) * B]
        with torch.cuda.stream(st):
            if xcorr_events is None:              # the three launches through one library call (es_front_batch / es_front_peak_batch)
                y, thr, peaks, npeaks, flags, _ = e.front(frames, band, pn_rows, start=start, out=rows)
            else:
                y, thr, peaks, npeaks, flags, _ = e.front_steps(frames, band, pn_rows, start=start, out=rows, events=xcorr_events)
            ready = st.record_event()
        for t in (frames, band, pn_rows):
            t.record_stream(st)
        g.ready.append(ready)
        g.count += 1
        ticket = GroupTicket(g, slot)
        if g.count == self.group:
            self._flush(g)
        return SyncResult(y, None, thr, peaks, npeaks, flags=flags), rows, ticket, ticket

    def _flush(self, g) -> None:
        if g.done is not None:
            return
        j = g.index % len(self.backs)
        back, e = self.backs[j], self.scl_engs[j]
        for ev in g.ready:
            back.wait_event(ev)
        lp = 1 << max(0, self.list_size - 1).bit_length()
        # one lane per path once the group gives every SIMD a wave (launches of several groups overlap); a lone batch: the library's choice
        e.set_option("scl_lanes", 1 if (g.count * g.B * lp >= 64 * 1024 or self._flush_lanes == 1) else 0)
        g.llr.record_stream(back)
        with torch.cuda.stream(back):
            g.scl = e.scl(g.llr[:g.count * g.B], list_size=self.list_size, skip_if_hard_ok=True)
            if g.select:
                g.selected = e.select(g.scl)
            g.done = back.record_event()
        if self._open is g:
            self._open = None

    def synchronize(self) -> None:
        if self._open is not None:
            self._flush(self._open)
        for st in (*self.lane_streams, *self.backs):
            st.synchronize()


class _Group:
    """Batches that share one list-decoder launch (GroupedPipeline)."""

    def __init__(self, pipe: GroupedPipeline, B: int, select: bool, prev):
        self.pipe, self.B, self.select = pipe, B, select
        self.index = pipe._g
        # a buffer of its own (the rows handed out to the caller stay valid as long as the caller keeps them), allocated by the first
        # submit on that batch's lane stream; the caching allocator is told about every other stream that touches it
        self.llr = self.alloc_ev = None
        self.throttle = prev.done if prev is not None else None
        self.lanes_used, self.ready, self.count = set(), [], 0      # lanes that know the buffer, their batches' `ready` events, batches so far
        self.scl = self.selected = self.done = None
        self.checked = False                      # the group's SclResult.check() has run


class GroupTicket:
    """A batch's place in its group: `result()` -> SclResult rows of this batch (flushes / waits as needed)."""

    def __init__(self, g: _Group, slot: int):
        self.g, self.slot = g, slot

    def synchronize(self) -> None:
        self.g.pipe._flush(self.g)
        self.g.done.synchronize()

    def result(self) -> SclResult:
        self.synchronize()
        lo, hi = self.slot * self.g.B, (self.slot + 1) * self.g.B
        s = self.g.scl
        if not self.g.checked:
            s.check(); self.g.checked = True                  # (the launch is complete: one small reduction per group)
        res = SclResult(s.hard_info[lo:hi], s.hard_ok[lo:hi], s.cand_info[lo:hi], s.cand_metric[lo:hi], s.cand_ok[lo:hi], s.ncand[lo:hi])
        if self.g.selected is not None:
            res.selected = tuple(t[lo:hi] for t in self.g.selected)
        return res
