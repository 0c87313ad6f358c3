"""Which library call goes to which HIP stream, in which order, behind which waits: DecodePipeline's three arrangements and
RxEngine.decode_batch, pinned call by call.

The other pipeline tests compare rows, which are values; a pipeline that dropped the side-stream fork or a throttle would still
return the right rows.  Here one ordered log is recorded per case and compared with the log written out below:

    es_xxx_batch @role              a library call that takes a stream (its last argument), recorded at the binding: a pass-through
                                    proxy around the `_lib` of every engine the pipeline uses
    es_set_option name=value
    a.wait_stream(b)                torch.cuda.Stream.wait_stream
    a.wait_event(evN)               torch.cuda.Stream.wait_event
    evN.record(a)                   torch.cuda.Event.record, with the stream that was current
    record_stream(a)                torch.Tensor.record_stream

Roles: caller (the stream that was current), front / side, lane[j], back[j] (a stream that is both a lane and a list-decoder
stream is lane[j]).  Events are numbered by first appearance.  Every batch is 8 one-frame records, the list size is 2."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.embedder import WatermarkEmbedder

KEY = b"\xAA" * 32
B = 8


class _Lib:
    """Pass-through proxy of the ctypes library: logs the entry points that take a stream, and es_set_option."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "es_set_option":
            def call(ctx, opt, value):
                self._log.append(("option", opt.decode(), int(value)))
                return fn(ctx, opt, value)
        elif name.endswith("_batch"):
            def call(*args):
                self._log.append(("call", name, int(args[-1] or 0)))
                return fn(*args)
        else:
            return fn
        return call


class _Recorder:
    def __init__(self, monkeypatch, device):
        self.raw: list = []
        self.device = device
        self._depth = 0                      # (Stream.wait_stream is itself an event record and a wait: only the outermost operation is logged)
        self._keep: list = []                # events seen, kept alive so that no two share an id
        for cls, name, entry in ((torch.cuda.Stream, "wait_stream", lambda s, other: ("wait_stream", s.cuda_stream, other.cuda_stream)),
                                 (torch.cuda.Stream, "wait_event", lambda s, ev: ("wait_event", s.cuda_stream, self._event(ev))),
                                 (torch.cuda.Event, "record", lambda ev, stream=None: ("record", self._event(ev), (
                                     stream if stream is not None else torch.cuda.current_stream(device)).cuda_stream)),
                                 (torch.Tensor, "record_stream", lambda t, s: ("record_stream", s.cuda_stream))):
            monkeypatch.setattr(cls, name, self._logged(getattr(cls, name), entry))

    def _logged(self, orig, entry):
        def op(*args, **kw):
            if self._depth == 0:
                self.raw.append(entry(*args, **kw))
            self._depth += 1
            try:
                return orig(*args, **kw)
            finally:
                self._depth -= 1
        return op

    def _event(self, ev) -> int:
        if not any(ev is e for e in self._keep):
            self._keep.append(ev)
        return id(ev)

    def watch(self, monkeypatch, engines) -> None:
        seen = []
        for e in engines:
            if not any(e is s for s in seen):
                seen.append(e)
                monkeypatch.setattr(e, "_lib", _Lib(e._lib, self.raw))

    def log(self, roles) -> list:
        """The log with stream handles as roles (`roles`: (name, stream) pairs, the first that matches names a handle)."""
        names: dict = {}
        for name, st in roles:
            names.setdefault(st.cuda_stream, name)
        events: dict = {}
        s = lambda h: names.get(h, f"unknown stream {h:#x}")
        ev = lambda i: events.setdefault(i, f"ev{len(events) + 1}")
        out = []
        for r in self.raw:
            if r[0] == "call":
                out.append(f"{r[1]} @{s(r[2])}")
            elif r[0] == "option":
                out.append(f"es_set_option {r[1]}={r[2]}")
            elif r[0] == "wait_stream":
                out.append(f"{s(r[1])}.wait_stream({s(r[2])})")
            elif r[0] == "wait_event":
                out.append(f"{s(r[1])}.wait_event({ev(r[2])})")
            elif r[0] == "record":
                out.append(f"{ev(r[1])}.record({s(r[2])})")
            else:
                out.append(f"record_stream({s(r[1])})")
        return out


@pytest.fixture(scope="module")
def batch(engine):
    """8 one-frame records of 1 215 samples with their schedule, on the device: every case submits this one batch, unchanged."""
    frames, _ = engine.synthetic_frames(KEY, 0, B)
    sec = WatermarkEmbedder(KEY).sec
    pn, band = engine.schedule(sec._prng.sub_key, KEY, ctr0=0, n=B)
    torch.cuda.synchronize()
    assert frames.shape == (B, 1215)
    return frames, band, pn


def _pipeline_log(engine, batch, monkeypatch, kwargs, submits, **submit_kw):
    """Build DecodePipeline(engine, list_size=2, **kwargs), then log `submits` submits of the batch and synchronize()."""
    from echoseal_amd.engine import DecodePipeline
    pipe = DecodePipeline(engine, list_size=2, **kwargs)
    caller = torch.cuda.current_stream(engine.device)
    torch.cuda.synchronize()
    if submit_kw.pop("events", False):
        submit_kw["xcorr_events"] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    rec = _Recorder(monkeypatch, engine.device)
    rec.watch(monkeypatch, [pipe.eng] + list(getattr(pipe, "lane_engs", [])) + list(pipe.scl_engs))
    out = [pipe.submit(*batch, **submit_kw) for _ in range(submits)]
    pipe.synchronize()
    torch.cuda.synchronize()
    roles = [("caller", caller)]
    if getattr(pipe, "front", None) is not None:
        roles += [("front", pipe.front), ("side", pipe.side)]
    roles += [(f"lane[{j}]", st) for j, st in enumerate(getattr(pipe, "lane_streams", []))]
    roles += [(f"back[{j}]", st) for j, st in enumerate(pipe.backs)]
    return rec.log(roles), pipe, out


def _lines(text: str) -> list:
    return [ln.strip() for ln in text.strip().splitlines() if ln.strip()]


STAGED = """
    front.wait_stream(caller)
    es_bpf2_batch @front
    side.wait_stream(front)
    es_llr_batch @side
    es_sync_fused_batch @front
    front.wait_stream(side)
    ev1.record(front)
    back[0].wait_event(ev1)
    record_stream(back[0])
    es_scl_batch @back[0]
    ev2.record(back[0])

    front.wait_stream(caller)
    es_bpf2_batch @front
    side.wait_stream(front)
    es_llr_batch @side
    es_sync_fused_batch @front
    front.wait_stream(side)
    ev3.record(front)
    back[1].wait_event(ev3)
    record_stream(back[1])
    es_scl_batch @back[1]
    ev4.record(back[1])

    front.wait_stream(caller)
    front.wait_event(ev2)
    es_bpf2_batch @front
    side.wait_stream(front)
    es_llr_batch @side
    es_sync_fused_batch @front
    front.wait_stream(side)
    ev5.record(front)
    back[0].wait_event(ev5)
    record_stream(back[0])
    es_scl_batch @back[0]
    ev6.record(back[0])
"""

STAGED_PEAK = """
    front.wait_stream(caller)
    es_bpf2_batch @front
    ev1.record(front)
    es_sync_fused_batch @front
    ev2.record(front)
    es_llr_at_batch @front
    ev3.record(front)
    back[0].wait_event(ev3)
    record_stream(back[0])
    es_scl_batch @back[0]
    ev4.record(back[0])

    front.wait_stream(caller)
    es_bpf2_batch @front
    ev1.record(front)
    es_sync_fused_batch @front
    ev2.record(front)
    es_llr_at_batch @front
    ev5.record(front)
    back[1].wait_event(ev5)
    record_stream(back[1])
    es_scl_batch @back[1]
    ev6.record(back[1])
"""

LANES = """
    lane[0].wait_stream(caller)
    es_bpf2_batch @lane[0]
    es_sync_fused_batch @lane[0]
    es_llr_batch @lane[0]
    es_scl_batch @lane[0]
    es_select_batch @lane[0]
    ev1.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    lane[1].wait_stream(caller)
    es_bpf2_batch @lane[1]
    es_sync_fused_batch @lane[1]
    es_llr_batch @lane[1]
    es_scl_batch @lane[1]
    es_select_batch @lane[1]
    ev2.record(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])

    lane[0].wait_stream(caller)
    es_bpf2_batch @lane[0]
    es_sync_fused_batch @lane[0]
    es_llr_batch @lane[0]
    es_scl_batch @lane[0]
    es_select_batch @lane[0]
    ev3.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
"""

LANES_PEAK = """
    lane[0].wait_stream(caller)
    es_bpf2_batch @lane[0]
    ev1.record(lane[0])
    es_sync_fused_batch @lane[0]
    ev2.record(lane[0])
    es_llr_at_batch @lane[0]
    es_scl_batch @lane[0]
    ev3.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    lane[1].wait_stream(caller)
    es_bpf2_batch @lane[1]
    ev1.record(lane[1])
    es_sync_fused_batch @lane[1]
    ev2.record(lane[1])
    es_llr_at_batch @lane[1]
    es_scl_batch @lane[1]
    ev4.record(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
"""

# groups of two batches on two lanes, one list-decoder stream: the ring holds two groups, so the third group is the first that
# waits (for the first group's `done`, ev4); synchronize() decodes it, incomplete
GROUPED = """
    lane[0].wait_stream(caller)
    ev1.record(lane[0])
    es_front_batch @lane[0]
    ev2.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    lane[1].wait_stream(caller)
    lane[1].wait_event(ev1)
    record_stream(lane[1])
    es_front_batch @lane[1]
    ev3.record(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    back[0].wait_event(ev2)
    back[0].wait_event(ev3)
    es_set_option scl_lanes=0
    record_stream(back[0])
    es_scl_batch @back[0]
    es_select_batch @back[0]
    ev4.record(back[0])

    lane[0].wait_stream(caller)
    ev5.record(lane[0])
    es_front_batch @lane[0]
    ev6.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    lane[1].wait_stream(caller)
    lane[1].wait_event(ev5)
    record_stream(lane[1])
    es_front_batch @lane[1]
    ev7.record(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    back[0].wait_event(ev6)
    back[0].wait_event(ev7)
    es_set_option scl_lanes=0
    record_stream(back[0])
    es_scl_batch @back[0]
    es_select_batch @back[0]
    ev8.record(back[0])

    lane[0].wait_stream(caller)
    lane[0].wait_event(ev4)
    ev9.record(lane[0])
    es_front_batch @lane[0]
    ev10.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    back[0].wait_event(ev10)
    es_set_option scl_lanes=0
    record_stream(back[0])
    es_scl_batch @back[0]
    es_select_batch @back[0]
    ev11.record(back[0])
"""

GROUPED_PEAK = """
    ev1.record(lane[0])
    es_bpf2_batch @lane[0]
    ev2.record(lane[0])
    es_sync_fused_batch @lane[0]
    ev3.record(lane[0])
    es_llr_at_batch @lane[0]
    ev4.record(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])
    record_stream(lane[0])

    lane[1].wait_event(ev1)
    record_stream(lane[1])
    es_bpf2_batch @lane[1]
    ev2.record(lane[1])
    es_sync_fused_batch @lane[1]
    ev3.record(lane[1])
    es_llr_at_batch @lane[1]
    ev5.record(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    record_stream(lane[1])
    back[0].wait_event(ev4)
    back[0].wait_event(ev5)
    es_set_option scl_lanes=0
    record_stream(back[0])
    es_scl_batch @back[0]
    ev6.record(back[0])
"""

PIPELINE_CASES = {
    "staged": (dict(), 3, dict(), STAGED),
    "staged, no side stream, at the peaks, events": (dict(side_stream=False), 2, dict(start="peak", events=True), STAGED_PEAK),
    "lanes": (dict(lanes=2), 3, dict(select=True), LANES),
    "lanes, at the peaks, events": (dict(lanes=2), 2, dict(start="peak", events=True), LANES_PEAK),
    "grouped": (dict(lanes=2, scl_streams=1, group=2), 5, dict(select=True), GROUPED),
    "grouped, at the peaks, events, inputs ready": (dict(lanes=2, scl_streams=1, group=2), 2,
                                                    dict(start="peak", events=True, inputs_ready=True), GROUPED_PEAK),
}


@pytest.mark.parametrize("case", list(PIPELINE_CASES))
def test_pipeline_call_order(engine, batch, monkeypatch, case):
    kwargs, submits, submit_kw, expected = PIPELINE_CASES[case]
    log, pipe, out = _pipeline_log(engine, batch, monkeypatch, kwargs, submits, **dict(submit_kw))
    assert log == _lines(expected)
    if kwargs.get("group"):                  # every batch's demodulator wrote its rows of the group's one buffer, in place
        for k, (_sy, rows, ticket, _done) in enumerate(out):
            assert rows.data_ptr() == ticket.g.llr.data_ptr() + (k % 2) * B * 1024 * 4 and rows.shape == (B, 1024)


DECODE_BATCH_CASES = {
    "fork and join": (dict(), """
        es_bpf2_batch @caller
        side.wait_stream(caller)
        es_llr_batch @side
        es_sync_fused_batch @caller
        caller.wait_stream(side)
        record_stream(caller)
        es_scl_batch @caller
    """),
    "at the peaks": (dict(start="peak"), """
        es_bpf2_batch @caller
        es_sync_fused_batch @caller
        es_llr_at_batch @caller
        es_scl_batch @caller
    """),
    "float64 correlation": (dict(keep_corr=True), """
        es_bpf_batch @caller
        side.wait_stream(caller)
        es_llr_batch @side
        es_xcorr_batch @caller
        es_pick_batch @caller
        caller.wait_stream(side)
        record_stream(caller)
        es_scl_batch @caller
    """),
}


@pytest.mark.parametrize("case", list(DECODE_BATCH_CASES))
def test_decode_batch_call_order(engine, batch, monkeypatch, case):
    kwargs, expected = DECODE_BATCH_CASES[case]
    caller = torch.cuda.current_stream(engine.device)
    torch.cuda.synchronize()
    rec = _Recorder(monkeypatch, engine.device)
    rec.watch(monkeypatch, [engine])
    engine.decode_batch(*batch, list_size=2, **kwargs)
    torch.cuda.synchronize()
    roles = [("caller", caller)] + ([("side", engine._side)] if getattr(engine, "_side", None) is not None else [])
    assert rec.log(roles) == _lines(expected)
