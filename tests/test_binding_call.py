"""CPU: the one place host Python calls the C ABI (RxEngine._call), the header rule it rests on, and monitor.pack_chunks.

`_call(name, *args)` looks `name` up on `_lib` at every call, passes the context first, a tensor as its data_ptr() and everything else as
it is, the current stream last exactly when the name ends in `_batch`, and raises what `nat.check` raises.  Here it runs without a GPU or
a library: on an RxEngine that was never initialised, over a fake `_lib` that records what it is given and returns a chosen code."""
import glob
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import echoseal_amd._native as nat
from echoseal_amd.engine import RxEngine
from echoseal_amd.monitor import pack_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTEXT_FUNCTIONS = {"es_create", "es_destroy", "es_last_error", "es_info_bytes", "es_abi_version"}      # called directly, in __init__ / close / load


class _FakeLib:
    """Every es_* attribute is a function that records its arguments and returns `rc`; es_last_error answers `msg`."""

    def __init__(self, rc: int = 0, msg: bytes | None = b"made up"):
        self.rc, self.msg, self.calls = rc, msg, []

    def __getattr__(self, name):
        if not name.startswith("es_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name,) + args)
            return self.msg if name == "es_last_error" else self.rc
        return fn


def _engine(monkeypatch, **kw):
    lib = _FakeLib(**kw)
    eng = RxEngine.__new__(RxEngine)
    eng._lib, eng._ctx = lib, 1234
    eng._stream = lambda: 77
    monkeypatch.setattr(nat, "_lib", lib)               # nat.check asks load().es_last_error(ctx): the fake answers, never the real library
    return eng, lib


def test_arguments_context_and_stream(monkeypatch):
    eng, lib = _engine(monkeypatch)
    t = torch.arange(6, dtype=torch.float32)
    size, addr, gain, key = 5, t.data_ptr() + 8, 0.25, b"\x01" * 32
    assert eng._call("es_mix_batch", t, None, size, addr, gain, key) is None
    assert eng._call("es_set_option", b"scl_multi", 1) is None
    batch, option = lib.calls
    assert batch == ("es_mix_batch", 1234, t.data_ptr(), None, 5, t.data_ptr() + 8, 0.25, key, 77)
    assert batch[3] is None and batch[4] is size and batch[5] is addr and batch[6] is gain and batch[7] is key      # handed through, not converted
    assert option == ("es_set_option", 1234, b"scl_multi", 1)                                                       # no stream: the name does not end in _batch
    assert eng._call("es_reserve", 8, 1215) is None and lib.calls[-1] == ("es_reserve", 1234, 8, 1215)


def test_the_function_is_looked_up_at_every_call(monkeypatch):
    """tests/test_gpu_pipeline_order.py replaces `_lib` on a live engine: nothing may be cached."""
    eng, lib = _engine(monkeypatch)
    eng._call("es_bpf_batch", 1)
    other = _FakeLib()
    eng._lib, eng._ctx = other, 99
    eng._call("es_bpf_batch", 2)
    assert lib.calls == [("es_bpf_batch", 1234, 1, 77)] and other.calls == [("es_bpf_batch", 99, 2, 77)]


@pytest.mark.parametrize("msg, said", [(b"made up", "made up"), (None, "?")])
def test_a_return_code_raises_what_check_raises(monkeypatch, msg, said):
    eng, lib = _engine(monkeypatch, rc=22, msg=msg)
    with pytest.raises(nat.NativeError) as want:
        nat.check(1234, 22, "es_plan_at_batch")
    with pytest.raises(nat.NativeError) as got:
        eng._call("es_plan_at_batch", None)
    assert str(got.value) == str(want.value) == f"es_plan_at_batch failed (code 22): {said}"
    assert lib.calls[-2:] == [("es_plan_at_batch", 1234, None, 77), ("es_last_error", 1234)]


def test_success_does_not_ask_for_an_error(monkeypatch):
    eng, lib = _engine(monkeypatch, rc=0)
    eng._call("es_pick_batch", 3)
    assert [c[0] for c in lib.calls] == ["es_pick_batch"]


def test_header_stream_last_exactly_for_batch_names():
    """The rule _call rests on: a declaration ends in `void* stream` if and only if its name ends in `_batch`; SIGNATURES agrees."""
    decl = nat.DECLARATIONS
    assert set(decl) == set(nat.SIGNATURES) and len(decl) == 56, set(decl) ^ set(nat.SIGNATURES)
    for name, params in decl.items():
        takes = bool(params) and params[-1] == ("void*", "stream")
        assert takes == name.endswith("_batch"), (name, params[-1:])
        assert not any(p == "stream" for _, p in params[:-1]), name
        argtypes = nat.SIGNATURES[name][1]
        assert len(argtypes) == len(params), name
        if takes:
            assert argtypes[-1] is nat.c_void_p and argtypes[0] is nat.c_void_p, name


def test_no_call_site_is_written_out_by_hand():
    """In the package only the five context functions are called on `_lib` directly, and the `_ptr` wrapper is gone."""
    files = sorted(glob.glob(os.path.join(ROOT, "echoseal_amd", "*.py")))
    assert len(files) > 10
    for path in files:
        src = open(path).read()
        direct = set(re.findall(r"_lib\.(es_[a-z0-9_]+)", src))
        assert direct <= CONTEXT_FUNCTIONS, (path, direct - CONTEXT_FUNCTIONS)
        assert not re.search(r"\b_ptr\b", src), path
        if os.path.basename(path) != "_native.py":
            assert "nat.check(" not in src or os.path.basename(path) == "engine.py", path
    assert open(os.path.join(ROOT, "echoseal_amd", "engine.py")).read().count("nat.check(") == 1


# ---------------------------------------------------------------------- pack_chunks against the two loops it replaces
def _chunks(kinds: str, lengths) -> list:
    """One chunk per letter, 'f' float32 or 'h' int16, of the given lengths, no value zero."""
    rng = np.random.default_rng(len(kinds) * 31 + sum(lengths))
    return [(rng.integers(1, 30000, n).astype(np.int16) if k == "h" else (1.0 + rng.random(n)).astype(np.float32)) for k, n in zip(kinds, lengths)]


def _resample_step_rows(arrs):
    """RxEngine.resample_step's staging buffer as it was written out there -> (buf, stride, k32, order)."""
    R = len(arrs)
    lengths = np.array([a.size for a in arrs], np.int64)
    order = np.argsort([a.dtype == np.int16 for a in arrs], kind="stable")
    k32 = int(sum(a.dtype != np.int16 for a in arrs))
    stride = max(4, (int(lengths.max()) + 3) // 4 * 4)
    buf = np.zeros(k32 * stride * 4 + (R - k32) * stride * 2, np.uint8)
    x32 = buf[:k32 * stride * 4].view(np.float32).reshape(k32, stride)
    x16 = buf[k32 * stride * 4:].view(np.int16).reshape(R - k32, stride)
    for k, i in enumerate(order):
        (x32 if k < k32 else x16)[k if k < k32 else k - k32, :arrs[i].size] = arrs[i]
    return buf, stride, k32, order


def _monitor_step_rows(arrs, other):
    """RxEngine.monitor_step's staging buffer as it was written out there -> (buf, stride, k32, order)."""
    R = len(arrs)
    raw = np.array([a.size for a in arrs], np.int64)
    i16 = np.array([a.dtype == np.int16 for a in arrs], bool)
    order = np.argsort(2 * other + i16, kind="stable")
    nA, nB, nC = (int(np.count_nonzero(m)) for m in (~other & ~i16, ~other & i16, other & ~i16))
    k32 = nA + nC
    stride = max(4, (int(raw.max()) + 3) // 4 * 4)
    buf = np.zeros(k32 * stride * 4 + (R - k32) * stride * 2, np.uint8)
    x32 = buf[:k32 * stride * 4].view(np.float32).reshape(k32, stride)
    x16 = buf[k32 * stride * 4:].view(np.int16).reshape(R - k32, stride)
    rows32 = np.concatenate((order[:nA], order[nA + nB: nA + nB + nC]))
    rows16 = np.concatenate((order[nA: nA + nB], order[nA + nB + nC:]))
    for k, i in enumerate(rows32):
        x32[k, :arrs[i].size] = arrs[i]
    for k, i in enumerate(rows16):
        x16[k, :arrs[i].size] = arrs[i]
    return buf, stride, k32, order


CASES = [("f", (0,)), ("h", (0,)), ("f", (1,)), ("h", (9,)), ("f", (4,)), ("h", (5,)),                  # a single chunk
         ("ffffff", (0, 1, 3, 4, 5, 9)), ("hhhhhh", (9, 5, 4, 3, 1, 0)),                                # all of one sample type
         ("fhfhfh", (0, 1, 3, 4, 5, 9)), ("hfhfhf", (9, 5, 4, 3, 1, 0)), ("hhffhf", (3, 0, 4, 4, 1, 5)), ("fh", (3, 4)), ("hf", (5, 0))]


def _check(got, want):
    buf, stride, k32 = got
    assert buf.dtype == np.uint8 and buf.ndim == 1 and isinstance(stride, int) and isinstance(k32, int)
    assert (stride, k32) == (want[1], want[2]) and buf.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("kinds, lengths", CASES)
def test_pack_chunks_is_resample_steps_buffer(kinds, lengths):
    arrs = _chunks(kinds, lengths)
    want = _resample_step_rows(arrs)
    _check(pack_chunks(arrs, want[3]), want)
    _check(pack_chunks(arrs, np.arange(len(arrs))), want)                   # the identity: the same stable partition


@pytest.mark.parametrize("kinds, lengths", CASES)
@pytest.mark.parametrize("pattern", [0b000000, 0b111111, 0b010101, 0b100110])
def test_pack_chunks_is_monitor_steps_buffer(kinds, lengths, pattern):
    arrs = _chunks(kinds, lengths)
    other = np.array([bool(pattern >> i & 1) for i in range(len(arrs))], bool)      # which chunks arrive at another rate
    want = _monitor_step_rows(arrs, other)
    _check(pack_chunks(arrs, want[3]), want)
    if not other.any():
        _check(pack_chunks(arrs, want[3]), _resample_step_rows(arrs))       # no other rate: both callers' sort keys give one order


def test_pack_chunks_rows_are_zero_filled_and_float32_first():
    arrs = _chunks("hfh", (5, 3, 1))
    buf, stride, k32 = pack_chunks(arrs, [2, 1, 0])
    assert (stride, k32, buf.size) == (8, 1, 1 * 8 * 4 + 2 * 8 * 2)
    x32, x16 = buf[:32].view(np.float32), buf[32:].view(np.int16).reshape(2, 8)
    assert np.array_equal(x32[:3], arrs[1]) and not x32[3:].any()
    assert np.array_equal(x16[0, :1], arrs[2]) and not x16[0, 1:].any() and np.array_equal(x16[1, :5], arrs[0]) and not x16[1, 5:].any()


def test_pack_chunks_of_no_chunks_is_empty():
    """Both callers return before they upload when nothing was pushed; the packer itself then gives an empty buffer and the least stride."""
    buf, stride, k32 = pack_chunks([], np.arange(0))
    assert buf.size == 0 and buf.dtype == np.uint8 and (stride, k32) == (4, 0)
