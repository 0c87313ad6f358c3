"""GPU: conditioning a queue of mixed-rate clips in one launch (es_resample_ragged_batch, RxEngine.resample_ragged) and the batch calls
that use it.

- the kernel against scipy.signal.resample_poly(x).astype(float32), bit for bit: int16, float32 and float64 samples, every rate pair in
  one launch, lengths around the taps-per-phase and around the tile, rep 1 and 4, a sentinel behind every record, a poisoned pool;
- argument checks of the entry point; graph capture of resample_ragged + sync_ragged;
- verify_batch / identify_batch over a mixed-rate list against a fresh detector on the clip conditioned on the host (utils.resample_to):
  results and traces; an all-48 kHz call never touches the new entry point."""
import math
import os

import numpy as np
import pytest
from scipy.signal import resample_poly

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import _native as nat
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.engine import RESAMPLE_TILE as TILE
from echoseal_amd.identify import WatermarkIdentifier
from echoseal_amd.utils import condition_plan, resample_to, resampled_length

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEY = b"\xAA" * 32
LIST = 8
RATES = [44_100, 8_000, 16_000, 32_000, 22_050, 11_025, 96_000, 192_000]       # -> 48 000; and 48 000 -> 44 100
SHORT = [1, 2, 21, 22, 63]
SENTINEL = -7.25
DTYPES = {np.int16: nat.ES_DTYPE_I16, np.float32: nat.ES_DTYPE_F32, np.float64: nat.ES_DTYPE_F64}
GAP = 5                                                                        # poisoned samples before, between and after the clips


def _n_in_for(n_out: int, fs_in: int, fs_out: int) -> int:
    n = next(n for n in range(1, 4 * n_out + 8) if resampled_length(n, fs_in, fs_out) == n_out)
    return n


def _records():
    """(n_in, fs_in, fs_out) of one launch: every rate pair at the short lengths, the tile edges at 44.1 and 96 kHz, identities."""
    recs = [(n, f, 48_000) for f in RATES for n in SHORT] + [(n, 48_000, 44_100) for n in SHORT]
    for f in (44_100, 96_000):
        recs += [(_n_in_for(k, f, 48_000), f, 48_000) for k in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)]
    recs += [(n, 48_000, 48_000) for n in (1, 63, TILE + 1)] + [(70, 44_100, 44_100)]
    return recs


def _samples(rng, n, dtype):
    x = rng.standard_normal(n) * 0.3
    if dtype == np.int16:
        return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x.astype(dtype)


def _reference(x, fs_in, fs_out):
    src = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
    if fs_in == fs_out:
        return src.astype(np.float32)
    g = math.gcd(fs_in, fs_out)
    return resample_poly(src, fs_out // g, fs_in // g).astype(np.float32)


_CASES: dict = {}


def _case(dtype):
    """Clips, the merged descriptor table of both target rates with the clips GAP samples apart, and SciPy's outputs -- made once."""
    if dtype not in _CASES:
        rng = np.random.default_rng(2024)
        recs = _records()
        clips = [_samples(rng, n, dtype) for n, _, _ in recs]
        if dtype != np.int16:
            for k in (len(recs) - 2, len(recs) - 1):                         # identity records with signed zeros
                clips[k][::3] = -0.0
                clips[k][1::3] = 0.0
        desc = np.zeros((len(recs), 8), np.int64)
        filters, at = [], 0
        for target in (48_000, 44_100):
            sel = [i for i, r in enumerate(recs) if r[2] == target]
            cp = condition_plan([recs[i][0] for i in sel], [recs[i][1] for i in sel], target, dtype)
            desc[sel] = cp.desc
            desc[sel, 4] += at
            filters.append(cp.filters); at += cp.filters.size
        off = GAP + np.cumsum([0] + [c.size + GAP for c in clips[:-1]])
        desc[:, 0] = off
        poison = np.int16(32767) if dtype == np.int16 else dtype(np.nan)
        pool = np.full(int(off[-1]) + clips[-1].size + GAP, poison, dtype)
        if dtype != np.int16:
            pool[::2] = np.inf
        for o, c in zip(off, clips):
            pool[o:o + c.size] = c
        refs = [_reference(c, r[1], r[2]) for c, r in zip(clips, recs)]
        assert [r.size for r in refs] == desc[:, 7].tolist()
        _CASES[dtype] = (recs, clips, desc, np.concatenate(filters), pool, refs)
    return _CASES[dtype]


def _check_rows(out, refs, rep, what):
    for r, ref in enumerate(refs):
        for c in range(rep):
            row = out[r * rep + c]
            assert np.array_equal(row[:ref.size].view(np.uint8), ref.view(np.uint8)), (what, r, c)      # (all rep rows equal the one reference)
            assert (row[ref.size:] == np.float32(SENTINEL)).all(), (what, r, c)


# ------------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("rep", [1, 4])
@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_kernel_equals_scipy_bit_for_bit(engine, dtype, rep):
    recs, clips, desc, filters, pool, refs = _case(dtype)
    d = engine.device
    longest = max(r.size for r in refs)
    stride = (longest + 3) // 4 * 4 + 8
    out = torch.full((len(recs) * rep, stride), SENTINEL, dtype=torch.float32, device=d)
    pd, fd, dd = torch.from_numpy(pool).to(d), torch.from_numpy(filters).to(d), torch.from_numpy(desc).to(d)
    st = torch.cuda.current_stream(d).cuda_stream
    rc = engine._lib.es_resample_ragged_batch(engine._ctx, pd.data_ptr(), DTYPES[dtype], pd.numel(), fd.data_ptr(), fd.numel(), dd.data_ptr(),
                                              len(recs), rep, out.data_ptr(), stride, longest, st)
    assert rc == 0, engine._lib.es_last_error(engine._ctx)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    _check_rows(got, refs, rep, "pool")
    if dtype != np.int16:                                                   # the identity records' signed zeros came through
        for k in (len(recs) - 2, len(recs) - 1):
            assert np.array_equal(np.signbit(got[k * rep, :clips[k].size]), np.signbit(clips[k])) and np.signbit(clips[k]).any()


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_resample_ragged_host_and_device_clips(engine, dtype):
    recs, clips, _, _, _, refs = _case(dtype)
    for target in (48_000, 44_100):
        sel = [i for i, r in enumerate(recs) if r[2] == target]
        sub, fs, want = [clips[i] for i in sel], [recs[i][1] for i in sel], [refs[i] for i in sel]
        rows, lens = engine.resample_ragged(sub, fs, target, rep=4)
        longest = max(w.size for w in want)
        assert rows.shape == (4 * len(sub), (longest + 3) // 4 * 4) and rows.dtype == torch.float32 and lens.tolist() == [w.size for w in want]
        out = torch.full_like(rows, SENTINEL)
        dev_clips = [torch.from_numpy(c).to(engine.device) for c in sub]
        rows2, _ = engine.resample_ragged(dev_clips, fs, target, rep=4, out=out)
        assert rows2 is out
        _check_rows(out.cpu().numpy(), want, 4, ("device", target))
        host = rows.cpu().numpy()
        for r, w in enumerate(want):                                        # new rows: zeros behind the record
            assert np.array_equal(host[4 * r, :w.size].view(np.uint8), w.view(np.uint8)) and not host[4 * r:4 * r + 4, w.size:].any()
    empty, lens = engine.resample_ragged([], [], 48_000, rep=4)
    assert empty.shape == (0, 0) and lens.size == 0
    with pytest.raises(ValueError):
        engine.resample_ragged([clips[0], clips[1].astype(np.float32 if dtype != np.float32 else np.float64)], 44_100, 48_000)
    with pytest.raises(ValueError):
        engine.resample_ragged([clips[0]], 44_100, 48_000, rep=0)


def test_bad_descriptors_read_and_write_nothing_outside(engine):
    """n_out beyond the row is cut to it; offsets, lengths and filters outside the pools give no read and, without a filter, no write."""
    recs, clips, desc, filters, pool, refs = _case(np.float32)
    k = next(i for i, r in enumerate(recs) if r[1] == 44_100 and r[0] > 900)
    d = engine.device
    bad = np.stack([desc[k]] * 6)
    bad[0, 7] = 10 ** 9                                                     # n_out far beyond the row
    pool_n = pool.size - GAP                                                # the pool ends with the last clip: what lies behind it is not the pool's
    bad[1, 0] = pool_n - 3                                                  # the record runs over the pool's end: only 3 samples are its own
    bad[2, 0] = -5                                                          # negative offset: no sample
    bad[3, 4] = filters.size - 7                                            # filter over the end of the pool: nothing written
    bad[4, 2] = 0                                                           # up = 0: nothing written
    bad[5, 1] = -4                                                          # negative n_in: no sample, zeros
    stride = 512
    out = torch.full((6, stride), SENTINEL, dtype=torch.float32, device=d)
    pd, fd, dd = torch.from_numpy(pool).to(d), torch.from_numpy(filters).to(d), torch.from_numpy(bad).to(d)
    rc = engine._lib.es_resample_ragged_batch(engine._ctx, pd.data_ptr(), nat.ES_DTYPE_F32, pool_n, fd.data_ptr(), fd.numel(), dd.data_ptr(), 6, 1,
                                              out.data_ptr(), stride, 10 ** 9, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[0].view(np.uint8), refs[k][:stride].view(np.uint8))
    tail = _reference(np.concatenate((pool[pool_n - 3:pool_n], np.zeros(recs[k][0] - 3, np.float32))), 44_100, 48_000)
    assert np.isfinite(got[1]).all() and np.array_equal(got[1, :8].view(np.uint8), tail[:8].view(np.uint8))
    assert not got[2].any() and not got[5].any()
    assert (got[3] == np.float32(SENTINEL)).all() and (got[4] == np.float32(SENTINEL)).all()


# ------------------------------------------------------------------------------------------------------------------- 2. arguments
def test_invalid_arguments_are_refused_before_any_launch(engine):
    recs, clips, desc, filters, pool, refs = _case(np.float32)
    lib, ctx, d = engine._lib, engine._ctx, engine.device
    st = torch.cuda.current_stream(d).cuda_stream
    pd, fd, dd = torch.from_numpy(pool).to(d), torch.from_numpy(filters).to(d), torch.from_numpy(desc).to(d)
    stride = 2 * TILE + 4
    out = torch.full((len(recs), stride), SENTINEL, dtype=torch.float32, device=d)
    p = lambda t: t.data_ptr()

    def call(pp=p(pd), dt=nat.ES_DTYPE_F32, pn=pd.numel(), fp=p(fd), fn=fd.numel(), dp=p(dd), R=len(recs), rep=1, op=p(out), stride=stride, mx=stride):
        return lib.es_resample_ragged_batch(ctx, pp, dt, pn, fp, fn, dp, R, rep, op, stride, mx, st)
    for kw, word in ((dict(rep=0), "rep"), (dict(rep=-2), "rep"), (dict(pn=-1), "negative"), (dict(fn=-1), "negative"), (dict(R=-1), "negative"),
                     (dict(stride=-4), "negative"), (dict(mx=-1), "negative"), (dict(dt=7), "dtype"), (dict(pp=None), "null"),
                     (dict(fp=None), "null"), (dict(dp=None), "null"), (dict(op=None), "null")):
        assert call(**kw) == -1, kw                                         # ES_EINVAL
        assert word in lib.es_last_error(ctx).decode() and "es_resample_ragged_batch" in lib.es_last_error(ctx).decode(), kw
    assert call(R=0) == 0 and call(mx=0) == 0 and call(R=0, pp=None, fp=None, dp=None, op=None) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                    # nothing was launched


# ------------------------------------------------------------------------------------------------------------------- 3. capture
def test_resample_ragged_and_sync_ragged_are_capturable(engine):
    rng = np.random.default_rng(5)
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"].astype(np.float32)
    host = [resample_to(44_100, clip[:30000], 48_000)[0].astype(np.float32), clip[:5000].copy(), (rng.standard_normal(700) * 0.1).astype(np.float32)]
    fs = [44_100, 48_000, 96_000]
    d = engine.device
    clips = [torch.from_numpy(c).to(d) for c in host]
    plan = engine.condition_upload([c.size for c in host], fs, 48_000, np.float32)
    lens = torch.from_numpy(np.repeat(plan.plan.n_out.astype(np.int32), 4)).to(d)
    band = torch.arange(4, dtype=torch.uint8, device=d).repeat(3)
    rows, n_out = engine.resample_ragged(clips, fs, 48_000, rep=4)
    engine.reserve(rows.shape[0], rows.shape[1])
    ref = engine.sync_ragged(rows, lens, band)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rows2, _ = engine.resample_ragged(clips, fs, 48_000, rep=4, plan=plan)
        out = engine.sync_ragged(rows2, lens, band)
    rows2.fill_(SENTINEL); out.thr.fill_(-1.0); out.npeaks.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for r, n in enumerate(n_out.tolist()):
        assert torch.equal(rows2[4 * r:4 * r + 4, :n], rows[4 * r:4 * r + 4, :n])
        assert torch.equal(out.y[4 * r:4 * r + 4, :n], ref.y[4 * r:4 * r + 4, :n])
    assert torch.equal(out.thr, ref.thr) and torch.equal(out.peaks, ref.peaks) and torch.equal(out.npeaks, ref.npeaks)


# ------------------------------------------------------------------------------------------------------------------- 4. end to end
def _queue(fs_target=48_000):
    """[(clip as uploaded, its rate)]: the golden 3 s clip, three cuts of it and three noise clips, each at 44.1, 32 and 96 kHz; one of them
    int16, one float64; two clips left at the target rate."""
    rng = np.random.default_rng(77)
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"].astype(np.float32)
    base = [clip, clip[:100_000], clip[20_000:81_234], clip[50_000:80_011]] + [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in (63, 100, 4000)]
    queue = []
    for k, c in enumerate(base):
        for f in (44_100, 32_000, 96_000):
            g = math.gcd(f, fs_target)
            queue.append((resample_poly(c.astype(np.float64), f // g, fs_target // g).astype(np.float32), f))
    x, f = queue[4]
    queue[4] = (np.clip(np.round(x.astype(np.float64) * 32768), -32768, 32767).astype(np.int16), f)
    x, f = queue[8]
    queue[8] = (x.astype(np.float64) * 1.0000001, f)
    queue.insert(3, (clip[10_000:40_000].copy(), fs_target))
    queue.append((base[6].copy(), fs_target))
    return queue


def _host_conditioned(x, f, fs_target):
    if x.dtype == np.int16:
        x = x.astype(np.float32) / np.float32(32768)
    return np.asarray(resample_to(fs_target, x, f)[0]).astype(np.float32)


def _traced(det):
    det._trace = []; det._hdr_trace = []
    return det


def test_verify_batch_over_mixed_rates_equals_host_conditioning(engine):
    queue = _queue()
    assert {x.dtype for x, _ in queue} == {np.dtype(np.int16), np.dtype(np.float32), np.dtype(np.float64)}
    want, trace, hdr = [], [], []
    for x, f in queue:
        det = _traced(WatermarkDetector(KEY, list_size=LIST, engine=engine))
        want.append(det.verify(_host_conditioned(x, f, 48_000), 48_000))
        trace += det._trace; hdr += det._hdr_trace
    calls = []
    real = engine.resample_ragged
    engine.resample_ragged = lambda *a, **k: (calls.append(len(a[0])), real(*a, **k))[1]
    try:
        det = _traced(WatermarkDetector(KEY, list_size=LIST, engine=engine))
        got = det.verify_batch([x for x, _ in queue], [f for _, f in queue])
    finally:
        del engine.resample_ragged
    assert got == want and det._trace == trace and det._hdr_trace == hdr
    assert len(trace) > 50 and len(hdr) > 20
    assert sorted(calls) == [1, 1, len(queue) - 2]                          # ONE conditioning launch per sample type
    # a single clip through verify()
    x, f = queue[0]
    one = _traced(WatermarkDetector(KEY, list_size=LIST, engine=engine))
    ref = _traced(WatermarkDetector(KEY, list_size=LIST, engine=engine))
    assert one.verify(x, f) == ref.verify(_host_conditioned(x, f, 48_000), 48_000) and one._trace == ref._trace and one._hdr_trace == ref._hdr_trace


def test_identify_batch_over_mixed_rates_equals_host_conditioning(engine):
    queue = _queue()[:8]
    keys = [bytes(32), KEY, b"\xFF" * 32, bytes(range(32))]
    ref = WatermarkIdentifier(keys, list_size=LIST, engine=engine); ref.trace = True
    want = [ref.identify(_host_conditioned(x, f, 48_000), 48_000) for x, f in queue]
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine); ident.trace = True
    matches, traces = ident.identify_batch([x for x, _ in queue], [f for _, f in queue])
    assert matches == [w[0] for w in want] and traces == [w[1] for w in want]
    assert sum(len(t[0]) for t in traces[0]) > 20
    # ... and a fresh detector of the clip's own key on the host-conditioned clip
    det = _traced(WatermarkDetector(KEY, list_size=LIST, engine=engine))
    x, f = queue[0]
    assert det.verify(_host_conditioned(x, f, 48_000), 48_000) == (matches[0][1] is not None)
    assert (det._trace, det._hdr_trace) == (list(traces[0][1][0]), list(traces[0][1][1]))


def test_verify_batch_at_another_target_rate():
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=LIST, fs=44_100)
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"].astype(np.float32)
    queue = [(clip[:60_000], 48_000), (resample_poly(clip[:50_000].astype(np.float64), 147, 160).astype(np.float32), 44_100), (clip[60_000:90_001], 48_000)]
    want, trace, hdr = [], [], []
    for x, f in queue:
        det = _traced(WatermarkDetector(KEY, fs_target=44_100, list_size=LIST, engine=eng))
        want.append(det.verify(_host_conditioned(x, f, 44_100), 44_100))
        trace += det._trace; hdr += det._hdr_trace
    det = _traced(WatermarkDetector(KEY, fs_target=44_100, list_size=LIST, engine=eng))
    assert det.verify_batch([x for x, _ in queue], [f for _, f in queue]) == want
    assert det._trace == trace and det._hdr_trace == hdr and len(hdr) > 0
    eng.close()


def test_all_target_rate_batch_never_conditions(engine):
    queue = [(x, f) for x, f in _queue() if f == 48_000]
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"]
    clips = [x for x, _ in queue] + [np.clip(np.round(clip[:20_000] * 32767), -32767, 32767).astype(np.int16)]
    calls = []
    real = engine.resample_ragged
    engine.resample_ragged = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        WatermarkDetector(KEY, list_size=LIST, engine=engine).verify_batch(clips, 48_000)
        WatermarkIdentifier([KEY, bytes(32)], list_size=LIST, engine=engine).identify_batch(clips, [48_000] * len(clips))
        assert calls == []
        WatermarkDetector(KEY, list_size=LIST, engine=engine).verify_batch(clips, [48_000] * (len(clips) - 1) + [44_100])
        assert calls == [1, 1]                                              # (the wrapper does count: float32 and int16 launches)
    finally:
        del engine.resample_ragged
