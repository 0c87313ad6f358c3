"""GPU: live streams that arrive at other sample rates (es_resample_stream_batch).

1. The resampler alone (RxEngine.open_resampler / resample_step): float32 and int16 streams of one table pushed over the cuts of
   tests/stream_resample_cases.py -- 1, 1, hpp - 2, hpp - 1, hpp and 0 samples, chunks that finalize 1 023, 1 024 and 1 025 outputs, then
   two tiles and a bit -- against scipy.signal.resample_poly over the whole stream, bit for bit after every tick.  The CPU suite proves
   that these pushes take all four staging arms at first and later tiles.
2. The monitor: streams at 44.1, 8, 96 and 48 kHz in one table against a plain at-rate monitor that is pushed the conditioned chunks.
3. The detector: a marked clip at 44.1 kHz int16 in 882-sample chunks against an at-rate LiveMonitor.
4. The entry point's refusals.
All comparisons are of bit patterns."""
import os

import numpy as np
import pytest
from scipy.signal import resample_poly

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import stream_resample_cases as C
from echoseal_amd import _native as nat
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.monitor import SEG, resample_counts
from echoseal_amd.utils import finalized, stream_resample_plan

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEY = b"\xAA" * 32
SENTINEL = -7.25


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _u64(t):
    return t.contiguous().view(torch.int64).cpu().numpy()


def _as_f32(x):
    return x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x.astype(np.float32)


def _samples(rng, n, dtype):
    if dtype == np.int16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return (0.3 * rng.standard_normal(n)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- 1. the resampler alone
def _resampler_streams(target):
    """[(fs_in, samples, cuts)]: every pair of this target as float32 and as int16, and one float32 stream of -0.0 and 1e-30 samples."""
    rng = np.random.default_rng(target)
    out = []
    for fs_in, fs_t in C.GPU_PAIRS:
        if fs_t == target:
            cuts = C.gpu_cuts(fs_in, fs_t)
            for dtype in (np.float32, np.int16):
                out.append((fs_in, _samples(rng, sum(cuts), dtype), cuts))
    fs_in = out[0][0]
    cuts = C.gpu_cuts(fs_in, target)
    tiny = (rng.standard_normal(sum(cuts)) * 1e-30).astype(np.float32)
    tiny[::3] = -0.0
    tiny[1::7] = 0.0
    out.append((fs_in, tiny, cuts))
    return out


@pytest.mark.parametrize("target", [48_000, 44_100])
def test_chunked_resampler_equals_scipy_over_the_whole_stream(engine, target):
    streams = _resampler_streams(target)
    S = len(streams)
    assert {x.dtype for _, x, _ in streams} == {np.dtype(np.float32), np.dtype(np.int16)}
    plans = [stream_resample_plan(f, target) for f, _, _ in streams]
    refs = [resample_poly(_as_f32(x), pl.up, pl.down) for (_, x, _), pl in zip(streams, plans)]
    assert all(r.dtype == np.float32 for r in refs)
    table = engine.open_resampler([f for f, _, _ in streams], target)
    assert table.tail.shape == (S, nat.ES_RSTREAM_TAIL) and not table.tail.any() and not table.nin.any()
    cursor, pos, got = [0] * S, [0] * S, [[] for _ in range(S)]
    tick = both_types = 0
    while any(cursor[s] < len(streams[s][2]) for s in range(S)):
        named = [s for s in range(S) if cursor[s] < len(streams[s][2]) and s != tick % S]      # one stream sits every tick out
        tick += 1
        if not named:
            continue
        ids = np.array(named[::-1] if tick % 2 else named)                  # sample types interleaved, in either order
        chunks = [streams[s][1][pos[s]: pos[s] + streams[s][2][cursor[s]]] for s in ids]
        both_types += len({c.dtype for c in chunks}) == 2
        want = np.array([finalized(pos[s] + c.size, plans[s].up, plans[s].down, plans[s].y0) - finalized(pos[s], plans[s].up, plans[s].down, plans[s].y0)
                         for s, c in zip(ids, chunks)], np.int64)
        assert np.array_equal(resample_counts(table, ids, np.array([c.size for c in chunks]))[1], want)
        tail0, nin0 = table.tail.cpu().numpy().copy(), table.nin.cpu().numpy().copy()
        buf = torch.full((len(ids), int(want.max()) + 9), SENTINEL, dtype=torch.float32, device=engine.device)
        rows, counts = engine.resample_step(table, ids, chunks, out=buf)
        rows = rows.cpu().numpy()
        assert np.array_equal(counts, want), (tick, counts, want)
        tail1, nin1 = table.tail.cpu().numpy(), table.nin.cpu().numpy()
        for i, s in enumerate(ids):
            c = int(counts[i])
            assert (rows[i, c:] == np.float32(SENTINEL)).all(), (tick, s)               # the poison beyond count is intact
            got[s].append(rows[i, :c].copy())
            pos[s] += chunks[i].size
            cursor[s] += 1
            so_far = np.concatenate(got[s])
            f = finalized(pos[s], plans[s].up, plans[s].down, plans[s].y0)
            assert so_far.size == f and np.array_equal(_u32(so_far), _u32(refs[s][:f])), (tick, s, streams[s][0], c)
            seen = _as_f32(streams[s][1][:pos[s]])
            assert nin1[s] == pos[s] == table.n_in_host[s]
            assert np.array_equal(_u32(tail1[s]), _u32(np.concatenate((np.zeros(nat.ES_RSTREAM_TAIL, np.float32), seen))[-nat.ES_RSTREAM_TAIL:])), (tick, s)
        rest = np.setdiff1d(np.arange(S), ids)
        assert np.array_equal(_u32(tail1[rest]), _u32(tail0[rest])) and np.array_equal(nin1[rest], nin0[rest])
    for s in range(S):
        assert pos[s] == streams[s][1].size and np.concatenate(got[s]).size > 3 * C.TILE + C.REST_OUTPUTS
    assert both_types >= 8


def test_a_stream_at_the_target_rate_is_copied(engine):
    """up == down: F(n) = n, the chunk is copied (int16 converted), more than one tile, signed zeros kept."""
    rng = np.random.default_rng(5)
    table = engine.open_resampler([48_000, 44_100, 48_000], 48_000)
    a, b = _samples(rng, 2 * C.TILE + 7, np.float32), _samples(rng, 2 * C.TILE + 7, np.int16)
    a[::5] = -0.0
    at = 0
    for ln in (3, 0, C.TILE + 1, C.TILE + 3):
        buf = torch.full((2, ln + 12), SENTINEL, dtype=torch.float32, device=engine.device)
        rows, counts = engine.resample_step(table, [2, 0], [b[at: at + ln], a[at: at + ln]], out=buf)
        rows = rows.cpu().numpy()
        assert counts.tolist() == [ln, ln] and (rows[:, ln:] == np.float32(SENTINEL)).all()
        assert np.array_equal(_u32(rows[0, :ln]), _u32(_as_f32(b[at: at + ln]))) and np.array_equal(_u32(rows[1, :ln]), _u32(a[at: at + ln]))
        at += ln
    assert table.nin.tolist() == [at, 0, at] == table.n_in_host.tolist()


# ------------------------------------------------------------------------------------------------------------------- 2. the monitor
W, CM = 2 * SEG, 700
RATES = [44_100, 8_000, 96_000, 48_000, 48_000]
TYPES = [np.int16, np.float32, np.float32, np.float32, np.int16]


def _table_rows(table, s):
    return _u64(table.y_hist[4 * s: 4 * s + 4]), _u64(table.corr_hist[4 * s: 4 * s + 4])


def test_monitor_of_mixed_rates_equals_an_at_rate_monitor_of_the_conditioned_streams(engine):
    rng = np.random.default_rng(21)
    S, fs_t = len(RATES), int(engine.fs)
    goal = W + SEG + CM + 300                                               # past the history row: every stream crosses a compaction
    n_in = [int(goal * f / fs_t) + 400 for f in RATES]
    xs = [_samples(rng, n, t) if t == np.int16 else (0.1 * rng.standard_normal(n)).astype(np.float32) for n, t in zip(n_in, TYPES)]
    plans = [stream_resample_plan(f, fs_t) for f in RATES]
    rs = [_as_f32(x) if pl.up == pl.down else resample_poly(_as_f32(x), pl.up, pl.down) for x, pl in zip(xs, plans)]
    F = lambda s, n: n if plans[s].up == plans[s].down else finalized(n, plans[s].up, plans[s].down, plans[s].y0)
    mon = engine.open_monitor(S, window=W, chunk_max=CM, fs=RATES)
    ref = engine.open_monitor(S, window=W, chunk_max=CM)
    assert mon.rs is not None and ref.rs is None and mon.hist == ref.hist == W + SEG + CM
    pos, zero_ticks, t = [0] * S, 0, 0
    while min(F(s, pos[s]) for s in range(S)) <= goal - 300:
        sid = [s for s in range(S) if (t + s) % 4 or t < 2]                 # from the third tick on a stream sits some ticks out
        lens = []
        for s in sid:
            most = int(CM * RATES[s] / fs_t) - 2                            # finalizes at most chunk_max
            ln = (0, 1, 5, most)[t] if t < 4 else int(rng.integers(0, most + 1))
            lens.append(min(ln, xs[s].size - pos[s]))
        chunks = [xs[s][pos[s]: pos[s] + ln] for s, ln in zip(sid, lens)]
        cond = [rs[s][F(s, pos[s]): F(s, pos[s] + ln)] for s, ln in zip(sid, lens)]
        assert all(c.size <= CM for c in cond)
        zero_ticks += sum(c.size == 0 and ln > 0 for c, ln in zip(cond, lens))
        got = engine.monitor_step(mon, sid, chunks)
        want = engine.monitor_step(ref, sid, cond)
        for s, ln in zip(sid, lens):
            pos[s] += ln
        for name in ("thr", "peaks", "npeaks"):
            a, b = getattr(got, name), getattr(want, name)
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b), (name, t)
        assert np.array_equal(got.offset, want.offset) and np.array_equal(got.length, want.length) and np.array_equal(got.rows, want.rows)
        assert np.array_equal(mon.n_host, ref.n_host) and np.array_equal(mon.base_host, ref.base_host)
        assert mon.n_host.tolist() == [F(s, pos[s]) for s in range(S)] and mon.n_in_host.tolist() == pos
        assert torch.equal(mon.pos, ref.pos) and mon.rs.nin.cpu().numpy()[:3].tolist() == pos[:3]
        for s in sid:
            for a, b in zip(_table_rows(mon, s), _table_rows(ref, s)):
                assert np.array_equal(a, b), (t, s)
        t += 1
    assert zero_ticks >= 2 and (mon.base_host > 0).all() and t < 40
    # y_hist against the band-pass of the whole conditioned stream
    band = torch.from_numpy(np.asarray(mon.bands)).to(engine.device)
    for s in range(S):
        n, base = int(mon.n_host[s]), int(mon.base_host[s])
        y = engine.bpf(torch.from_numpy(np.repeat(rs[s][None, :n], 4, axis=0).copy()).to(engine.device), band)
        assert np.array_equal(_u64(mon.y_hist[4 * s: 4 * s + 4, :n - base]), _u64(y[:, base:n])), s


# ------------------------------------------------------------------------------------------------------------------- 3. the detector
def test_live_monitor_at_44100_equals_an_at_rate_monitor_of_the_conditioned_chunks(engine):
    """The golden clip's first half second, converted to 44.1 kHz int16 on the host, pushed in 882-sample chunks.  The reference's DSP cannot
    produce a decodable frame (tests/test_gpu_monitor.py), so the last pushes run with the demodulator's output replaced by the clean
    LLRs of blobs sealed for the counters asked for: that is where the yardstick reaches True.  On those mocked pushes a True says nothing
    about the conditioning -- both monitors accept whatever the resampler produced; there the conditioning is held by the traces (which
    peaks were tried, at which starts and counters), positions and windows, and on the pushes before them by the real demodulator too."""
    from echoseal_amd.polar_fast import encode
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"][:24_000].astype(np.float64)
    x = np.clip(np.round(resample_poly(clip, 147, 160) * 32768), -32768, 32767).astype(np.int16)
    pl = stream_resample_plan(44_100, 48_000)
    r = resample_poly(_as_f32(x), pl.up, pl.down)
    cuts = list(range(0, x.size, 882)) + [x.size]
    det = WatermarkDetector(KEY, list_size=8, engine=engine)
    real_llr, real_schedule = engine.llr, engine.schedule
    asked, clean = {}, {}

    def schedule(*a, ctrs=None, **k):
        asked["ctrs"] = [int(c) for c in ctrs.tolist()]
        return real_schedule(*a, ctrs=ctrs, **k)

    def llr(y, band, pn, **k):
        for c in asked["ctrs"]:
            if c not in clean:
                clean[c] = ((2.0 * encode(det.sec.seal(b"ESAL" + c.to_bytes(4, "big") + b"\x07" * 8 + bytes(11))).astype(np.float32) - 1.0) * 6.0).astype(np.float32)
        return torch.from_numpy(np.stack([clean[c] for c in asked["ctrs"]])).to(engine.device)

    def run(mon, chunk_of):
        out = []
        try:
            for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                if i == len(cuts) - 4:                                      # the last three pushes: clean LLRs
                    engine.llr, engine.schedule = llr, schedule
                ok = mon.push([chunk_of(a, b)], [0])
                out.append((ok, mon.traces(0), mon.session_nonce(0), mon.position(0), mon.window(0)))
        finally:
            engine.llr, engine.schedule = real_llr, real_schedule
        return out

    F = lambda n: finalized(n, pl.up, pl.down, pl.y0)
    yard = det.open_streams(1, chunk_max=1000, trace=True)
    want = run(yard, lambda a, b: r[F(a): F(b)])
    assert any(ok[0] for ok, *_ in want) and not want[0][0][0]              # the yardstick reaches True
    assert sum(len(tr[0]) for _, tr, *_ in want) > 20
    mon = det.open_streams(1, fs=44_100, chunk_max=1000, trace=True)
    with pytest.raises(ValueError, match="opened at 44100 Hz"):
        mon.push([x[:10]], [0], fs=48_000)
    got = run(mon, lambda a, b: x[a:b])
    assert len(got) == len(want) == len(cuts) - 1 >= 25
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[0], w[0], g[3:], w[3:])
    assert mon.received(0) == x.size and mon.position(0) == F(x.size) and mon.rate(0) == 44_100 and yard.rate(0) == 48_000
    # close, then add at another rate on the same slot: a zero tail, nothing received
    mon.close([0])
    assert list(mon.add(1, fs=8_000)) == [0] and mon.rate(0) == 8_000 and mon.received(0) == 0 == mon.position(0)
    rt = mon.table.rs
    assert not rt.tail[0].view(torch.int32).any() and int(rt.nin[0]) == 0 and rt.rate_host[0].tolist()[:2] == [6, 1]
    fresh = det.open_streams(1, fs=8_000, chunk_max=1000)
    x8 = (0.1 * np.random.default_rng(3).standard_normal(150)).astype(np.float32)
    assert mon.push([x8], [0], fs=8_000) == fresh.push([x8], [0])
    assert mon.position(0) == fresh.position(0) == 6 * 150 - 61
    assert np.array_equal(_u64(mon.table.y_hist[:4]), _u64(fresh.table.y_hist[:4])) and torch.equal(rt.tail[0], fresh.table.rs.tail[0])
    # the table grows by streams at further rates: the streams it has keep their tails
    assert list(mon.add(2, fs=[96_000, 48_000])) == [1, 2] and [mon.rate(s) for s in range(3)] == [8_000, 96_000, 48_000] and len(mon) == 3
    x96 = (0.1 * np.random.default_rng(4).standard_normal(500)).astype(np.float32)
    assert mon.push([x8[:70], x96, x96[:300]], [0, 1, 2]) == fresh.push([x8[:70]], [0]) + [False, False]
    assert [mon.position(s) for s in range(3)] == [6 * 220 - 61, finalized(500, 1, 2, 11), 300] and [mon.received(s) for s in range(3)] == [220, 500, 300]
    rt = mon.table.rs
    assert np.array_equal(_u64(mon.table.y_hist[:4]), _u64(fresh.table.y_hist[:4])) and torch.equal(rt.tail[0], fresh.table.rs.tail[0])
    assert rt.nin.tolist()[:2] == [220, 500]


# ------------------------------------------------------------------------------------------------------------------- 4. refusals
def test_c_abi_refuses_bad_records_and_writes_nothing(engine):
    table = engine.open_resampler([44_100, 8_000], 48_000)
    lib, ctx = engine._lib, engine._ctx
    x = torch.zeros((2, 64), dtype=torch.float32, device=engine.device)
    out = torch.full((2, 200), SENTINEL, dtype=torch.float32, device=engine.device)
    sid_len = torch.tensor([[0, 1], [40, 40]], dtype=torch.int64, device=engine.device)
    good = np.array([[0, 40, 0, 0, finalized(40, 160, 147, 11), 160, 147, 11], [1, 40, 0, 0, 6 * 40 - 61, 6, 1, 61]], np.int64)

    def call(rec, *, dtype=nat.ES_DTYPE_F32, R=2, n_stride=64, S=2, out_stride=200):
        rec = np.ascontiguousarray(rec, np.int64)
        return lib.es_resample_stream_batch(ctx, x.data_ptr(), dtype, R, n_stride, sid_len[0].data_ptr(), sid_len[1].data_ptr(), rec.ctypes.data, S,
                                            table.rate.data_ptr(), table.filt.data_ptr(), int(table.filters.size), table.tail.data_ptr(),
                                            table.nin.data_ptr(), out.data_ptr(), out_stride, engine._stream())

    def edit(r, w, v):
        rec = good.copy(); rec[r, w] = v
        return rec

    bad = [(edit(1, 0, 2), {}, "sid outside"), (edit(1, 0, 0), {}, "named twice"), (edit(0, 1, 65), {}, "length outside"), (edit(0, 1, -1), {}, "length outside"),
           (edit(0, 4, good[0, 4] + 1), {}, "disagree"), (edit(1, 3, 1), {}, "disagree"), (edit(0, 5, 0), {}, "rate words"), (edit(1, 7, -1), {}, "rate words"),
           (edit(0, 2, (1 << 62) // 160), {}, "62 bits"), (good, {"out_stride": 178}, "more outputs"),
           (good, {"dtype": nat.ES_DTYPE_F64}, "dtype"), (good, {"R": -1}, "negative")]
    for rec, kw, word in bad:
        assert call(rec, **kw) == -1, word                                  # ES_EINVAL
        msg = lib.es_last_error(ctx).decode()
        assert word in msg and "es_resample_stream_batch" in msg, (word, msg)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and not table.tail.any() and not table.nin.any()
    assert call(good[:0], R=0) == 0
    assert call(good) == 0
    torch.cuda.synchronize()
    c0 = int(good[0, 4])
    assert table.nin.tolist() == [40, 40] and (out[0, c0:] == SENTINEL).all() and (out[1, 179:] == SENTINEL).all() and not (out[0, :c0] == SENTINEL).any()
