"""GPU: the live monitor -- RxEngine.open_monitor / monitor_step and WatermarkDetector.open_streams / LiveMonitor.push.

The yardsticks are the existing calls on the whole stream: y_hist against eng.bpf of everything pushed so far, corr_hist against
eng.xcorr of that, a tick's thr / peaks / npeaks against eng.xcorr + eng.pick on the contiguous slice y_whole[w0 : n], verdicts and
traces against a private WatermarkDetector per stream.  Everything is compared bit for bit."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import _native as nat
from echoseal_amd.detector import FRAME_LEN, HDR_L, PEAK_LIMIT, WatermarkDetector, _Frames, _Scan
from echoseal_amd.monitor import SEG, window_start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEY = b"\xAA" * 32
N5 = 6000
CUT_A = (1, 31, 32, 33, 0, 63, 64, 65, 1215, 1216, 700)                    # + the rest of 6 000
CUTS_BPF = (CUT_A, (2999, 0), (17, 1300, 1300, 1300, 1300))
# ends one sample before, at and after multiples of 1216 (1215, 1216, 1217, 2431, 2432, 2433) and of 19 (2450, 2451, 2452); chunks shorter
# than 63 from the opening (ends 10, 30, 62, 63, 64, 94)
CUTS_XC = ((1215, 1, 1, 1214, 1, 1, 17, 1, 1), (10, 20, 32, 1, 1, 30, 62, 63))


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _band4(engine, n):
    return _dev(engine, np.tile(np.arange(4, dtype=np.uint8), n))


def _whole(engine, streams):
    """eng.bpf and eng.xcorr of whole streams of one length and sample type -> (y [4 n, T], corr [4 n, T - 62]), row 4 i + band."""
    x = _dev(engine, np.repeat(np.stack(streams), 4, axis=0))
    band = _band4(engine, len(streams))
    y = engine.bpf(x, band)
    return y, (engine.xcorr(y, band) if y.shape[1] >= 63 else None)


def _f32_streams(rng, n):
    noise = (0.1 * rng.standard_normal(n)).astype(np.float32)
    late = noise.copy(); late[: n // 3] = 0.0
    zeros = (0.1 * rng.standard_normal(n)).astype(np.float32)
    zeros[:40] = -0.0; zeros[rng.integers(0, n, n // 4)] = -0.0
    return [noise, late, (1e-30 * rng.standard_normal(n)).astype(np.float32), (1e15 * rng.standard_normal(n)).astype(np.float32), zeros]


def _i16_streams(rng, n):
    noise = rng.integers(-3000, 3000, n).astype(np.int16)
    late = noise.copy(); late[: n // 3] = 0
    return [noise, late, rng.integers(-1, 2, n).astype(np.int16), rng.choice(np.array([-32768, 32767], np.int16), n),
            np.where(rng.random(n) < 0.9, 0, noise).astype(np.int16)]


def _cut(total, cut):
    cut = list(cut)
    return cut + [total - sum(cut)]


def _run_continuity(engine, cuts):
    """Streams x cuts in ONE table; tick t pushes chunk t of every stream that still has one.  After every tick the pushed rows of y_hist
    and corr_hist are compared with the whole-stream results at every index held; -> the table."""
    rng = np.random.default_rng(5)
    kinds = _f32_streams(rng, N5) + _i16_streams(rng, N5)
    yf, cf = _whole(engine, kinds[:5])
    yi, ci = _whole(engine, kinds[5:])
    y_ref, c_ref = _u64(torch.cat((yf, yi))), _u64(torch.cat((cf, ci)))       # [40, 6000], [40, 5938]
    plan = [(k, _cut(N5, c)) for c in cuts for k in range(len(kinds))]      # stream s = (kind, its cut)
    chunk_max = max(max(c) for _, c in plan)
    window = 5 * SEG                                                        # >= 6 000: base stays 0, column = absolute index
    table = engine.open_monitor(len(plan), window=window, chunk_max=chunk_max)
    pos = [0] * len(plan)
    for t in range(max(len(c) for _, c in plan)):
        sid = [s for s, (_, c) in enumerate(plan) if t < len(c)]
        chunks = [kinds[plan[s][0]][pos[s]: pos[s] + plan[s][1][t]] for s in sid]
        empty = [s for s, c in zip(sid, chunks) if c.size == 0]
        z_before = _u64(table.z)
        tick = engine.monitor_step(table, sid, chunks)
        for s, c in zip(sid, chunks):
            pos[s] += c.size
        yh, ch, z_after = _u64(table.y_hist), _u64(table.corr_hist), _u64(table.z)
        for s in empty:                                                     # a chunk of 0 samples leaves the delay elements alone
            assert np.array_equal(z_before[4 * s: 4 * s + 4], z_after[4 * s: 4 * s + 4]), (t, s)
        for i, s in enumerate(sid):
            k, n = plan[s][0], pos[s]
            assert np.array_equal(yh[4 * s: 4 * s + 4, :n], y_ref[4 * k: 4 * k + 4, :n]), ("y", t, s, k, n)
            assert np.array_equal(ch[4 * s: 4 * s + 4, :max(n - 62, 0)], c_ref[4 * k: 4 * k + 4, :max(n - 62, 0)]), ("corr", t, s, k, n)
            assert int(tick.length[4 * i]) == n and int(tick.offset[4 * i]) == 0
        assert np.array_equal(table.pos.cpu().numpy()[:, 0], np.array(pos))
    assert pos == [N5] * len(plan)
    return table


def test_bandpass_continues_bit_for_bit_over_any_cuts(engine):
    """Five float32 and five int16 streams (noise, silence then noise, 1e-30, 1e15 / one LSB, full scale, -0.0 samples / mostly zeros), each
    cut three ways, mixed sample types in every tick: y_hist == eng.bpf(whole stream) in the uint64 view after every tick, all four
    bands; a 0-sample chunk leaves the delay elements as they are."""
    _run_continuity(engine, CUTS_BPF)


def test_correlation_history_equals_whole_stream_correlation(engine):
    """The same streams cut so that chunks end one sample before, at and after multiples of 1216 and of 19, and with chunks shorter than
    63 samples from the opening: corr_hist == eng.xcorr(eng.bpf(whole)) at every lag held, after every tick."""
    _run_continuity(engine, CUTS_XC + (CUT_A,))


def test_every_launched_bandpass_form(engine):
    """1 100 streams = 4 400 band rows, more than the sixteen-lanes-per-row form is given by es_bpf_batch on 256 CUs.  The stream
    band-pass has ONE form (a block per stream, sixteen lanes per row) that serves every record count: this runs it at that count,
    float32 and int16 streams in one tick, chunks of 33, 1 and 70 samples."""
    rng = np.random.default_rng(6)
    S, n = 1100, 104
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) if s % 3 else rng.integers(-3000, 3000, n).astype(np.int16) for s in range(S)]
    f32, i16 = [s for s in range(S) if s % 3], [s for s in range(S) if s % 3 == 0]
    ref = np.zeros((4 * S, n), np.uint64)
    for grp in (f32, i16):
        y, _ = _whole(engine, [xs[s] for s in grp])
        ref[(4 * np.array(grp)[:, None] + np.arange(4)).reshape(-1)] = _u64(y)
    table = engine.open_monitor(S, window=2 * SEG, chunk_max=70)
    at = 0
    for ln in (33, 1, 70):
        engine.monitor_step(table, np.arange(S), [x[at: at + ln] for x in xs])
        at += ln
        assert np.array_equal(_u64(table.y_hist[:, :at]), ref[:, :at]), ln
    cr = engine.xcorr(_dev(engine, ref.view(np.float64)), _band4(engine, S))
    assert np.array_equal(_u64(table.corr_hist[:, : n - 62]), _u64(cr))


W8, CM8, N8 = 3648, 1300, 14_800


def _marked(engine, rng, n, ctr0=0, ampl=0.05):
    host = (ampl * rng.standard_normal(n)).astype(np.float32)
    return engine.embed(KEY, host[None, :], ctr0=ctr0, seed=11).audio[0].cpu().numpy()


def _slice_pick(engine, y_whole, w0, n):
    """eng.xcorr + eng.pick on the contiguous slice y_whole[:, w0 : n] of one stream's four rows -> (thr u64, peaks, npeaks)."""
    if n - w0 < 63:
        return np.zeros(4, np.uint64), np.full((4, nat.ES_MAX_PEAKS), -1, np.int32), np.zeros(4, np.int32)
    ys = y_whole[:, w0:n].contiguous()
    thr, peaks, npeaks = engine.pick(engine.xcorr(ys, _band4(engine, 1)))
    return _u64(thr), peaks.cpu().numpy(), npeaks.cpu().numpy()


def test_window_pick_and_compaction(engine):
    """W = 3 648, chunk_max = 1 300 and the smallest history row, 6 164 columns.  A row is moved down only when a chunk would not fit and
    the new base is the window's start, at least n - W rounded up to 1216: the moves come after samples 6 164, 9 812 and 13 460 at the
    earliest, so the streams run to 14 800 samples for three of them.  Streams: quiet noise with embedded frames (peaks above the
    threshold), plain noise (fallback rows), silence (correlation identically zero) and one that never reaches 63 samples.  Per tick,
    thr / peaks / npeaks (bit 30 included) equal eng.xcorr + eng.pick on y_whole[w0 : n]; the window's part of corr_hist equals the
    whole-stream correlation."""
    rng = np.random.default_rng(8)
    xs = [_marked(engine, rng, N8, ampl=1e-4), (0.1 * rng.standard_normal(N8)).astype(np.float32), np.zeros(N8, np.float32),
          (0.1 * rng.standard_normal(50)).astype(np.float32)]
    y_all, c_all = _whole(engine, xs[:3])
    c_all = _u64(c_all)
    y_short, _ = _whole(engine, [np.pad(xs[3], (0, 20))])
    lens = [1300, 1216, 1215, 1, 0, 700, 1300, 63, 62, 1217, 19, 1300, 1300, 608, 1300, 1300, 1300]
    lens += [N8 - sum(lens)]
    assert 0 < lens[-1] <= CM8
    table = engine.open_monitor(4, window=W8, chunk_max=CM8)
    assert table.hist == W8 + SEG + CM8
    at, moves, fallback, real = 0, 0, 0, 0
    for t, ln in enumerate(lens):
        sid = [0, 1, 2] + ([3] if t < 3 else [])
        chunks = [x[at: at + ln] for x in xs[:3]] + ([xs[3][(0, 20, 40)[t]: (20, 40, 50)[t]]] if t < 3 else [])
        base_before = table.base_host.copy()
        tick = engine.monitor_step(table, sid, chunks)
        at += ln
        moves += int(table.base_host[0] != base_before[0])
        assert (table.base_host[:3] == table.base_host[0]).all() and table.base_host[0] % SEG == 0
        thr, peaks, npeaks = _u64(tick.thr), tick.peaks.cpu().numpy(), tick.npeaks.cpu().numpy()
        ch = _u64(table.corr_hist)
        w0 = int(window_start(at, W8))
        for i, s in enumerate(sid):
            if s < 3:
                want = _slice_pick(engine, y_all[4 * s: 4 * s + 4], w0, at)
                assert (int(tick.offset[4 * i]), int(tick.length[4 * i])) == (w0 - int(table.base_host[s]), at - w0)
                if at - w0 > 62:
                    c0 = w0 - int(table.base_host[s])
                    assert np.array_equal(ch[4 * s: 4 * s + 4, c0: c0 + at - w0 - 62], c_all[4 * s: 4 * s + 4, w0: at - 62]), (t, s)
            else:
                want = _slice_pick(engine, y_short, 0, (20, 40, 50)[t])
            got = (thr[4 * i: 4 * i + 4], peaks[4 * i: 4 * i + 4], npeaks[4 * i: 4 * i + 4])
            for g, w, what in zip(got, want, ("thr", "peaks", "npeaks")):
                assert np.array_equal(g, w), (what, t, s, g, w)
            if s == 0:
                real += int(((npeaks[4 * i: 4 * i + 4] >> 30) == 0).sum())
            if s == 1:
                fallback += int(((npeaks[4 * i: 4 * i + 4] >> 30) & 1).sum())
    assert moves >= 3, moves
    assert real > 0 and fallback > 0, (real, fallback)


def _reference_scan(engine, det, y_whole, w0, n):
    """One clip's scan assembled from the calls that existed before the monitor, on the contiguous slice y_whole[:, w0 : n] whose rows are
    in the detector's band order: eng.xcorr + eng.pick, eng.header at the fitting peaks, then _scan_decide band by band."""
    order = det._band_order()
    bid = np.array([det._band_id(b) for b in order], np.uint8)
    ys = y_whole[:, w0:n].contiguous()
    thr, peaks, npeaks = engine.pick(engine.xcorr(ys, _dev(engine, bid)))
    pk, npk = peaks.cpu().numpy(), npeaks.cpu().numpy() & 0xFFFF
    rows, starts = [], []
    for r in range(4):
        for st in pk[r, :min(int(npk[r]), pk.shape[1], PEAK_LIMIT)]:
            if st + FRAME_LEN <= n - w0:
                rows.append(r); starts.append(int(st))
    rows, starts = np.array(rows, np.int64), np.array(starts, np.int64)
    src, hdr = None, (np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0))
    if rows.size:
        src = _Frames(ys, rows, starts)
        ok, val, score = engine.header(ys, _dev(engine, bid[rows]), _dev(engine, np.packbits(det.sec.pn_bits(0, HDR_L)).reshape(1, -1)),
                                       rows=_dev(engine, rows.astype(np.int32)), start=_dev(engine, starts.astype(np.int32)))
        hdr = (ok.cpu().numpy().astype(bool), val.cpu().numpy().astype(np.int64), score.cpu().numpy().astype(np.float64))
    scan = _Scan(order, src, rows, np.arange(rows.size), starts, hdr)
    return any(det._scan_decide(scan, bi) for bi in range(4))               # (any() stops at the first True, like the walk)


def test_verdicts_and_traces_equal_a_private_detector_per_stream(engine):
    """Three streams (noise with embedded frames, a golden clip, plain noise) at list size 8, W = 3 648.  While n <= W a push equals
    WatermarkDetector.verify(everything so far) of a private detector per stream: result, _trace and _hdr_trace.  Afterwards it equals
    the scan assembled from the existing calls on the slice y_whole[w0 : n].  The reference's DSP cannot produce a decodable frame, so,
    as tests/test_detector.py::test_try_decode_frame_true_positive does, the last ticks run with the demodulator's output replaced by
    clean LLRs of sealed blobs: streams accept and lock to the blobs' nonce, blobs with another nonce are then refused by the locked
    streams and accepted by a stream opened in between -- the per-stream session_nonce path, against the private detectors."""
    from echoseal_amd.polar_fast import encode
    rng = np.random.default_rng(9)
    g = np.load(os.path.join(GOLD, "verify_trace.npz"))
    n_all = 9000
    xs = [_marked(engine, rng, n_all), g["clip"][:n_all].astype(np.float32), (0.1 * rng.standard_normal(n_all)).astype(np.float32),
          (0.1 * rng.standard_normal(n_all)).astype(np.float32)]
    det = WatermarkDetector(KEY, list_size=8, engine=engine)
    order = det._band_order()
    bid = np.array([det._band_id(b) for b in order], np.uint8)
    y_all = engine.bpf(_dev(engine, np.repeat(np.stack(xs), 4, axis=0)), _dev(engine, np.tile(bid, len(xs))))
    mon = det.open_streams(3, window_s=W8 / 48_000, chunk_max=CM8, trace=True)
    assert mon.table.window == W8 and list(mon.table.bands) == list(bid)
    refs = [WatermarkDetector(KEY, list_size=8, engine=engine) for _ in xs]
    pos = [0] * len(xs)

    def tick(sid, ln):
        got = mon.push([xs[s][pos[s]: pos[s] + ln] for s in sid], sid)
        for s, ok in zip(sid, got):
            pos[s] += ln
            ref = refs[s]
            ref._trace, ref._hdr_trace = [], []
            w0, n = mon.window(s)
            assert (w0, n) == (int(window_start(pos[s], W8)), pos[s]) and mon.position(s) == n
            if w0 == 0:
                want = ref.verify(xs[s][:n], 48_000)
            else:
                want = _reference_scan(engine, ref, y_all[4 * s: 4 * s + 4], w0, n)
            tr, htr = mon.traces(s)
            assert ok == want and tr == ref._trace and htr == ref._hdr_trace, (s, n, w0, ok, want, len(tr), len(ref._trace))
            assert mon.session_nonce(s) == ref.session_nonce, (s, n)
        return got

    tried = 0
    for ln in (40, 1260, 1216, 1130, 1300, 1300):                          # n = 40, 1300, 2516, 3646 (<= W), then 4946, 6246 (windows cut at w0 > 0)
        tick([0, 1, 2], ln)
        tried += sum(len(mon.traces(s)[0]) for s in range(3))
    assert tried > 20
    assert all(mon.session_nonce(s) is None for s in range(3))
    # accepted frames: every candidate's demodulator output is replaced by the clean LLRs of a blob sealed for that candidate's own
    # counter (the counters are those of the schedule call that precedes each demodulation), so a stream accepts the first candidate it
    # tries unless its session nonce says otherwise
    real_llr, real_schedule = engine.llr, engine.schedule
    asked = {}

    def schedule(*a, ctrs=None, **k):
        asked["ctrs"] = [int(c) for c in ctrs.tolist()]
        return real_schedule(*a, ctrs=ctrs, **k)
    try:
        engine.schedule = schedule
        for nonce8, fresh in ((b"\x07" * 8, False), (b"\x09" * 8, True)):
            clean = {}

            def llr(y, band, pn, **k):
                for c in asked["ctrs"]:
                    if c not in clean:
                        blob = det.sec.seal(b"ESAL" + c.to_bytes(4, "big") + nonce8 + bytes(11))
                        clean[c] = ((2.0 * encode(blob).astype(np.float32) - 1.0) * 6.0).astype(np.float32)
                return torch.from_numpy(np.stack([clean[c] for c in asked["ctrs"]])).to(engine.device)
            engine.llr = llr
            locked = {s: mon.session_nonce(s) for s in range(3)}
            if fresh:                                                       # a stream opened now accepts the second nonce ...
                assert list(mon.add(1)) == [3] and len(mon) == 4
                tick([3], 1300)
                tick([3, 0, 1, 2], 1216)
                tick([3], 1216)
                assert mon.session_nonce(3) == nonce8
                assert any(v == b"\x07" * 8 for v in locked.values())
                assert all(mon.session_nonce(s) == v for s, v in locked.items() if v is not None)     # ... the locked ones stay locked
            else:
                got = tick([0, 1, 2], 1216)
                assert any(got), got
                assert all(mon.session_nonce(s) == (nonce8 if ok else None) for s, ok in zip(range(3), got))
    finally:
        engine.llr, engine.schedule = real_llr, real_schedule


def _table_bytes(table):
    return [t.detach().cpu().numpy().tobytes() for t in (table.z, table.pos, table.y_hist, table.corr_hist)]


def test_streams_are_independent(engine):
    """The same pushes grouped into ticks three ways and in permuted stream order give byte-identical tables and identical verdicts; a
    stream a tick does not name keeps every byte of its rows and state; a slot that is closed and reopened behaves as a fresh stream."""
    rng = np.random.default_rng(10)
    S = 4
    seqs = [[int(v) for v in rng.choice([0, 1, 62, 63, 700, 1215, 1216, 1300, 1299, 1300], 9)] for _ in range(S)]
    xs = [(0.1 * rng.standard_normal(sum(q))).astype(np.float32) for q in seqs]
    xs[1] = (xs[1] * 20000).astype(np.int16)

    def chunk(s, k):
        a = sum(seqs[s][:k])
        return xs[s][a: a + seqs[s][k]]

    def run(groups):
        det = WatermarkDetector(KEY, list_size=1, engine=engine)
        mon = det.open_streams(S, window_s=W8 / 48_000, chunk_max=CM8)
        verdicts = {}
        for k in range(9):
            for grp in groups(k):
                before = _table_bytes(mon.table) if k == 6 else None
                for s, ok in zip(grp, mon.push([chunk(s, k) for s in grp], grp)):
                    verdicts[(s, k)] = ok
                if before is not None:                                      # rows and state of the streams this tick did not name
                    for s in set(range(S)) - set(grp):
                        z, pos, yh, ch = (np.frombuffer(b, np.uint8) for b in before)
                        zz, pp, yy, cc = (np.frombuffer(b, np.uint8) for b in _table_bytes(mon.table))
                        H8 = mon.table.hist * 8
                        for a, b, w in ((z, zz, 64), (yh, yy, H8), (ch, cc, H8)):
                            assert np.array_equal(a[4 * s * w: 4 * (s + 1) * w], b[4 * s * w: 4 * (s + 1) * w]), (s, k)
                        assert np.array_equal(pos[16 * s: 16 * s + 16], pp[16 * s: 16 * s + 16])
        return mon, verdicts

    mon_a, va = run(lambda k: [[0, 1, 2, 3]])
    mon_b, vb = run(lambda k: [[s] for s in range(S)])
    mon_c, vc = run(lambda k: [[3, 1], [2, 0]] if k % 2 else [[2, 3, 0], [1]])
    assert va == vb == vc
    assert _table_bytes(mon_a.table) == _table_bytes(mon_b.table) == _table_bytes(mon_c.table)
    assert int(mon_a.table.base_host.max()) > 0                            # rows were moved down on the way
    # close and reopen slot 1: the reopened slot replays stream 2's chunks and must end exactly as slot 2 did
    mon_a.close([1])
    assert len(mon_a) == S - 1
    with pytest.raises(ValueError):
        mon_a.push([chunk(1, 0)], [1])
    assert list(mon_a.add(1)) == [1]
    for k in range(9):
        assert mon_a.push([chunk(2, k)], [1]) == [va[(2, k)]]
    z, pos, yh, ch = (t.cpu().numpy() for t in (mon_a.table.z, mon_a.table.pos, mon_a.table.y_hist, mon_a.table.corr_hist))
    assert np.array_equal(z[4:8].view(np.uint64), z[8:12].view(np.uint64)) and np.array_equal(pos[1], pos[2])
    assert np.array_equal(yh[4:8].view(np.uint64), yh[8:12].view(np.uint64)) and np.array_equal(ch[4:8].view(np.uint64), ch[8:12].view(np.uint64))


def test_c_abi_refuses_bad_records_and_writes_nothing(engine):
    """Through the host-checked record only (the device copies hold a valid tick): a sid outside the table, a sid named twice, an
    over-long chunk and a chunk that does not fit its row are each ES_EINVAL from both record-checked entry points, and no byte of
    the table changes."""
    rng = np.random.default_rng(12)
    table = engine.open_monitor(3, window=2 * SEG, chunk_max=64)
    engine.monitor_step(table, [0, 1, 2], [(0.1 * rng.standard_normal(64)).astype(np.float32)] * 3)
    H, S = table.hist, table.n
    good = np.array([[0, 64, 64, 0, 0], [1, 64, 64, 0, 0]], np.int64)
    rec_d = _dev(engine, np.ascontiguousarray(good.T))
    x = _dev(engine, (0.1 * rng.standard_normal((2, 64))).astype(np.float32))
    before = _table_bytes(table)
    p = lambda t: t.data_ptr()

    def both(rec):
        rec = np.ascontiguousarray(rec, np.int64)
        a = engine._lib.es_bpf_stream_batch(engine._ctx, p(x), nat.ES_DTYPE_F32, 2, 64, *(p(rec_d[w]) for w in range(5)), rec.ctypes.data, S, H,
                                            p(table.band), p(table.z), p(table.pos), p(table.y_hist), p(table.corr_hist), engine._stream())
        b = engine._lib.es_xcorr_stream_batch(engine._ctx, p(table.y_hist), 2, 64, p(rec_d[0]), p(rec_d[1]), p(rec_d[2]), rec.ctypes.data, S, H,
                                              p(table.band), p(table.corr_hist), engine._stream())
        torch.cuda.synchronize()
        return a, b

    bad = {"sid outside": [[3, 64, 64, 0, 0], good[1]], "sid negative": [[-1, 64, 64, 0, 0], good[1]], "sid twice": [good[0], good[0]],
           "over-long": [[0, 65, 64, 0, 0], good[1]], "negative length": [[0, -1, 64, 0, 0], good[1]],
           "does not fit": [[0, 64, H - 63, 0, 0], good[1]], "column outside": [[0, 0, H + 1, 0, 0], good[1]],
           "move off the grid": [[0, 64, 64, 19, 0], good[1]], "base off the grid": [[0, 64, 64, 0, 19], good[1]]}
    EINVAL = -1
    for what, rec in bad.items():
        assert both(rec) == (EINVAL, EINVAL), what
        assert _table_bytes(table) == before, what
    assert both(good) == (0, 0)                                             # the valid tick the device copies hold goes through
    assert _table_bytes(table) != before
