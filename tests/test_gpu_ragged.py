"""GPU: recordings of unequal length in one batch, bit for bit against the per-record calls they replace.

- es_sync_ragged_batch against engine.sync on every record alone and against the CPU oracle on the record's own samples, with the
  rows' padding poisoned (NaN / inf for float32, full-scale samples for int16), in two row orders;
- es_plan_ragged_batch against identify.plan_reference with the row's own sample count and against es_plan_batch called per row;
- graph capture of sync_ragged after reserve;
- verify_batch / identify_batch over clips of many lengths against the clip-by-clip walk: booleans, traces, session nonce, and the
  number of sync launch sequences they cost."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from identify_cases import plan_inputs
from test_gpu_identify import KEY, LIST, N_KEYS, _clips, _keys
from echoseal_amd._native import ES_MAX_PEAKS, NativeError
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier, plan_reference
from echoseal_amd.tables import pack_tables

GOLD = os.path.join(os.path.dirname(__file__), "golden")
# below the template, one lag, the fallback with fewer than 5 lags, a frame that just fits (1215) and one that just does not (1214),
# both sides of the 4096-lag boundary (4158 / 4159 samples), and a row of several correlation segments
LENS = [0, 10, 62, 63, 64, 66, 67, 68, 1214, 1215, 1277, 4158, 4159, 5000, 20000]
T_ROW = max(LENS)


def _contents():
    """Record i of LENS[i] samples: golden-clip slices, noise, digital silence and a constant, float32."""
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"].astype(np.float32)
    rng = np.random.default_rng(11)
    recs = []
    for i, n in enumerate(LENS):
        kind = i % 4
        if n == 20000 or n == 4159 or n == 1215:
            kind = 0                                                       # the long rows carry real audio
        if kind == 0:
            r = clip[1000 * i:1000 * i + n].copy()
        elif kind == 1:
            r = rng.normal(0, 0.1, n).astype(np.float32)
        elif kind == 2:
            r = np.zeros(n, np.float32)
        else:
            r = np.full(n, 0.25, np.float32)
        assert r.size == n
        recs.append(r)
    return recs


def _batch(recs, dtype, order):
    """The padded [B, T_ROW] batch in row order `order`, padding poisoned: -> (x, lens, band) host arrays."""
    B = len(order)
    if dtype == np.float32:
        x = np.empty((B, T_ROW), np.float32)
        x[:, 0::3] = np.nan; x[:, 1::3] = np.inf; x[:, 2::3] = -np.inf
    else:
        x = np.empty((B, T_ROW), np.int16)
        x[:, 0::2] = 32767; x[:, 1::2] = -32767
    for row, i in enumerate(order):
        x[row, :LENS[i]] = recs[i]
    lens = np.array([LENS[i] for i in order], np.int32)
    band = np.array([i % 4 for i in order], np.uint8)
    return x, lens, band


@pytest.fixture(scope="module", params=["float32", "int16"])
def ragged_case(request, engine, oracle):
    """Per sample type: the records, what engine.sync gives for each alone, and the oracle's results on the record's own samples
    (computed once, shared by the tests below)."""
    dtype = np.float32 if request.param == "float32" else np.int16
    recs = _contents()
    if dtype == np.int16:
        recs = [np.clip(np.round(r * 32767), -32767, 32767).astype(np.int16) for r in recs]
    ba, tpl, _taps, _ntaps, _ = pack_tables()
    alone, orc = [], []
    for i, r in enumerate(recs):
        if r.size < 63:
            alone.append(None); orc.append(None)
            continue
        b = i % 4
        sy = engine.sync(torch.from_numpy(r.reshape(1, -1)).to(engine.device), torch.tensor([b], dtype=torch.uint8, device=engine.device))
        alone.append(sy)
        xf = r if dtype == np.float32 else r.astype(np.float32) / np.float32(32768)
        y = oracle.lfilter(ba[b, :9], ba[b, 9:], xf)
        corr = oracle.ncc(y, tpl[b])
        thr, _, _ = oracle.cfar_threshold(corr)
        orc.append((y, corr, thr, oracle.pick_peaks(corr, thr)))
    return dtype, recs, alone, orc


def _check_rows(engine, case, order):
    dtype, recs, alone, orc = case
    x, lens, band = _batch(recs, dtype, order)
    d = engine.device
    sy = engine.sync_ragged(torch.from_numpy(x).to(d), torch.from_numpy(lens).to(d), torch.from_numpy(band).to(d), keep_corr=True)
    sy2 = engine.sync_ragged(torch.from_numpy(x).to(d), lens, torch.from_numpy(band).to(d))                  # corr in the context's workspace
    assert sy.y.shape == (len(order), T_ROW) and sy.corr.shape == (len(order), T_ROW - 62) and sy2.corr is None
    assert torch.equal(sy.thr, sy2.thr) and torch.equal(sy.peaks, sy2.peaks) and torch.equal(sy.npeaks, sy2.npeaks)
    flags = 0
    for row, i in enumerate(order):
        n = LENS[i]
        if n < 63:                                                         # rtwm/detector.py:71-73
            assert int(sy.npeaks[row]) == 0 and float(sy.thr[row]) == 0.0 and bool((sy.peaks[row] == -1).all()), (i, n)
            continue
        one = alone[i]
        assert torch.equal(sy.thr[row], one.thr[0]) and torch.equal(sy.peaks[row], one.peaks[0]) and torch.equal(sy.npeaks[row], one.npeaks[0]), (i, n)
        assert torch.equal(sy.y[row, :n], one.y[0]) and torch.equal(sy2.y[row, :n], one.y[0]), (i, n)
        assert torch.equal(sy.corr[row, :n - 62], one.corr[0]), (i, n)
        y, corr, thr, (peaks, tot, fb) = orc[i]
        assert np.array_equal(y, sy.y[row, :n].cpu().numpy()), (i, n)
        assert np.array_equal(corr, sy.corr[row, :n - 62].cpu().numpy()), (i, n)
        assert thr == float(sy.thr[row]), (i, n)
        word = int(sy.npeaks[row])
        flags += word >> 30
        if not recs[i].any():
            continue                                                       # all-zero correlation: every lag ties (declared ambiguous)
        k = word & 0xFFFF
        assert k == tot and bool(word >> 30) == fb and list(sy.peaks[row, :min(k, ES_MAX_PEAKS)].cpu().numpy()) == list(peaks[:min(k, ES_MAX_PEAKS)]), (i, n)
    return flags


def test_sync_ragged_equals_per_record_sync_and_oracle(engine, ragged_case):
    flags = _check_rows(engine, ragged_case, list(range(len(LENS))))
    assert flags >= 3                                                      # the fallback branch ran (rows with fewer than 5 lags among them)


def test_sync_ragged_in_another_row_order_and_batch_size(engine, ragged_case):
    order = np.random.default_rng(1).permutation(len(LENS)).tolist()
    _check_rows(engine, ragged_case, order + order[:6][::-1])              # 21 rows: no multiple of the 4, 16 or 64 records of a block
    _check_rows(engine, ragged_case, [14])
    _check_rows(engine, ragged_case, [2, 14, 0])


def test_sync_ragged_with_full_rows_equals_sync(engine):
    rng = np.random.default_rng(3)
    for T in (63, 1300, 4159):
        x = torch.from_numpy(rng.normal(0, 0.1, (5, T)).astype(np.float32)).to(engine.device)
        band = torch.tensor([0, 1, 2, 3, 1], dtype=torch.uint8, device=engine.device)
        a = engine.sync(x, band)
        for lens in (np.full(5, T, np.int32), np.full(5, T + 1000, np.int32)):                              # (lengths are clamped to T)
            b = engine.sync_ragged(x, lens, band, keep_corr=True)
            for name in ("y", "corr", "thr", "peaks", "npeaks"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (T, name)
    neg = engine.sync_ragged(x, np.array([-5, 0, 62, 63, T], np.int32), band)                              # ... and to 0
    assert neg.npeaks[:3].tolist() == [0, 0, 0] and neg.thr[:3].tolist() == [0.0] * 3 and bool((neg.peaks[:3] == -1).all())
    assert torch.equal(neg.peaks[4], a.peaks[4]) and int(neg.npeaks[3]) == (1 | 1 << 30)


@pytest.mark.parametrize("kind", ["quad", "lane"])
def test_sync_ragged_poisoned_padding_under_the_large_batch_bandpass_kernels(engine, kind):
    """The batches above run the sixteen-lanes-per-record band-pass only.  Batches just past its threshold (four lanes per record) and
    of 262 144 records and more (one lane per record) make the same promise: poisoned padding, and every group of equally long records
    equal to engine.sync on that group alone (itself a smaller batch, i.e. another band-pass kernel; those are pinned to each other
    and to the oracle by tests/test_gpu_parity.py)."""
    cus = torch.cuda.get_device_properties(engine.device).multi_processor_count
    B, T = (16 * cus + 5, 100) if kind == "quad" else (262144 + 5, 64)
    choices = np.array([0, 40, 63, 64, 77, 100] if kind == "quad" else [10, 63, 64], np.int32)
    rng = np.random.default_rng(B)
    lens = choices[rng.integers(0, choices.size, B)]
    lens[:choices.size] = choices; lens[-1] = T
    band = (np.arange(B) % 4).astype(np.uint8)
    d = engine.device
    for dtype in (np.float32, np.int16):
        if dtype == np.float32:
            body = rng.normal(0, 0.1, (B, T)).astype(np.float32)
            x = np.where(np.arange(T)[None, :] < lens[:, None], body, np.float32(np.nan))
            x[:, 1::2] = np.where(np.arange(1, T, 2)[None, :] < lens[:, None], body[:, 1::2], np.float32(np.inf))
        else:
            body = rng.integers(-9000, 9000, (B, T)).astype(np.int16)
            x = np.where(np.arange(T)[None, :] < lens[:, None], body, np.int16(32767))
            x[:, 1::2] = np.where(np.arange(1, T, 2)[None, :] < lens[:, None], body[:, 1::2], np.int16(-32767))
        x = np.ascontiguousarray(x, dtype=dtype)
        xd, bd = torch.from_numpy(x).to(d), torch.from_numpy(band).to(d)
        sy = engine.sync_ragged(xd, lens, bd, keep_corr=True)
        for n in choices.tolist():
            idx = torch.from_numpy(np.flatnonzero(lens == n)).to(d)
            if n < 63:
                assert not sy.npeaks[idx].any() and not sy.thr[idx].any() and bool((sy.peaks[idx] == -1).all()), (kind, n)
                continue
            one = engine.sync(xd[idx, :n].contiguous(), bd[idx])
            assert torch.equal(sy.thr[idx], one.thr) and torch.equal(sy.peaks[idx], one.peaks) and torch.equal(sy.npeaks[idx], one.npeaks), (kind, n)
            assert torch.equal(sy.y[idx, :n], one.y) and torch.equal(sy.corr[idx, :n - 62], one.corr), (kind, n)
        del sy


def test_sync_ragged_argument_checks(engine):
    d = engine.device
    empty = engine.sync_ragged(torch.empty((0, 100), dtype=torch.float32, device=d), np.zeros(0, np.int32), torch.empty(0, dtype=torch.uint8, device=d))
    assert empty.thr.numel() == 0 and empty.peaks.shape == (0, ES_MAX_PEAKS)
    lib, ctx = engine._lib, engine._ctx
    assert lib.es_sync_ragged_batch(ctx, None, 0, 0, 100, None, None, None, None, None, None, None, None) == 0     # B = 0 launches nothing
    x = torch.zeros((2, 100), dtype=torch.float32, device=d)
    band = torch.zeros(2, dtype=torch.uint8, device=d)
    y = torch.empty((2, 100), dtype=torch.float64, device=d)
    thr = torch.full((2,), 7.0, dtype=torch.float64, device=d)
    peaks = torch.empty((2, ES_MAX_PEAKS), dtype=torch.int32, device=d); npk = torch.empty(2, dtype=torch.int32, device=d)
    p = lambda t: t.data_ptr()
    rc = lib.es_sync_ragged_batch(ctx, p(x), 0, 2, 100, None, p(band), p(y), None, p(thr), p(peaks), p(npk), None)  # null len_dev
    assert rc != 0 and b"null pointer" in lib.es_last_error(ctx)
    torch.cuda.synchronize()
    assert thr.tolist() == [7.0, 7.0]                                      # a refused call enqueues nothing
    with pytest.raises(NativeError):
        engine.sync_ragged(torch.zeros((2, 62), dtype=torch.float32, device=d), np.array([62, 62], np.int32), band)   # T < 63
    with pytest.raises(ValueError):
        engine.sync_ragged(x, np.array([100], np.int32), band)


# ------------------------------------------------------------------------------------------------------------------- plan
def test_plan_ragged_equals_reference_and_per_row_plan(engine):
    N = N_KEYS
    Ms = [1215, 1216, 1300, 5000, 12_000, 30_011, 48_000, 240_000]
    rng = np.random.default_rng(99)
    parts = [plan_inputs(rng, M, 3, N) for M in Ms]
    peaks = np.concatenate([p[0] for p in parts]); npeaks = np.concatenate([p[1] for p in parts])
    rowband = np.concatenate([p[2] for p in parts])
    widths = [p[4].shape[1] for p in parts]
    base = np.concatenate([p[3] + off for p, off in zip(parts, np.cumsum([0] + widths[:-1]))]).astype(np.int32)
    hok = np.concatenate([p[4] for p in parts], axis=1); hlo = np.concatenate([p[5] for p in parts], axis=1)
    hop = parts[-1][6]                                                     # the widest table: that of the longest row
    lens = np.repeat(np.array(Ms, np.int32), 3)
    perm = rng.permutation(lens.size)                                      # rows in no order of length
    peaks, npeaks, rowband, base, lens = peaks[perm], npeaks[perm], rowband[perm], base[perm], lens[perm]
    rows = lens.size
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)
    args = (d(hok), d(hlo), d(hop))
    res = engine.plan(d(peaks), d(npeaks), rowband, base, lens, *args)
    res_t = engine.plan(d(peaks), d(npeaks), rowband, base, torch.from_numpy(lens), *args)
    slot = res.slot.cpu().numpy(); ctr = res.ctr.cpu().numpy(); count = res.count.cpu().numpy(); looked = res.looked.cpu().numpy()
    assert np.array_equal(count, res_t.count.cpu().numpy()) and np.array_equal(looked, res_t.looked.cpu().numpy())
    nonempty = cut = 0
    for r in range(rows):
        one = engine.plan(d(peaks[r:r + 1]), d(npeaks[r:r + 1]), rowband[r:r + 1], base[r:r + 1], int(lens[r]), *args)
        o_slot = one.slot.cpu().numpy(); o_ctr = one.ctr.cpu().numpy(); o_count = one.count.cpu().numpy(); o_looked = one.looked.cpu().numpy()
        for k in range(N):
            p = k * rows + r
            want, want_looked = plan_reference(peaks[r], npeaks[r], int(lens[r]), int(rowband[r]), hok[k, base[r]:], hlo[k, base[r]:], hop[k])
            got = list(zip(slot[p, :count[p]].tolist(), ctr[p, :count[p]].tolist()))
            assert got == want and looked[p] == want_looked, (k, r, int(lens[r]), count[p], len(want))
            assert count[p] == o_count[k] and looked[p] == o_looked[k], (k, r)
            assert np.array_equal(slot[p, :count[p]], o_slot[k, :count[p]]) and np.array_equal(ctr[p, :count[p]], o_ctr[k, :count[p]]), (k, r)
            nonempty += bool(want); cut += len(want) == 400
    assert nonempty > 100 and cut > 0, (nonempty, cut)
    with pytest.raises(ValueError):
        engine.plan(d(peaks), d(npeaks), rowband, base, lens[:-1], *args)


# ------------------------------------------------------------------------------------------------------------------- graph capture
def test_sync_ragged_is_capturable_after_reserve(engine):
    recs = _contents()
    order = [14, 3, 12, 0, 9, 13]
    x, lens, band = _batch(recs, np.float32, order)
    d = engine.device
    xd, ld, bd = torch.from_numpy(x).to(d), torch.from_numpy(lens).to(d), torch.from_numpy(band).to(d)
    engine.reserve(len(order), T_ROW)
    ref = engine.sync_ragged(xd, ld, bd)                                   # corr in the workspace es_reserve sized
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = engine.sync_ragged(xd, ld, bd)
    for _ in range(2):
        out.thr.fill_(-1.0); out.npeaks.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.thr, ref.thr) and torch.equal(out.peaks, ref.peaks) and torch.equal(out.npeaks, ref.npeaks)
        for row, i in enumerate(order):
            assert torch.equal(out.y[row, :LENS[i]], ref.y[row, :LENS[i]])


# ------------------------------------------------------------------------------------------------------------------- end to end
CUTS = [5000, 48000, 62, 1277, 30011, 0, 1214, 12000]                      # input order is not length order
MID = 4                                                                    # the 30 011-sample clip: in the middle of the queue and of its launch


def _ragged_clips():
    """The clips of tests/test_gpu_identify.py cut to CUTS, and one int16 clip."""
    src = _clips()
    g1, g3, noise, rev, half = src[0], src[1], src[2], src[5], src[6]
    by_len = {48000: g3, 30011: half, 12000: noise, 5000: rev, 1277: g1, 1214: g1[5000:], 62: src[3], 0: src[4]}
    clips = [np.asarray(by_len[n][:n], np.float32).copy() for n in CUTS]
    assert [c.size for c in clips] == CUTS
    i16 = np.clip(np.round(g3[5000:25000] * 32767), -32767, 32767).astype(np.int16)
    return clips[:3] + [i16] + clips[3:]                                   # MID + 1 = 5: the 30 011-sample clip


def _count_syncs(engine, calls):
    real = {n: getattr(engine, n) for n in ("sync", "sync_fast", "sync_ragged")}

    def wrap(name):
        def f(frames, *a, **k):
            calls.append((name, frames.dtype, frames.shape[0]))
            return real[name](frames, *a, **k)
        return f
    for n in real:
        setattr(engine, n, wrap(n))

    def undo():
        for n in real:
            delattr(engine, n)
    return undo


def _walk(engine, clips, batched):
    det = WatermarkDetector(KEY, list_size=LIST, engine=engine); det._trace = []; det._hdr_trace = []
    if batched:
        res = det.verify_batch(clips, 48_000)
        return res, det._trace, det._hdr_trace, det.session_nonce
    res, marks = [], []
    for c in clips:
        res.append(det.verify(c, 48_000))
        marks.append((len(det._trace), len(det._hdr_trace)))
    return res, det._trace, det._hdr_trace, det.session_nonce, marks


def test_verify_batch_over_unequal_lengths_equals_the_clip_by_clip_walk(engine):
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.polar_fast import encode
    clips = _ragged_clips()
    mid = MID + 1
    assert clips[mid].size == 30011 and clips[3].dtype == np.int16
    want = _walk(engine, clips, False)
    calls: list = []
    undo = _count_syncs(engine, calls)
    try:
        got = _walk(engine, clips, True)
    finally:
        undo()
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
    assert len(want[1]) > 50 and len(want[2]) > 10
    f32 = [c for c in calls if c[1] == torch.float32]
    assert f32 == [("sync_ragged", torch.float32, 6 * 4)], calls            # six float32 clips of >= 63 samples, four bands: ONE sync call
    assert [c for c in calls if c[1] != torch.float32] == [("sync", torch.int16, 4)], calls
    # a true positive in the middle of the ragged launch (the demodulator patch of test_identify_true_positive): every candidate carries
    # the clean LLRs of a blob sealed for a counter of the middle clip's walk; that clip accepts, the session nonce is set, and the
    # later clips are walked with it -- as clip by clip
    marks = want[4]
    tr_mid = want[1][marks[mid - 1][0]:marks[mid][0]]
    assert len(tr_mid) > 10
    ctr = tr_mid[len(tr_mid) // 2][2]
    blob = SecureChannel(KEY).seal(b"ESAL" + ctr.to_bytes(4, "big") + b"\x07" * 8 + bytes(11))
    clean = torch.from_numpy((2.0 * encode(blob).astype(np.float32) - 1.0) * 6.0).to(engine.device).reshape(1, 1024)
    real_llr = engine.llr
    try:
        engine.llr = lambda *a, **k: clean.expand((k["rows"] if k.get("rows") is not None else a[0]).shape[0], 1024).contiguous()
        want2 = _walk(engine, clips, False)
        got2 = _walk(engine, clips, True)
    finally:
        engine.llr = real_llr
    assert want2[0][mid] is True and want2[3] == b"\x07" * 8
    assert got2[0] == want2[0] and got2[1] == want2[1] and got2[2] == want2[2] and got2[3] == want2[3]
    assert len(want2[1]) < len(want[1])                                    # the early return cut the middle clip's walk
    assert want2[4][-1][0] > want2[4][mid][0]                              # ... and later clips were still walked


@pytest.fixture(scope="module")
def per_clip_identify(engine):
    keys, clips = _keys(), _ragged_clips()
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine)
    ident.trace = True
    return keys, clips, [ident.identify(c, 48_000) for c in clips]


@pytest.mark.parametrize("cap", [None, 7])
def test_identify_batch_over_unequal_lengths_equals_per_clip_identify(engine, per_clip_identify, cap):
    keys, clips, want = per_clip_identify
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine)
    ident.trace = True
    if cap is not None:
        ident._pair_cap = lambda: cap
    calls: list = []
    undo = _count_syncs(engine, calls)
    try:
        matches, traces = ident.identify_batch(clips, 48_000)
    finally:
        undo()
    assert [c[0] for c in calls if c[1] == torch.float32] == ["sync_ragged"], calls
    tries = 0
    for c in range(len(clips)):
        assert [m is not None for m in matches[c]] == [m is not None for m in want[c][0]], c
        for k in range(N_KEYS):
            assert traces[c][k][0] == want[c][1][k][0], (c, k)
            assert traces[c][k][1] == want[c][1][k][1], (c, k)
            tries += len(traces[c][k][0])
    assert tries > 20 * N_KEYS
