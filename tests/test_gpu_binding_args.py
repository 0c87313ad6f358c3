"""GPU: what each RxEngine method hands to the C ABI, argument by argument.

ctypes converts a pointer of any kind to `void*`, so two tensors swapped in a call are seen by nothing but the values that come back, and
only where a test happens to look at them.  Here the `_lib` of one engine (list_size_max=8) is a pass-through proxy that logs every
`es_*_batch` call with all its arguments, and for every public method whose arguments the caller can see the logged tuple is compared,
element by element, with one written out below from include/echoseal_hip.h: the context first, the `data_ptr()` of the inputs and of the
returned tensors, the sizes, None where an optional output is off, the stream last.

Tensors a method makes for itself come from the engine's own helpers (`_ctr_dev`, `_dev`); those are watched on the instance, so their
results are visible too.  Where a pointer stays out of sight (a staging buffer, the int32 copy of `hop_row`), what is asserted is its
relation to its neighbours -- the byte offsets the method derives -- or, failing that, that it is a pointer no other argument holds.

Shapes are the smallest at which every call still does work: 4 records of 1 215 samples, list size 2, 2 keys, 2 live streams with a chunk
of either sample type, one 2 048-sample clip."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
from echoseal_amd.embedder import WatermarkEmbedder
from echoseal_amd.utils import db_to_lin

KEY, KEY2 = b"\xAA" * 32, b"\x5C" * 32
B, T, L = 4, 1215, 2
OTHER = object()                     # a pointer the caller cannot see: an int no other argument of the call holds


class _Lib:
    """Pass-through proxy of the ctypes library: logs every entry point that takes a stream, with all its arguments."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.endswith("_batch"):
            return fn

        def call(*args):
            self._log.append((name,) + args)
            return fn(*args)
        return call


def P(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def rig():
    """The engine behind the proxy, its log, and the inputs every case reads (never written)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=8)
    dev = eng.device
    f32, _ = eng.synthetic_frames(KEY, 0, B)
    sec = WatermarkEmbedder(KEY).sec
    pn, band = eng.schedule(sec._prng.sub_key, KEY, ctr0=0, n=B)
    hdr = torch.from_numpy(np.packbits(sec.pn_bits(0, 128))).to(dev).repeat(B, 1).contiguous()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    i64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    r = SimpleNamespace(eng=eng, log=[], dev=dev, f32=f32, i16=(f32 * 8000.0).to(torch.int16), pn=pn, band=band, hdr=hdr, sec=sec, i32=i32, i64=i64,
                        rows=i32([3, 2, 1, 0]), start=i32([0, 0, 0, 0]), ctrs=i64([0, 1, 2, 3]), kidx=i32([0, 1, 1, 0]),
                        mk=torch.from_numpy(np.frombuffer(KEY + KEY2, np.uint8).reshape(2, 32).copy()).to(dev))
    r.side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    eng._lib = _Lib(eng._lib, r.log)
    yield r
    torch.cuda.synchronize()
    eng.close()


@pytest.fixture(autouse=True)
def _on_a_stream_of_its_own(rig):
    """Every case runs on a stream that is not the default one, so the stream argument is a handle and not 0."""
    with torch.cuda.stream(rig.side):
        yield
    torch.cuda.synchronize()


def run(r, fn):
    """-> (what fn returned, the calls it logged)."""
    del r.log[:]
    out = fn()
    return out, list(r.log)


def same(r, got, name, *want):
    want = (name, r.eng._ctx) + want + (r.eng._stream(),)
    assert got[0] == name and len(got) == len(want), (got[0], len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if w is OTHER:
            assert isinstance(g, int) and g and g not in [x for j, x in enumerate(got) if j != i], (name, i, g)
        else:
            assert (g is None) == (w is None) and g == w and isinstance(g, float) == isinstance(w, float), (name, i, g, w)


def one(r, fn):
    out, calls = run(r, fn)
    assert len(calls) == 1, [c[0] for c in calls]
    return out, calls[0]


def watch(monkeypatch, eng, name) -> list:
    """The results of the engine's helper `name` from here on, in order."""
    orig, seen = getattr(eng, name), []

    def helper(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]
    monkeypatch.setattr(eng, name, helper)
    return seen


@pytest.fixture(scope="module")
def synced(rig):
    """Band-pass and sync outputs the later stages read, made once."""
    r = rig
    y, y32 = r.eng.bpf2(r.f32, r.band)
    thr, peaks, npeaks, flags = r.eng.sync_fused(y, y32, r.band)
    llr = r.eng.llr(y, r.band, r.pn, variant=0)
    scl = r.eng.scl(llr, list_size=L, skip_if_hard_ok=False)
    torch.cuda.synchronize()
    return SimpleNamespace(y=y, y32=y32, peaks=peaks, npeaks=npeaks, llr=llr, scl=scl)


@pytest.mark.parametrize("kind", ["i16", "f32"])
def test_band_pass_and_ragged_sync(rig, kind):
    r, e = rig, rig.eng
    x, dt = (r.i16, nat.ES_DTYPE_I16) if kind == "i16" else (r.f32, nat.ES_DTYPE_F32)
    y, c = one(r, lambda: e.bpf(x, r.band))
    same(r, c, "es_bpf_batch", P(x), dt, B, T, P(r.band), P(y))
    (y, y32), c = one(r, lambda: e.bpf2(x, r.band))
    same(r, c, "es_bpf2_batch", P(x), dt, B, T, P(r.band), P(y), P(y32))
    lens = r.i32([1215, 1000, 700, 63])
    for keep in (False, True):
        s, c = one(r, lambda: e.sync_ragged(x, lens, r.band, keep_corr=keep))
        assert (s.corr is not None) == keep
        same(r, c, "es_sync_ragged_batch", P(x), dt, B, T, P(lens), P(r.band), P(s.y), P(s.corr), P(s.thr), P(s.peaks), P(s.npeaks))


def test_sync_stages(rig, synced):
    r, e, s = rig, rig.eng, synced
    (thr, peaks, npeaks, flags), c = one(r, lambda: e.sync_fused(s.y, s.y32, r.band))
    same(r, c, "es_sync_fused_batch", P(s.y32), P(s.y), B, T, P(r.band), P(thr), P(peaks), P(npeaks), P(flags))
    corr32, c = one(r, lambda: e.xcorr32(s.y32, r.band))
    same(r, c, "es_xcorr32_batch", P(s.y32), B, T, P(r.band), P(corr32))
    (thr, peaks, npeaks, flags), c = one(r, lambda: e.pick_exact(corr32, s.y, r.band))
    same(r, c, "es_pick_exact_batch", P(corr32), P(s.y), B, T, P(r.band), P(thr), P(peaks), P(npeaks), P(flags))
    corr, c = one(r, lambda: e.xcorr(s.y, r.band))
    same(r, c, "es_xcorr_batch", P(s.y), B, T, P(r.band), P(corr))
    (thr, peaks, npeaks), c = one(r, lambda: e.pick(corr))
    same(r, c, "es_pick_batch", P(corr), B, T - 62, P(thr), P(peaks), P(npeaks))


def test_demodulator_and_header_both_arms(rig, synced):
    r, e, s = rig, rig.eng, synced
    # plain arm: start goes through as it is given
    out, c = one(r, lambda: e.llr(s.y, r.band, r.pn, variant=1))
    same(r, c, "es_llr_batch", P(s.y), B, T, None, P(r.band), P(r.pn), 1, P(out), None, None)
    (out, best, score), c = one(r, lambda: e.llr(s.y, r.band, r.pn, start=r.start, variant=0, want_diag=True))
    same(r, c, "es_llr_batch", P(s.y), B, T, P(r.start), P(r.band), P(r.pn), 0, P(out), P(best), P(score))
    (ok, val, score), c = one(r, lambda: e.header(s.y, r.band, r.hdr))
    same(r, c, "es_header_batch", P(s.y), B, T, None, P(r.band), P(r.hdr), P(ok), P(val), P(score), None)
    (ok, val, score, best), c = one(r, lambda: e.header(s.y, r.band, r.hdr, start=r.start, want_diag=True))
    same(r, c, "es_header_batch", P(s.y), B, T, P(r.start), P(r.band), P(r.hdr), P(ok), P(val), P(score), P(best))
    # in place: rows= with a start per record, and start="peak" on the peaks of a sync call
    mine = torch.empty((B, 1024), dtype=torch.float32, device=r.dev)
    out, c = one(r, lambda: e.llr(s.y, r.band, r.pn, start=r.start, rows=r.rows, variant=1, out=mine))
    assert out is mine
    same(r, c, "es_llr_at_batch", P(s.y), B, T, B, P(r.rows), P(r.start), 1, P(r.band), P(r.pn), 1, P(mine), None, None)
    (out, best, score), c = one(r, lambda: e.llr(s.y, r.band, r.pn, start="peak", peaks=s.peaks, want_diag=True))
    same(r, c, "es_llr_at_batch", P(s.y), B, T, B, None, P(s.peaks), nat.ES_MAX_PEAKS, P(r.band), P(r.pn), 0, P(out), P(best), P(score))
    (ok, val, score), c = one(r, lambda: e.header(s.y, r.band, r.hdr, rows=r.rows))
    same(r, c, "es_header_at_batch", P(s.y), B, T, B, P(r.rows), None, 1, P(r.band), P(r.hdr), P(ok), P(val), P(score), None)
    (ok, val, score, best), c = one(r, lambda: e.header(s.y, r.band, r.hdr, start="peak", peaks=s.peaks, rows=r.rows, want_diag=True))
    same(r, c, "es_header_at_batch", P(s.y), B, T, B, P(r.rows), P(s.peaks), nat.ES_MAX_PEAKS, P(r.band), P(r.hdr), P(ok), P(val), P(score), P(best))


def test_list_decoder_and_selection(rig, synced, monkeypatch):
    r, e, s = rig, rig.eng, synced
    for skip in (True, False):
        res, c = one(r, lambda: e.scl(s.llr, list_size=L, skip_if_hard_ok=skip))
        same(r, c, "es_scl_batch", P(s.llr), nat.ES_DTYPE_F32, B, L, int(skip), P(res.hard_info), P(res.hard_ok), P(res.cand_info), P(res.cand_metric),
             P(res.cand_ok), P(res.ncand))
    q = s.scl
    tail = lambda out: (P(q.hard_info), P(q.hard_ok), P(q.cand_info), P(q.cand_metric), P(q.cand_ok), P(q.ncand), P(out[0]), P(out[1]), P(out[2]))
    out, c = one(r, lambda: e.select(q))
    same(r, c, "es_select_batch", None, None, B, L, *tail(out))
    ctr = watch(monkeypatch, e, "_ctr_dev")
    out, c = one(r, lambda: e.select(q, key32=KEY, ctrs=r.ctrs))
    same(r, c, "es_select_batch", KEY, P(ctr[-1]), B, L, *tail(out))
    ring = e.keyring(r.mk)
    out, c = one(r, lambda: e.select(q, ring=ring, key_idx=r.kidx, ctrs=r.ctrs))
    same(r, c, "es_select_keyed_batch", P(ring.ring), 2, P(r.kidx), P(ctr[-1]), B, L, *tail(out))
    assert len(ctr) == 2


def test_schedules_and_key_ring(rig, monkeypatch):
    r, e = rig, rig.eng
    aes = r.sec._prng.sub_key
    (pn, band), c = one(r, lambda: e.schedule(aes, KEY, ctr0=5, n=B))
    same(r, c, "es_schedule_batch", bytes(aes), KEY, None, 5, B, P(pn), P(band))
    ctr = watch(monkeypatch, e, "_ctr_dev")
    (pn, band), c = one(r, lambda: e.schedule(aes, KEY, r.ctrs))
    same(r, c, "es_schedule_batch", bytes(aes), KEY, P(ctr[-1]), 0, B, P(pn), P(band))
    ring, c = one(r, lambda: e.keyring(r.mk))
    assert ring.n == 2
    same(r, c, "es_keyring_derive_batch", P(r.mk), 2, P(ring.ring))
    (pn, band), c = one(r, lambda: e.schedule_keyed(ring, r.kidx, r.ctrs))
    same(r, c, "es_schedule_keyed_batch", P(ring.ring), 2, P(r.kidx), P(ctr[-1]), B, P(pn), P(band))
    (pn, band), c = one(r, lambda: e.schedule_keyed(ring, r.kidx, r.ctrs, want_pn=False))
    assert pn is None
    same(r, c, "es_schedule_keyed_batch", P(ring.ring), 2, P(r.kidx), P(ctr[-1]), B, None, P(band))
    hop, c = one(r, lambda: e.hop_window(ring, r.i64([0, 7, 9]), 403))
    assert hop.shape == (2, 3, 403)
    same(r, c, "es_hop_window_batch", P(ring.ring), 2, P(ctr[-1]), 3, 403, P(hop))


def test_plan_three_arms(rig, synced, monkeypatch):
    r, e, s = rig, rig.eng, synced
    N, C, Pk = 2, 203, B                                # two keys, ceil(1215 / 1215) + 201 + 1 counters, one fitting peak per row
    rowband = r.band.clone()
    base = r.i32([0, 1, 2, 3])
    hok = torch.ones((N, Pk), dtype=torch.uint8, device=r.dev)
    lo16 = torch.zeros((N, Pk), dtype=torch.int32, device=r.dev)
    hop = torch.zeros((N, C), dtype=torch.uint8, device=r.dev)
    head = (P(s.peaks), P(s.npeaks), P(rowband), P(base), B)
    outs = lambda res: (P(res.slot), P(res.ctr), P(res.count), P(res.looked))
    res, c = one(r, lambda: e.plan(s.peaks, s.npeaks, rowband, base, T, hok, lo16, hop))
    same(r, c, "es_plan_batch", *head, T, P(hok), P(lo16), Pk, P(hop), N, C, *outs(res))
    lens = r.i32([1215, 1100, 900, 640])
    res, c = one(r, lambda: e.plan(s.peaks, s.npeaks, rowband, base, lens, hok, lo16, hop))
    same(r, c, "es_plan_ragged_batch", *head, P(lens), 1215, P(hok), P(lo16), Pk, P(hop), N, C, *outs(res))
    # the absolute arm: pos0 and hop_row come through _dev, ctr0 and hop_base through _ctr_dev; hop_row is then copied to int32
    hop3 = torch.zeros((N, 2, 403), dtype=torch.uint8, device=r.dev)
    pos0, hrow = r.i64([0, 10, 20, 30]), r.i64([0, 1, 1, 0])
    ctr = watch(monkeypatch, e, "_ctr_dev")
    res, c = one(r, lambda: e.plan(s.peaks, s.npeaks, rowband, base, lens, hok, lo16, hop3, pos0=pos0, ctr0=[5, 6, 7, 8], hop_row=hrow, hop_base=[0, 100]))
    assert len(ctr) == 2 and ctr[0].numel() == B and ctr[1].numel() == 2
    same(r, c, "es_plan_at_batch", *head, P(lens), 1215, P(hok), P(lo16), Pk, P(hop3), N, 403, P(pos0), P(ctr[0]), OTHER, P(ctr[1]), 2, *outs(res))
    res, c = one(r, lambda: e.plan(s.peaks, s.npeaks, rowband, base, T, hok, lo16, hop3[:, :1].contiguous(), pos0=pos0))      # T as an int: the method fills the lengths
    assert c[0] == "es_plan_at_batch" and c[7] not in (None, 0, P(lens), P(base)) and c[8] == T and c[15] == P(pos0) and c[19] == 1


def test_validator_and_memo(rig, monkeypatch):
    r, e = rig, rig.eng
    blobs = torch.zeros((B, 55), dtype=torch.uint8, device=r.dev)
    ctr = watch(monkeypatch, e, "_ctr_dev")
    ok, c = one(r, lambda: e.aead_check(KEY, blobs, r.ctrs))
    same(r, c, "es_aead_check_batch", KEY, P(blobs), B, 1, P(ctr[-1]), P(ok), None)
    grouped = torch.zeros((2, L, 55), dtype=torch.uint8, device=r.dev)
    (ok, plain), c = one(r, lambda: e.aead_check(KEY, grouped, r.ctrs[:2], want_plain=True))
    assert ok.shape == (2, L) and plain.shape == (2, L, 27)
    same(r, c, "es_aead_check_batch", KEY, P(grouped), 2 * L, L, P(ctr[-1]), P(ok), P(plain))
    memo = e.open_memo(16)
    k0, k1 = r.i64([1, 2, 3, 4]), r.i64([5, 6, 7, 8])
    _, c = one(r, lambda: e.memo_insert(memo, k0, k1))
    same(r, c, "es_memo_insert_batch", P(memo.table), P(memo.claim), 16, P(k0), P(k1), B)
    hit, c = one(r, lambda: e.memo_probe(memo, k0, k1))
    same(r, c, "es_memo_probe_batch", P(memo.table), 16, P(k0), P(k1), B, P(hit))


def test_seal_and_mix(rig):
    r, e = rig, rig.eng
    nonces = torch.zeros((B, 12), dtype=torch.uint8, device=r.dev)
    plain = torch.zeros((B, 27), dtype=torch.uint8, device=r.dev)
    blobs, c = one(r, lambda: e.aead_seal(KEY, nonces, plain))
    same(r, c, "es_aead_seal_batch", KEY, P(nonces), P(plain), B, P(blobs))
    x = 0.05 * torch.ones((B, T), dtype=torch.float32, device=r.dev)
    tgt, floor = db_to_lin(-10.0), db_to_lin(-35.0)
    out, c = one(r, lambda: e.mix(x, r.f32, block=512))
    same(r, c, "es_mix_batch", P(x), B, T, 512, P(r.f32), T, None, tgt, floor, P(out), None)
    off = r.i64([0, 0, 0, 0])
    (out, scale), c = one(r, lambda: e.mix(x, r.f32, block=512, chip_off=off, want_scale=True, target_rel_db=-12.0))
    same(r, c, "es_mix_batch", P(x), B, T, 512, P(r.f32), T, P(off), db_to_lin(-12.0), floor, P(out), P(scale))
    lens, cbase, ccnt = r.i64([1215, 1000, 512, 1]), r.i64([0, 1215, 2430, 3645]), r.i64([1215] * B)
    out, c = one(r, lambda: e.mix_ragged(x, lens, r.f32, cbase, ccnt, block=512))
    same(r, c, "es_mix_ragged_batch", P(x), B, T, P(lens), 512, P(r.f32), B * T, P(cbase), P(ccnt), tgt, floor, P(out), None)
    (out, scale), c = one(r, lambda: e.mix_ragged(x, lens, r.f32, cbase, ccnt, block=512, want_scale=True, out=x))
    assert out is x
    same(r, c, "es_mix_ragged_batch", P(x), B, T, P(lens), 512, P(r.f32), B * T, P(cbase), P(ccnt), tgt, floor, P(x), P(scale))


def test_embed_chains_its_launches(rig):
    """One 2 048-sample clip through `embed`: five launches, each reading what the one before it wrote."""
    r, e = rig, rig.eng
    x = 0.05 * torch.ones(2048, dtype=torch.float32, device=r.dev)
    res, calls = run(r, lambda: e.embed(KEY, x, seed=7))
    assert [c[0] for c in calls] == ["es_aead_seal_batch", "es_polar_encode_batch", "es_schedule_batch", "es_tx_frames_batch", "es_mix_batch"]
    seal, enc, sched, txf, mix = calls
    st = e._stream()
    assert all(c[1] == e._ctx and c[-1] == st for c in calls)
    assert seal[2] == r.sec._aead._key and seal[5] == 2                     # two frames: ceil(2048 / 1215)
    assert enc[2] == seal[6] and enc[3] == 2                                # the sealed blobs are what is encoded
    assert sched[2:4] == (bytes(r.sec._prng.sub_key), KEY) and sched[4] is not None and sched[6] == 2
    assert txf[2:5] == (enc[4], sched[7], sched[8]) and txf[5] not in (None, sched[4]) and txf[8] == 2      # code, pn, band, the counters
    assert isinstance(txf[6], bytes) and len(txf[6]) == 8 and txf[7] == np.packbits(r.sec.pn_bits(0, 128)).tobytes()
    assert mix[2:6] == (P(x), 1, 2048, 1024) and mix[6] == txf[10] and mix[7] == 2 * 1215 and mix[8] is None
    assert mix[9:11] == (db_to_lin(-10.0), db_to_lin(-35.0)) and mix[11] == P(res.audio) and mix[12] is None


def test_resample_step_one_chunk_of_each_sample_type(rig):
    """Two streams at 44.1 kHz, an int16 and a float32 chunk in one step: one upload, float32 rows first, one launch per sample type."""
    r, e = rig, rig.eng
    rt = e.open_resampler([44_100, 44_100], 48_000)
    rng = np.random.default_rng(3)
    chunks = [(3000 * rng.standard_normal(700)).astype(np.int16), rng.standard_normal(1215).astype(np.float32)]
    out = torch.zeros((2, 1400), dtype=torch.float32, device=r.dev)
    (rows, counts), calls = run(r, lambda: e.resample_step(rt, [0, 1], chunks, out=out))
    assert [c[0] for c in calls] == ["es_resample_stream_batch"] * 2 and rows.shape == (2, 1400)
    f, h = calls
    stride, nfilt = 1216, int(rt.filters.size)
    table = (2, P(rt.rate), P(rt.filt), nfilt, P(rt.tail), P(rt.nin))
    #     ctx x dtype R n_stride sid len rec_host S rate filt nfilt tail nin out out_stride stream
    same(r, f, "es_resample_stream_batch", OTHER, nat.ES_DTYPE_F32, 1, stride, OTHER, OTHER, OTHER, *table, P(out), 1400)
    same(r, h, "es_resample_stream_batch", f[2] + 4 * stride, nat.ES_DTYPE_I16, 1, stride, f[6] + 8, f[7] + 8, OTHER, *table, P(out) + 4 * 1400, 1400)
    assert f[7] - f[6] == 16                                                # ids and lengths: the two rows of one [2, R] int64 tensor


def test_monitor_step_two_streams(rig):
    """A monitor of two streams at the engine's rate, a float32 and an int16 chunk: two band-pass launches, the lags, the peaks."""
    r, e = rig, rig.eng
    t = e.open_monitor(2, window=2432, chunk_max=1300)
    rng = np.random.default_rng(4)
    chunks = [rng.standard_normal(1215).astype(np.float32), (3000 * rng.standard_normal(900)).astype(np.int16)]
    tick, calls = run(r, lambda: e.monitor_step(t, [0, 1], chunks))
    assert [c[0] for c in calls] == ["es_bpf_stream_batch", "es_bpf_stream_batch", "es_xcorr_stream_batch", "es_pick_at_batch"]
    a, b, xc, pk = calls
    S, H, stride = 2, t.hist, 1216
    state = (S, H, P(t.band), P(t.z), P(t.pos), P(t.y_hist), P(t.corr_hist))
    #     ctx x dtype R n_stride sid len col move base rec_host S H band z pos y_hist corr_hist stream
    same(r, a, "es_bpf_stream_batch", OTHER, nat.ES_DTYPE_F32, 1, stride, OTHER, OTHER, OTHER, OTHER, OTHER, OTHER, *state)
    cols = [a[6 + w] + 8 for w in range(5)]
    same(r, b, "es_bpf_stream_batch", a[2] + 4 * stride, nat.ES_DTYPE_I16, 1, stride, *cols, a[11] + 5 * 8, *state)
    assert [a[7 + w] - a[6 + w] for w in range(4)] == [16] * 4             # the rows of one [6, R] int64 tensor
    same(r, xc, "es_xcorr_stream_batch", P(t.y_hist), 2, stride, a[6], a[7], a[8], a[11], S, H, P(t.band), P(t.corr_hist))
    same(r, pk, "es_pick_at_batch", P(t.corr_hist), 4 * S, H, 8, OTHER, OTHER, OTHER, P(tick.thr), P(tick.peaks), P(tick.npeaks))
    assert pk[7] - pk[6] == pk[8] - pk[7] == 4 * 8                          # rows, offsets, lengths: one [3, 4 R] int32 tensor
