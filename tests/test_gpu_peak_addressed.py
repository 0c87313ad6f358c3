"""Demodulation and header decode at detected peaks, in place (es_llr_at_batch, es_header_at_batch, es_front_peak_batch).

Record i of a peak-addressed call reads row r = rows[i] of y from s = max(start[i * stride], 0); its outputs must equal, bit for
bit, those of es_llr_batch / es_header_batch on the torch-gathered row y[r] with start s, and a row outside [0, n_rows) must
give the output of a start at T (an empty frame).  Checked at 48 000 Hz (160-tap build) and 44 100 Hz (576-tap build), both
variants, with repeated rows, every start class, start strides 1 and 32, and launches of several times the grid cap.  Then the
callers: es_front_peak_batch against bpf2 -> sync_fused -> clamp -> llr and against the CPU oracle, DecodePipeline(start="peak")
in every arrangement and decode_batch(start="peak") against the lanes path, and the detector's in-place header and LLR values
against the same calls on gathered frames."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.crypto import SecureChannel
from echoseal_amd.tables import pack_tables

HERE = os.path.dirname(os.path.abspath(__file__))
KEY = b"\xAA" * 32
T = 2048
FL = 1215


def _bits(t):
    """Bit pattern of a float tensor (so that -0.0 / NaN compare as what they are)."""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = (_bits(a) != _bits(b))
    if bad.dim() > 1:
        bad = bad.flatten(1).any(dim=1)
    n = int(bad.sum().item())
    assert n == 0, f"{what}: {n} records differ, first {torch.nonzero(bad).flatten()[:8].tolist()}"


@pytest.fixture(scope="module")
def windows():
    """Config-3 windows (workloads.c3_windows_device) with their schedule, made once on a front-end engine."""
    from echoseal_amd import workloads as WL
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    n = 4096
    pn, band = eng.schedule(SecureChannel(KEY)._prng.sub_key, KEY, ctr0=0, n=n)
    clean = eng.synthetic_frames(KEY, 0, n)[0]
    win, _ = WL.c3_windows_device(clean, seed=36)
    torch.cuda.synchronize()
    eng.close()
    return win, band, pn


def _engine(fs):
    from echoseal_amd.engine import RxEngine
    return RxEngine(0, fs=fs, list_size_max=0)


def _addressing(eng, y, band, pn, B, seed):
    """B records over the rows of y: repeated rows, out-of-range rows, and starts at 0, at T-1215, past it (short frame), at and
    past T, negative, and at the first detected peak.  -> rows, start (int32), band_i, pn_i, and the gathered reference inputs."""
    R = y.shape[0]
    dev = eng.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = torch.randint(-3, R + 3, (B,), generator=g, dtype=torch.int32)
    rows[:64] = 5                                                              # one row many times
    peaks0 = eng.sync_fused(y, y.float(), band)[1][:, 0].cpu()
    cls = torch.randint(0, 8, (B,), generator=g)
    short = torch.randint(1, 1100, (B,), generator=g, dtype=torch.int32)
    pk = peaks0[rows.clamp(0, R - 1).long()]
    start = torch.stack([torch.zeros(B, dtype=torch.int32), torch.full((B,), T - FL, dtype=torch.int32), T - FL + short,
                         torch.full((B,), T, dtype=torch.int32), T + short, -short, pk, torch.full((B,), -1, dtype=torch.int32)])
    start = start.gather(0, cls[None, :])[0].contiguous()
    inr = (rows >= 0) & (rows < R)
    assert inr.any() and (~inr).any() and (rows[inr] == 5).sum() >= 64
    gi = torch.where(inr, rows, torch.zeros_like(rows)).long()
    s_ref = torch.where(inr, start.clamp(min=0), torch.full_like(start, T)).to(torch.int32)
    bi = torch.randint(0, 4, (B,), generator=g, dtype=torch.uint8)
    pni = pn[torch.randint(0, pn.shape[0], (B,), generator=g).to(dev)].contiguous()
    return (rows.to(dev), start.to(dev), bi.to(dev), pni, y[gi.to(dev)].contiguous(), s_ref.to(dev))


def _as_peaks(start):
    """start [B] as column 0 of a [B, 32] peaks table whose other columns hold garbage (stride 32)."""
    p = torch.randint(-5, 5000, (start.numel(), 32), dtype=torch.int32, device=start.device)
    p[:, 0] = start
    return p.contiguous()


@pytest.mark.parametrize("fs", [48_000, 44_100])
def test_llr_at_equals_llr_on_gathered_rows(windows, fs):
    win, band, pn = windows
    eng = _engine(fs)
    y = eng.bpf(win[:1024].contiguous(), band[:1024].contiguous())
    cap = torch.cuda.get_device_properties(eng.device).multi_processor_count * 64
    B = 3 * cap + 37
    rows, start, bi, pni, yg, s_ref = _addressing(eng, y, band[:1024].contiguous(), pn, B, seed=fs)
    for variant in (0, 1):
        want = eng.llr(yg, bi, pni, start=s_ref, variant=variant, want_diag=True)
        for how in ("stride1", "stride32"):
            kw = dict(start=start) if how == "stride1" else dict(start="peak", peaks=_as_peaks(start))
            got = eng.llr(y, bi, pni, rows=rows, variant=variant, want_diag=True, **kw)
            for name, a, b in zip(("llr", "best_s", "score"), want, got):
                _eq(b, a, f"fs={fs} variant={variant} {how} {name}")
    # empty frames really are empty: zeros, shift 0, scores -1
    out = eng.llr(y, bi, pni, rows=torch.full((8,), -1, dtype=torch.int32, device=eng.device), start=start[:8], want_diag=True)
    assert not out[0].any() and not out[1].any() and bool((out[2] == -1.0).all())
    eng.close()


@pytest.mark.parametrize("fs", [48_000, 44_100])
def test_header_at_equals_header_on_gathered_rows(windows, fs):
    win, band, pn = windows
    eng = _engine(fs)
    y = eng.bpf(win[:1024].contiguous(), band[:1024].contiguous())
    cap = torch.cuda.get_device_properties(eng.device).multi_processor_count * 32
    B = 3 * cap + 37
    rows, start, bi, _pni, yg, s_ref = _addressing(eng, y, band[:1024].contiguous(), pn, B, seed=fs + 1)
    hp = torch.from_numpy(np.packbits(SecureChannel(KEY).pn_bits(0, 128)).reshape(1, 16)).to(eng.device)
    for hdr in (hp, hp.expand(B, 16).contiguous() ^ torch.randint(0, 2, (B, 16), dtype=torch.uint8, device=eng.device)):
        want = eng.header(yg, bi, hdr, start=s_ref, want_diag=True)
        for how in ("stride1", "stride32"):
            kw = dict(start=start) if how == "stride1" else dict(start="peak", peaks=_as_peaks(start))
            got = eng.header(y, bi, hdr, rows=rows, want_diag=True, **kw)
            for name, a, b in zip(("ok", "val", "score", "best_s"), want, got):
                _eq(b, a, f"fs={fs} hdr rows={hdr.shape[0]} {how} {name}")
    eng.close()


def test_argument_errors_launch_nothing():
    import echoseal_amd._native as nat
    eng = _engine(48_000)
    lib, ctx, dev = eng._lib, eng._ctx, eng.device
    y = torch.zeros((2, T), dtype=torch.float64, device=dev)
    b8 = torch.zeros(4, dtype=torch.uint8, device=dev)
    pn = torch.zeros((4, 152), dtype=torch.uint8, device=dev)
    llr = torch.full((4, 1024), 7.0, device=dev)
    ok = torch.zeros(4, dtype=torch.uint8, device=dev); val = torch.zeros(4, dtype=torch.int32, device=dev)
    sc = torch.zeros(4, device=dev)
    p = lambda t: None if t is None else t.data_ptr()                     # noqa: E731
    E = -1
    bad_llr = [(2, 4, 0, p(llr)), (0, 4, 1, p(llr)), (2, -1, 1, p(llr)), (2, 4, 1, None), (-1, 4, 1, p(llr))]
    for n_rows, B, stride, out in bad_llr:
        assert lib.es_llr_at_batch(ctx, p(y), n_rows, T, B, None, None, stride, p(b8), p(pn), 0, out, None, None, None) == E
    assert lib.es_llr_at_batch(ctx, p(y), 2, T, 4, None, None, 1, p(b8), p(pn), 2, p(llr), None, None, None) == E   # variant
    for n_rows, B, stride, out in [(2, 4, 0, p(ok)), (0, 4, 1, p(ok)), (2, -1, 1, p(ok)), (2, 4, 1, None)]:
        assert lib.es_header_at_batch(ctx, p(y), n_rows, T, B, None, None, stride, p(b8), p(pn), out, p(val), p(sc), None, None) == E
    Tl = 62 + 4097                                                         # one lag too many (buffers sized for it all the same)
    fr = torch.zeros((4, Tl), device=dev); yl = torch.zeros((4, Tl), dtype=torch.float64, device=dev)
    thr = torch.zeros(4, dtype=torch.float64, device=dev); pk = torch.zeros((4, 32), dtype=torch.int32, device=dev)
    full = (p(yl), p(fr), p(thr), p(pk), p(val), p(ok), p(llr))
    assert lib.es_front_peak_batch(ctx, p(fr), 0, 4, T, p(b8), p(pn), p(yl), None, None, None, None, None, p(llr), None) == E
    assert lib.es_front_peak_batch(ctx, p(fr), 0, 4, Tl, p(b8), p(pn), *full, None) == E
    assert lib.es_front_peak_batch(ctx, p(fr), 0, -1, T, p(b8), p(pn), *full, None) == E
    assert lib.es_front_peak_batch(ctx, p(fr), 7, 4, T, p(b8), p(pn), *full, None) == E                # dtype
    torch.cuda.synchronize()
    assert bool((llr == 7.0).all()) and not yl.any()                       # nothing ran
    with pytest.raises(nat.NativeError):
        eng.llr(y, b8, pn, rows=torch.zeros(4, dtype=torch.int32, device=dev), start=torch.zeros(4, dtype=torch.int32, device=dev),
                variant=3)
    with pytest.raises(ValueError):
        eng.llr(y, b8, pn, start="first")
    with pytest.raises(ValueError):
        eng.llr(y, b8, pn, start="peak")                                  # no peaks=
    eng.close()


def test_front_peak_equals_the_composed_calls_on_headline_windows():
    """es_front_peak_batch on 65 536 headline windows (bench.py's construction, seed 34) = bpf2 -> sync_fused -> clamp -> llr."""
    from echoseal_amd import workloads as WL
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    n = 65536
    pn, band = eng.schedule(SecureChannel(KEY)._prng.sub_key, KEY, ctr0=0, n=n)
    clean = torch.cat([eng.synthetic_frames(KEY, c0, 16384)[0] for c0 in range(0, n, 16384)])
    win, _ = WL.c3_windows_device(clean, seed=34)
    del clean
    y, thr, peaks, npeaks, flags, llr = eng.front(win, band, pn, start="peak")
    y2, y32 = eng.bpf2(win, band)
    thr2, peaks2, npeaks2, flags2 = eng.sync_fused(y2, y32, band)
    llr2 = eng.llr(y2, band, pn, start=peaks2[:, 0].clamp(min=0).contiguous())
    for name, a, b in (("y", y, y2), ("thr", thr, thr2), ("peaks", peaks, peaks2), ("npeaks", npeaks, npeaks2), ("flags", flags, flags2),
                       ("llr", llr, llr2)):
        assert torch.equal(a, b) if a.dtype != torch.float32 else torch.equal(_bits(a), _bits(b)), name
    eng.close()


def test_front_peak_vs_oracle_on_c3_fixture(oracle):
    g = np.load(os.path.join(HERE, "golden", "c3_windows.npz"))
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0)
    sec = SecureChannel(KEY)
    P = sec.pn_bytes_batch([int(c) for c in g["ctr"]], 152)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)   # noqa: E731
    _y, thr, peaks, npeaks, _f, llr = eng.front(d(g["win"]), d(g["band"]), d(P), start="peak")
    thr, peaks, npeaks, llr = thr.cpu().numpy(), peaks.cpu().numpy(), npeaks.cpu().numpy(), llr.cpu().numpy()
    ba, tpl, taps, ntaps, _ = pack_tables()
    for i in range(g["win"].shape[0]):
        b = int(g["band"][i])
        o = oracle.headline_record(g["win"][i], ba[b], tpl[b], taps[b, :ntaps[b]], np.unpackbits(P[i])[:1215], L=8)
        k = min(int(o["npeaks"]), 32)
        assert (int(npeaks[i]) & 0xFFFF) == k and list(peaks[i, :k]) == list(o["peaks"][:k]), i
        assert thr[i] == np.float64(o["thr"]), i
        assert np.array_equal(llr[i].view(np.int32), np.asarray(o["llr"], np.float32).view(np.int32)), i
    eng.close()


def _scl_fields(s):
    return {k: getattr(s, k) for k in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok")}


def test_pipelines_and_decode_batch_at_peak(windows):
    """start="peak" in the lanes, grouped and front/back arrangements and in decode_batch: the llr and list-decoder results of the
    lanes path (which used to gather the first peaks with a torch kernel between sync and the demodulator)."""
    from echoseal_amd.engine import DecodePipeline, RxEngine
    win, band, pn = windows
    eng = RxEngine(0, list_size_max=8)
    batches = [(win[k:k + 1024].contiguous(), band[k:k + 1024].contiguous(), pn[k:k + 1024].contiguous()) for k in (0, 1024)]
    ref_pipe = DecodePipeline(eng, list_size=8, lanes=2)
    refs = [ref_pipe.submit(f, b, p, start="peak") for f, b, p in batches]
    ref_pipe.synchronize()
    # the reference: the first peak gathered on the host side of the library (the composed calls)
    for (f, b, p), (sy, llr, scl, _d) in zip(batches, refs):
        y2, y32 = eng.bpf2(f, b)
        pk = eng.sync_fused(y2, y32, b)[1]
        _eq(llr, eng.llr(y2, b, p, start=pk[:, 0].clamp(min=0).contiguous()), "lanes llr vs composed")
    arrangements = {"grouped": dict(group=2, lanes=2), "front/back": dict()}
    for name, kw in arrangements.items():
        pipe = DecodePipeline(eng, list_size=8, **kw)
        outs = [pipe.submit(f, b, p, start="peak") for f, b, p in batches]
        pipe.synchronize()
        for k, ((sy, llr, scl, _d), (rsy, rllr, rscl, _r)) in enumerate(zip(outs, refs)):
            _eq(sy.peaks, rsy.peaks, f"{name} peaks {k}")
            _eq(llr, rllr, f"{name} llr {k}")
            got = scl.result() if name == "grouped" else scl
            for f_, t in _scl_fields(got).items():
                _eq(t, getattr(rscl, f_), f"{name} {f_} {k}")
        del pipe
    for k, ((f, b, p), (rsy, rllr, rscl, _r)) in enumerate(zip(batches, refs)):
        sy, llr, scl = eng.decode_batch(f, b, p, start="peak", list_size=8)
        torch.cuda.synchronize()
        _eq(llr, rllr, f"decode_batch llr {k}")
        for f_, t in _scl_fields(scl).items():
            _eq(t, getattr(rscl, f_), f"decode_batch {f_} {k}")
    del ref_pipe
    eng.close()


def test_detector_in_place_headers_and_llrs_equal_gathered_frames(engine):
    """verify3s.npz: for every peak of every band of the scan, the header decoded in place (es_header_at_batch) and the LLRs
    demodulated in place (es_llr_at_batch, both variants) equal the same calls on the [P, 1215] gathered frames."""
    from echoseal_amd.detector import FRAME_LEN, WatermarkDetector
    g = np.load(os.path.join(HERE, "golden", "verify3s.npz"))
    det = WatermarkDetector(KEY, list_size=2, engine=engine)
    order = det._band_order()
    scan = det._scan_prepare([g["clip"].astype(np.float32)], order)[0]
    src = scan.src
    P = src.rows.size
    assert P > 20
    dev = engine.device
    rt = torch.from_numpy(src.rows).to(dev)
    cols = torch.from_numpy(src.starts).to(dev)[:, None] + torch.arange(FRAME_LEN, device=dev)[None, :]
    frames = src.y[rt[:, None], cols].contiguous()
    bid = torch.tensor([det._band_id(order[int(r) % len(order)]) for r in src.rows], dtype=torch.uint8, device=dev)
    hp = torch.from_numpy(np.packbits(det.sec.pn_bits(0, 128)).reshape(1, 16)).to(dev)
    ok, val, score = engine.header(frames, bid, hp)
    assert np.array_equal(ok.cpu().numpy().astype(bool), scan.hdr[0])
    assert np.array_equal(val.cpu().numpy().astype(np.int64), scan.hdr[1])
    assert np.array_equal(score.cpu().numpy().astype(np.float64), scan.hdr[2])
    ctrs = [int(round(s / FRAME_LEN)) for s in src.starts]
    pn, bands = engine.schedule(det.sec._prng.sub_key, det._band_key, ctrs=torch.tensor(ctrs, dtype=torch.int64))
    at = dict(rows=torch.from_numpy(src.rows.astype(np.int32)).to(dev), start=torch.from_numpy(src.starts.astype(np.int32)).to(dev))
    for variant in (0, 1):
        _eq(engine.llr(src.y, bands, pn, variant=variant, **at), engine.llr(frames, bands, pn, variant=variant), f"variant {variant}")
