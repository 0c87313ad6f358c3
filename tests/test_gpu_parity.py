"""GPU parity: every HIP kernel, called through the C ABI (echoseal_amd.engine -> ctypes ->
libechoseal_hip.so), against the C oracle on the same seeded inputs, against the golden vectors
captured from the reference, and -- at BASELINE sizes -- through size-independent properties.

Bars: sync offsets, thresholds, LLRs, decoded bits, path metrics are compared BIT-EXACT with the
oracle (both implement the same fixed-order arithmetic); against the reference's golden vectors
sync offsets / decoded bits are exact and LLRs are within 1e-5 (BASELINE.json north_star)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.embedder import WatermarkEmbedder, synthetic_payloads
from echoseal_amd.tables import pack_tables
from echoseal_amd.utils import band_index

KEY = b"\xAA" * 32


def _workload(B, noise=0.0, seed=3, ctr0=0):
    tx = WatermarkEmbedder(KEY)
    ctrs = list(range(ctr0, ctr0 + B))
    frames = tx.make_frames(ctrs, synthetic_payloads(tx.sec, ctrs))
    if noise:
        frames = (frames + np.random.default_rng(seed).normal(0, noise, frames.shape)).astype(np.float32)
    band = np.array([band_index(KEY, c) for c in ctrs], np.uint8)
    pn = tx.sec.pn_bytes_batch(ctrs, 152)
    return frames, band, pn


def _dev(eng, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in arrs]


def test_native_library_is_loaded(engine):
    import echoseal_amd._native as nat
    assert nat.load().es_abi_version() == nat.ES_ABI_VERSION == 2


def test_pipeline_bit_exact_vs_oracle(engine, oracle):
    B = 96
    frames, band, pn = _workload(B)
    frames[B // 2:] = (frames[B // 2:] + np.random.default_rng(5).normal(0, 0.2, frames[B // 2:].shape)).astype(np.float32)
    ba, tpl, taps, ntaps, _ = pack_tables()
    f, b, p = _dev(engine, frames, band, pn)
    sy, llr, _ = engine.decode_batch(f, b, p, list_size=8, keep_corr=True)
    res = engine.scl(llr, list_size=8, skip_if_hard_ok=False)
    y = sy.y.cpu().numpy(); corr = sy.corr.cpu().numpy(); thr = sy.thr.cpu().numpy()
    pk = sy.peaks.cpu().numpy(); npk = sy.npeaks.cpu().numpy(); L = llr.cpu().numpy()
    for i in range(B):
        bi = band[i]
        o = oracle.decode_frame(frames[i], ba[bi], tpl[bi], taps[bi, :ntaps[bi]], np.unpackbits(pn[i])[:1215], L=8)
        assert np.array_equal(o["y"], y[i]) and np.array_equal(o["corr"], corr[i]) and o["thr"] == thr[i]
        n = int(npk[i]) & 0xFFFF
        assert n == min(o["npeaks"], 32) and bool(npk[i] >> 30) == o["fallback"]
        assert list(o["peaks"][:n]) == list(pk[i, :n])
        assert np.array_equal(o["llr"], L[i])
        hinfo, hok = oracle.polar_hard(L[i].astype(np.float64))
        assert np.packbits(hinfo).tobytes() == res.hard_info[i].cpu().numpy().tobytes() and hok == bool(res.hard_ok[i])
        nn, ci, cm, cc = oracle.scl_list(L[i].astype(np.float64), 8)
        assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy())
        assert np.array_equal(cm, res.cand_metric[i].cpu().numpy())
        assert np.array_equal(cc, res.cand_ok[i].cpu().numpy())


@pytest.mark.parametrize("L", [1, 2, 4, 8, 16, 32])
def test_scl_all_list_sizes_vs_oracle(engine, oracle, L):
    rng = np.random.default_rng(100 + L)
    llr = np.clip(rng.normal(0, 3, (12, 1024)), -12, 12)
    llr[0] = 0.0; llr[0, 0] = 1e-3                                       # every candidate ties
    llr[1] = np.where(rng.integers(0, 2, 1024) == 1, 12.0, -12.0)        # saturated, many exact ties
    llr[2] = rng.normal(0, 3000, 1024)                                   # exp underflow / subnormals
    for dt in (np.float64, np.float32):
        x = llr.astype(dt)
        res = engine.scl(torch.from_numpy(x).to(engine.device), list_size=L, skip_if_hard_ok=False)
        for i in range(x.shape[0]):
            nn, ci, cm, cc = oracle.scl_list(x[i].astype(np.float64), L)
            assert int(res.ncand[i]) == nn == L
            assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy()), (L, i)
            assert np.array_equal(cm, res.cand_metric[i].cpu().numpy()), (L, i)
            assert np.array_equal(cc, res.cand_ok[i].cpu().numpy()), (L, i)


def test_scl_matches_reference_golden(engine, golden_polar):
    from echoseal_amd.engine import select_payload
    mode, g = golden_polar
    names = sorted({k.split("/")[0] for k in g.files if k.endswith("/llr")})
    for L in (1, 4, 8, 16, 32):
        llrs = [g[f"{n}/llr"] for n in names]
        for dt in (np.float32, np.float64):
            idx = [i for i, v in enumerate(llrs) if v.dtype == dt]
            if not idx:
                continue
            x = torch.from_numpy(np.stack([llrs[i] for i in idx])).to(engine.device)
            res = engine.scl(x, list_size=L, skip_if_hard_ok=True)
            for row, i in enumerate(idx):
                payload, ok = select_payload(res, row, None)
                assert ok == bool(g[f"{names[i]}/L{L}/ok"]), (names[i], L)
                assert payload == g[f"{names[i]}/L{L}/info"].tobytes(), (names[i], L)      # decoded bits: exact
                key = f"{names[i]}/L{L}/cand_metric"
                if key in g.files:
                    assert int(res.ncand[row]) == L
                    assert np.array_equal(res.cand_info[row].cpu().numpy(), g[f"{names[i]}/L{L}/cand_info"])
                    m = res.cand_metric[row].cpu().numpy()
                    if mode == "glibc":
                        assert np.array_equal(m, g[key])
                    else:
                        assert np.allclose(m, g[key], rtol=1e-13, atol=0)
                else:
                    assert int(res.ncand[row]) == 0


def test_sync_and_llr_match_reference_golden(engine, golden_detector):
    g = golden_detector
    n = int(g["det/count"])
    tags = [f"det/{i:02d}" for i in range(n)]
    x = np.stack([g[f"{t}/x"] for t in tags]); band = np.array([int(g[f"{t}/band"]) for t in tags], np.uint8)
    pn = np.zeros((n, 152), np.uint8); pn[:, :] = np.stack([g[f"{t}/pn"] for t in tags])
    f, b, p = _dev(engine, x, band, pn)
    sy = engine.sync(f, b)
    llr0, bs0, _ = engine.llr(sy.y, b, p, variant=0, want_diag=True)
    llr1, bs1, _ = engine.llr(sy.y, b, p, variant=1, want_diag=True)
    y = sy.y.cpu().numpy(); corr = sy.corr.cpu().numpy(); thr = sy.thr.cpu().numpy()
    pk = sy.peaks.cpu().numpy(); npk = sy.npeaks.cpu().numpy()
    worst = 0.0
    for i, t in enumerate(tags):
        assert np.array_equal(y[i], g[f"{t}/y"])                                  # IIR: bit exact
        assert np.max(np.abs(corr[i] - g[f"{t}/corr"])) < 1e-12
        assert abs(thr[i] - float(g[f"{t}/thr"])) < 1e-12
        k = int(npk[i]) & 0xFFFF
        assert list(pk[i, :k]) == list(g[f"{t}/peaks"]) and bool(npk[i] >> 30) == bool(g[f"{t}/fallback"])
        assert int(bs0[i]) == int(g[f"{t}/best_s"][0]) and int(bs1[i]) == int(g[f"{t}/best_s"][1])
        worst = max(worst, float(np.max(np.abs(llr0[i].cpu().numpy() - g[f"{t}/llr0"]))),
                    float(np.max(np.abs(llr1[i].cpu().numpy() - g[f"{t}/llr1"]))))
    assert worst <= 1e-5, worst
    # short records: frame = y[:700] -> zero padded LLR (rtwm/detector.py:410-414)
    ys = sy.y[:, :700].contiguous()
    ls, bss, _ = engine.llr(ys, b, p, variant=0, want_diag=True)
    for i, t in enumerate(tags):
        assert int(bss[i]) == int(g[f"{t}/best_s"][2])
        assert np.max(np.abs(ls[i].cpu().numpy() - g[f"{t}/llr_short700"])) <= 1e-5


def test_bandpass_bits_all_kernels(engine, oracle):
    """The three band-pass kernels (sixteen lanes per record for small batches, four lanes per record, one lane per record for huge
    batches) against the oracle's lfilter BIT FOR BIT (uint64 view: signed zeros count): random, silence, negative zeros, sparse
    impulses (delay elements pass through +-0), denormals, a long record."""
    ba, tpl, taps, ntaps, _ = pack_tables()
    rng = np.random.default_rng(77)

    def rows(n, T):
        x = rng.normal(0, 0.2, (n, T)).astype(np.float32)
        x[1 % n] = 0.0
        x[2 % n] = -0.0
        x[3 % n] = 0.0; x[3 % n, ::37] = rng.choice(np.array([-1.0, 1.0, 0.5], np.float32), x[3 % n, ::37].shape)
        x[4 % n] = np.where(rng.random(T) < 0.5, np.float32(0.0), np.float32(-0.0)); x[4 % n, T // 2] = 1e-3
        x[5 % n] = (rng.normal(0, 1, T) * 1e-42).astype(np.float32)            # float32 denormals
        return x

    def check(x, band, idx):
        f, b = _dev(engine, x, band)
        y = engine.bpf(f, b).cpu().numpy()
        y2, y32 = engine.bpf2(f, b)
        assert np.array_equal(y2.cpu().numpy().view(np.uint64), y.view(np.uint64))
        assert np.array_equal(y32.cpu().numpy().view(np.uint32), y.astype(np.float32).view(np.uint32))
        for i in idx:
            ref = oracle.lfilter(ba[band[i], :9], ba[band[i], 9:], x[i])
            assert np.array_equal(ref.view(np.uint64), y[i].view(np.uint64)), (x.shape, i)

    for n, T in ((7, 100), (6, 1215), (3, 20011)):                       # sixteen lanes per record
        check(rows(n, T), (np.arange(n) % 4).astype(np.uint8), range(n))
    x = rows(5003, 300)                                                   # four lanes per record
    check(x, (np.arange(5003) % 4).astype(np.uint8), list(range(8)) + [63, 64, 4097, 5002])
    x = rows(8, 64)                                                       # one lane per record (>= 262 144 records)
    big = np.tile(x, (32768 + 1, 1))[:262144 + 5]
    check(big, (np.arange(big.shape[0]) % 4).astype(np.uint8), list(range(8)) + [262143, 262148])


def test_pick_threshold_saturation_shortcut(engine, oracle):
    """es_pick_batch proves `thr == 0.95` from one histogram pass where it can and takes the exact order statistics where it cannot:
    rows on both sides of the saturation boundary (4.5 sigma ~ 0.95 for Gaussian rows), shifted medians, values at +-1, an even and an odd
    length, a 240 000-lag row (one band of a 5 s recording), a row with a NaN -- threshold, peak list and fallback flag equal the oracle's."""
    rng = np.random.default_rng(2024)
    rows = []
    for n in (4096, 4097):
        for sigma in (0.05, 0.15, 0.19, 0.205, 0.2105, 0.2115, 0.215, 0.23, 0.3, 0.6):
            rows.append(np.clip(rng.normal(0.0, sigma, n), -1.0, 1.0))
        rows.append(np.clip(rng.normal(0.3, 0.25, n), -1.0, 1.0))
        rows.append(np.clip(rng.normal(-0.4, 0.3, n), -1.0, 1.0))
        r = np.clip(rng.normal(0.0, 0.25, n), -1.0, 1.0); r[::50] = 1.0; r[7::90] = -1.0
        rows.append(r)
        rows.append(np.where(rng.random(n) < 0.5, -0.5, 0.5) + rng.normal(0, 1e-3, n))        # bimodal: MAD 0.5
    saturated = exact = 0
    for r in rows + [np.clip(rng.normal(0.0, 0.25, 240000), -1.0, 1.0), np.clip(rng.normal(0.0, 0.12, 240000), -1.0, 1.0)]:
        c = torch.from_numpy(np.ascontiguousarray(r).reshape(1, -1)).to(engine.device)
        thr, peaks, npeaks = engine.pick(c)
        t_ref, med, mad = oracle.cfar_threshold(r)
        assert float(thr[0]) == t_ref, (r.size, float(thr[0]), t_ref)
        saturated += t_ref == 0.95; exact += t_ref < 0.95
        pk, tot, fb = oracle.pick_peaks(r, t_ref)
        k = int(npeaks[0]) & 0xFFFF                              # the count is not capped at the 32 peaks that are stored
        assert k == tot and bool(int(npeaks[0]) >> 30) == fb, (r.size, k, tot)
        assert list(peaks[0, :min(k, 32)].cpu().numpy()) == list(pk[:min(k, 32)])
    assert saturated >= 12 and exact >= 12, (saturated, exact)
    r = np.clip(rng.normal(0.0, 0.3, 5000), -1.0, 1.0); r[123] = np.nan                        # a NaN must not be "proven" anything
    c = torch.from_numpy(r.reshape(1, -1)).to(engine.device)
    thr_nan, _, _ = engine.pick(c)
    engine_exact = float(thr_nan[0])
    assert engine_exact != engine_exact or engine_exact <= 0.95


def test_edge_records(engine, oracle):
    ba, tpl, taps, ntaps, _ = pack_tables()
    rng = np.random.default_rng(8)
    # ragged tail (batch not a multiple of 64), window longer than a frame, silence, constants, int16
    for T in (63, 64, 700, 1215, 2048):
        x = rng.normal(0, 0.1, (5, T)).astype(np.float32)
        x[1] = 0.0
        x[2] = 0.25
        band = np.array([0, 1, 2, 3, 1], np.uint8)
        f, b = _dev(engine, x, band)
        sy = engine.sync(f, b)
        for i in range(5):
            y = oracle.lfilter(ba[band[i], :9], ba[band[i], 9:], x[i])
            assert np.array_equal(y, sy.y[i].cpu().numpy())
            corr = oracle.ncc(y, tpl[band[i]])
            assert np.array_equal(corr, sy.corr[i].cpu().numpy())
            thr, _, _ = oracle.cfar_threshold(corr)
            assert thr == float(sy.thr[i])
            peaks, tot, fb = oracle.pick_peaks(corr, thr)
            if i == 1:
                continue                     # all-zero correlation: every lag ties (declared ambiguous)
            k = int(sy.npeaks[i]) & 0xFFFF
            assert bool(int(sy.npeaks[i]) >> 30) == fb and list(sy.peaks[i, :k].cpu().numpy()) == list(peaks[:k])
    xi = np.clip(np.round(rng.normal(0, 0.2, (3, 1215)) * 32767), -32767, 32767).astype(np.int16)
    band = np.array([3, 0, 2], np.uint8)
    f, b = _dev(engine, xi, band)
    yi = engine.bpf(f, b).cpu().numpy()
    xf = xi.astype(np.float32) / np.float32(32768)         # what soundfile.read returns for PCM16 (rx_app.py:26); exact in float32
    assert np.array_equal(yi, engine.bpf(torch.from_numpy(xf).to(engine.device), b).cpu().numpy())     # int16 ingest == float32 path
    for i in range(3):
        assert np.array_equal(yi[i], oracle.lfilter(ba[band[i], :9], ba[band[i], 9:], xf[i]))
    # frames starting inside a longer window, including one that runs off the end
    frames, bnd, pn = _workload(4)
    win = np.zeros((4, 2048), np.float32); starts = np.array([0, 100, 833, 1500], np.int32)
    for i in range(4):
        seg = frames[i][: 2048 - starts[i]]
        win[i, starts[i]:starts[i] + seg.size] = seg
    f, b, p, s = _dev(engine, win, bnd, pn, starts)
    y = engine.bpf(f, b)
    llr, bs, _ = engine.llr(y, b, p, start=s, want_diag=True)
    for i in range(4):
        yy = y[i].cpu().numpy()
        o, obs, _, _ = oracle.llr(yy[starts[i]:starts[i] + 1215], np.unpackbits(pn[i])[191:1215], taps[bnd[i], :ntaps[bnd[i]]])
        assert obs == int(bs[i]) and np.array_equal(o, llr[i].cpu().numpy())
    # empty batch and argument errors
    e = torch.empty((0, 1024), dtype=torch.float32, device=engine.device)
    assert engine.scl(e, list_size=8).ncand.numel() == 0
    from echoseal_amd._native import NativeError
    with pytest.raises(NativeError):
        engine.scl(torch.zeros((1, 1024), device=engine.device), list_size=0)
    with pytest.raises(NativeError):
        engine.scl(torch.zeros((1, 1024), device=engine.device), list_size=64)       # above this context's list_size_max


def test_polar_encode_kernel(engine, oracle):
    rng = np.random.default_rng(9)
    info = rng.integers(0, 256, (37, 55), dtype=np.uint8)
    code = engine.polar_encode(torch.from_numpy(info).to(engine.device)).cpu().numpy()
    for i in range(37):
        assert np.array_equal(code[i], oracle.polar_encode(np.unpackbits(info[i])))


def test_full_size_properties(engine, oracle):
    """BASELINE config 2 (1 024 clean frames) and a 65 536-record batch: size-independent checks.
    encode -> +-LLR -> decode round trip; sync finds offset 0 on every clean frame; a spot-checked
    subset equals the oracle bit for bit; results do not depend on batch position."""
    B = 1024
    frames, band, pn = _workload(B)
    f, b, p = _dev(engine, frames, band, pn)
    sy, llr, scl = engine.decode_batch(f, b, p, list_size=8)
    npk = sy.npeaks.cpu().numpy(); pk = sy.peaks.cpu().numpy()
    # every clean frame syncs at offset 0 (a few also show a second >0.95 peak further than 607 lags away)
    assert np.all(npk >= 1) and np.all(npk < 4) and np.all(pk[:, 0] == 0) and np.all(sy.thr.cpu().numpy() == 0.95)
    ba, tpl, taps, ntaps, _ = pack_tables()
    L = llr.cpu().numpy()
    for i in range(0, B, 97):
        o = oracle.decode_frame(frames[i], ba[band[i]], tpl[band[i]], taps[band[i], :ntaps[band[i]]],
                                np.unpackbits(pn[i])[:1215], L=8)
        assert np.array_equal(o["llr"], L[i])
        nn, ci, cm, cc = oracle.scl_list(L[i].astype(np.float64), 8)
        if int(scl.ncand[i]):
            assert np.array_equal(np.packbits(ci, axis=1), scl.cand_info[i].cpu().numpy())
            assert np.array_equal(cm, scl.cand_metric[i].cpu().numpy())
    # round trip at scale: random payloads -> GPU encode -> +-4 LLR with 3 % flips -> SCL-8
    rng = np.random.default_rng(77)
    Bb = 65536
    info = torch.from_numpy(rng.integers(0, 256, (Bb, 55), dtype=np.uint8)).to(engine.device)
    code = engine.polar_encode(info)
    soft = (code.to(torch.float32) * 2 - 1) * 4.0
    res = engine.scl(soft, list_size=8, skip_if_hard_ok=True)
    assert bool(torch.all(res.hard_ok == 1)) and bool(torch.all(res.hard_info == info))
    # batch-position independence: the same 64 LLR rows at the start and the end of a big batch
    big = soft.clone()
    noise = torch.from_numpy(rng.normal(0, 5, (64, 1024)).astype(np.float32)).to(engine.device)
    big[:64] = noise; big[-64:] = noise
    r2 = engine.scl(big, list_size=8, skip_if_hard_ok=True)
    assert bool(torch.all(r2.cand_info[:64] == r2.cand_info[-64:])) and bool(torch.all(r2.cand_metric[:64] == r2.cand_metric[-64:]))
    assert bool(torch.all(r2.ncand[:64] == r2.ncand[-64:]))


def test_polarcode_api_on_gpu(golden_polar):
    """Reference-style calls (tests/test_polar.py of the reference) through the drop-in API."""
    from rtwm.polar_fast import decode, encode, N_DEFAULT, K_DEFAULT
    from rtwm.fastpolar import PolarCode
    _, g = golden_polar
    payload = bytes(range(55))
    chips = encode(payload)
    assert decode(np.where(chips == 1, 10.0, -10.0).astype(np.float32)) == payload
    rng = np.random.default_rng(1234)
    pc = PolarCode(N_DEFAULT, K_DEFAULT, list_size=8, crc_size=8)
    info = rng.integers(0, 2, 440, dtype=np.uint8)
    cw = pc.encode(info)
    rx = 2.0 * cw.astype(np.float64) - 1.0 + rng.normal(0.0, 0.15, 1024)
    bits, ok = pc.decode(2.0 * rx / 0.15 ** 2)
    assert ok and np.array_equal(bits, info)
    # validator that rejects everything: reference returns the best CRC-passing (or lowest-metric) path, ok False
    out, ok = decode(g["garbage_rng7/llr"], list_size=8, return_ok=True, validator=lambda b: False)
    assert ok is False and len(out) == 55
    with pytest.raises(ValueError):
        decode(np.zeros(1000))
    with pytest.raises(ValueError):
        encode(b"short")


@pytest.mark.parametrize("L", [64, 128, 256])
def test_scl_wide_lists_vs_oracle(oracle, L):
    """Lists above 32 (the detector's default is 256) run on the workgroup-per-frame kernel."""
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=256)
    rng = np.random.default_rng(500 + L)
    llr = np.clip(rng.normal(0, 3, (6, 1024)), -12, 12)
    llr[0] = 0.0; llr[0, 0] = 1e-3
    llr[1] = np.where(rng.integers(0, 2, 1024) == 1, 12.0, -12.0)
    for dt in (np.float32, np.float64):
        x = llr.astype(dt)
        res = eng.scl(torch.from_numpy(x).to(eng.device), list_size=L, skip_if_hard_ok=False)
        for i in range(x.shape[0]):
            nn, ci, cm, cc = oracle.scl_list(x[i].astype(np.float64), L)
            assert int(res.ncand[i]) == nn == L
            assert np.array_equal(cm, res.cand_metric[i].cpu().numpy()), (L, i)
            assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy()), (L, i)
            assert np.array_equal(cc, res.cand_ok[i].cpu().numpy()), (L, i)
    eng.close()


@pytest.mark.parametrize("K", [9, 13, 16, 24, 40, 64, 200, 301, 440, 456, 512, 1000, 1016, 1023, 1024])
def test_scl_other_codes_vs_oracle(oracle, K):
    """Polar(1024, K) + CRC-8 for K other than 448 (a last trace-back window of any length; one or 32 windows; K - 8 not a whole number of bytes;
    one information bit; no frozen position): lists of every
    capacity against the oracle built for the same K, float32 and float64 LLRs, ragged batch sizes, and the API's PolarCode.decode."""
    from echoseal_amd.engine import RxEngine
    from rtwm.fastpolar import PolarCode
    eng = RxEngine(0, list_size_max=256, code_k=K)
    rng = np.random.default_rng(900 + K)
    pc = PolarCode(1024, K, list_size=8, crc_size=8)
    B = 37
    codes = np.stack([pc.encode(rng.integers(0, 2, K - 8, dtype=np.uint8)) for _ in range(B)]).astype(np.float64)
    llr = np.clip(2.0 * (2.0 * codes - 1.0 + rng.normal(0, 0.9, codes.shape)) / 0.81, -12, 12)
    llr[0] = 0.0
    llr[1] = np.where(codes[1] > 0, 12.0, -12.0)
    llr[2] = np.clip(rng.normal(0, 3, 1024), -12, 12)
    llr[3] = np.where(codes[3] > 0, 1.0, -1.0) * rng.integers(1, 4, 1024)       # small integers: ties
    with oracle.code_k(K):
        for L, dt in ((1, np.float32), (2, np.float64), (8, np.float32), (8, np.float64), (32, np.float32), (50, np.float32), (256, np.float64)):
            x = llr.astype(dt)[: (B if L <= 8 else 9)]
            res = eng.scl(torch.from_numpy(x).to(eng.device), list_size=L, skip_if_hard_ok=False).check()
            short = eng.scl(torch.from_numpy(x).to(eng.device), list_size=L, skip_if_hard_ok=True).check()
            assert res.cand_info.shape[-1] == (K - 8 + 7) // 8
            for i in range(x.shape[0]):
                hinfo, hok = oracle.polar_hard(x[i].astype(np.float64))
                assert np.packbits(hinfo).tobytes() == res.hard_info[i].cpu().numpy().tobytes() and hok == bool(res.hard_ok[i]), (L, i)
                assert (int(short.ncand[i]) == 0) == hok, (L, i)
                nn, ci, cm, cc = oracle.scl_list(x[i].astype(np.float64), L)
                assert int(res.ncand[i]) == nn, (L, i)
                assert np.array_equal(cm[:nn], res.cand_metric[i, :nn].cpu().numpy()), (L, i)
                assert np.array_equal(np.packbits(ci[:nn], axis=1), res.cand_info[i, :nn].cpu().numpy()), (L, i)
                assert np.array_equal(cc[:nn], res.cand_ok[i, :nn].cpu().numpy()), (L, i)
        # the drop-in class (its own engine for this K), against the oracle's PolarCode.decode
        for i in (1, 4, 5):
            bits, ok = pc.decode(llr[i])
            info, ook, _ = oracle.polar_decode(llr[i], 8)
            assert ok == ook and np.array_equal(bits, info), i
    # entry points that only exist for the detector's code say so
    import echoseal_amd._native as nat
    with pytest.raises(nat.NativeError, match="reference's own code"):
        eng.polar_encode(torch.zeros((1, 55), dtype=torch.uint8, device=eng.device))
    eng.close()
    small = RxEngine(0, list_size_max=8, code_k=K)
    with pytest.raises(nat.NativeError, match="lane-per-path kernel only"):
        small.scl(torch.zeros((1, 1024), device=small.device), list_size=8)
    small.close()


@pytest.mark.parametrize("mode", ["default", "glibc"])
def test_scl_wide_matches_reference_golden(mode):
    import os
    from echoseal_amd.engine import RxEngine, select_payload
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"polar_wide_{mode}.npz"))
    eng = RxEngine(0, list_size_max=256)
    names = sorted({k.split("/")[0] for k in g.files if k.endswith("/llr")})
    for L in (64, 256):
        for n in names:
            llr = g[f"{n}/llr"]
            x = torch.from_numpy(np.ascontiguousarray(llr)).to(eng.device).reshape(1, 1024)
            res = eng.scl(x, list_size=L, skip_if_hard_ok=True)
            payload, ok = select_payload(res, 0, None)
            assert ok == bool(g[f"{n}/L{L}/ok"]) and payload == g[f"{n}/L{L}/info"].tobytes(), (n, L)
            key = f"{n}/L{L}/cand_metric"
            if key in g.files:
                assert np.array_equal(res.cand_info[0].cpu().numpy(), g[f"{n}/L{L}/cand_info"])
                m = res.cand_metric[0].cpu().numpy()
                assert np.array_equal(m, g[key]) if mode == "glibc" else np.allclose(m, g[key], rtol=1e-13, atol=0)
    eng.close()


def test_config3_noisy_jittered_windows(engine, oracle):
    """BASELINE config 3 shape: 65 536 records of W = 2048 samples, each holding a frame resampled
    by a factor in [0.95, 1.05] (linear interpolation, seed 3) at a random offset, plus AWGN at
    -15 dB SNR (seed 4).  512 distinct windows are generated and tiled to 65 536 records; checks:
    spot rows equal the oracle bit for bit (sync, LLR at the detected peak, SCL-8), and every copy
    of a window gives identical results wherever it sits in the batch."""
    from scipy.signal import lfilter  # noqa: F401  (scipy present on the GPU box; only numpy is used below)
    U, B, W = 512, 65536, 2048
    frames, band, pn = _workload(U)
    rng3, rng4 = np.random.default_rng(3), np.random.default_rng(4)
    win = np.zeros((U, W), np.float32)
    for i in range(U):
        fac = rng3.uniform(0.95, 1.05)
        m = int(np.floor((1215 - 1) / fac)) + 1
        res = np.interp(np.arange(m) * fac, np.arange(1215), frames[i]).astype(np.float32)
        off = int(rng3.integers(0, W - m + 1))
        win[i, off:off + m] = res
        rms = float(np.sqrt(np.mean(res.astype(np.float64) ** 2)))
        win[i] += rng4.normal(0.0, rms * 10 ** (15 / 20), W).astype(np.float32)
    reps = B // U
    f = torch.from_numpy(win).to(engine.device).repeat(reps, 1)
    b = torch.from_numpy(band).to(engine.device).repeat(reps)
    p = torch.from_numpy(pn).to(engine.device).repeat(reps, 1)
    sy = engine.sync(f, b, keep_corr=False)
    start = sy.peaks[:, 0].clamp(min=0).contiguous()
    llr, bs, _ = engine.llr(sy.y, b, p, start=start, want_diag=True)
    res = engine.scl(llr, list_size=8, skip_if_hard_ok=True)
    # position independence
    for t in (sy.thr, sy.peaks, sy.npeaks, llr, bs, res.cand_info, res.cand_metric, res.ncand, res.hard_info):
        v = t.reshape(reps, U, -1)
        assert bool(torch.all(v == v[0:1])), "result depends on the position in the batch"
    # spot parity with the oracle
    ba, tpl, taps, ntaps, _ = pack_tables()
    y = sy.y[:U].cpu().numpy(); thr = sy.thr[:U].cpu().numpy(); pk = sy.peaks[:U].cpu().numpy(); npk = sy.npeaks[:U].cpu().numpy()
    L = llr[:U].cpu().numpy()
    for i in range(0, U, 37):
        bi = band[i]
        yy = oracle.lfilter(ba[bi, :9], ba[bi, 9:], win[i])
        assert np.array_equal(yy, y[i])
        corr = oracle.ncc(yy, tpl[bi]); th, _, _ = oracle.cfar_threshold(corr)
        peaks, tot, fb = oracle.pick_peaks(corr, th)
        k = int(npk[i]) & 0xFFFF
        assert th == thr[i] and bool(npk[i] >> 30) == fb and list(pk[i, :k]) == list(peaks[:k])
        st = int(peaks[0])
        o, obs, _, _ = oracle.llr(yy[st:st + 1215], np.unpackbits(pn[i])[191:1215], taps[bi, :ntaps[bi]])
        assert np.array_equal(o, L[i])
        hinfo, hok = oracle.polar_hard(o.astype(np.float64))
        assert np.packbits(hinfo).tobytes() == res.hard_info[i].cpu().numpy().tobytes() and hok == bool(res.hard_ok[i])
        assert (int(res.ncand[i]) == 0) == hok, i                        # compaction: no list exactly when the hard decision passes
        if not hok:
            nn, ci, cm, cc = oracle.scl_list(o.astype(np.float64), 8)
            assert int(res.ncand[i]) == nn
            assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy())
            assert np.array_equal(cm.view(np.uint64), res.cand_metric[i].cpu().numpy().view(np.uint64))
            assert np.array_equal(cc, res.cand_ok[i].cpu().numpy())


def _adversarial_records(rng, n, T):
    """Records built to stress the float32 screen: near-threshold peaks, exact repeats, constants,
    periodic signals (many equal correlations), huge / tiny amplitudes, isolated clicks."""
    x = rng.normal(0, 0.1, (n, T)).astype(np.float32)
    x[0] = 0.0
    x[1] = 0.3
    x[2] = np.tile(rng.normal(0, 0.2, 64).astype(np.float32), T // 64 + 1)[:T]          # period 64
    x[3] = np.sin(2 * np.pi * 5000 / 48000 * np.arange(T)).astype(np.float32)           # in-band tone
    x[4] *= 1e-20
    x[5] *= 1e6
    x[6] = 0.0; x[6, T // 2] = 1.0                                                       # click
    x[7, : T // 2] = x[7, T - T // 2:][: T // 2]                                         # repeated half
    x[8] = np.where(np.arange(T) % 2 == 0, 0.5, -0.5).astype(np.float32)                # Nyquist
    x[9] = 0.0; x[9, :63] = 1.0
    x[10] *= 1e25                                                                      # float32 energy overflows
    x[11, 100:200] *= 1e22
    return x


def test_sync_fast_equals_float64_path(engine, oracle):
    """es_xcorr32 + es_pick_exact (float32 screen, float64 fix-ups) must give bit-identical
    thr / peaks / npeaks to the all-float64 kernels, on clean frames, noisy frames and records
    built to break a float32 screen; corr32 stays within the proven error bound."""
    rng = np.random.default_rng(2026)
    frames, band, pn = _workload(192)
    noisy = (frames[:96] + rng.normal(0, 0.15, (96, 1215))).astype(np.float32)
    adv = _adversarial_records(rng, 32, 1215)
    # near-threshold cases: scale the preamble-bearing frame into noise so corr[0] lands around 0.95
    near = np.stack([(frames[i] * a + rng.normal(0, 0.05, 1215)).astype(np.float32)
                     for i, a in zip(range(64), np.linspace(0.28, 0.42, 64))])
    x = np.concatenate([frames, noisy, adv, near])
    bnd = np.concatenate([band, band[:96], rng.integers(0, 4, 32).astype(np.uint8), band[:64]])
    floor = rng.normal(0, 1e-3, (x.shape[0], 2048)).astype(np.float32)
    cases = {
        "frame-sized": x,
        # digital silence around the frame: hundreds of correlations are exactly 0 and tie with the
        # median, so the screen hands the record to the float64 kernels (the fallback is exercised)
        "window, zero padded": np.pad(x, ((0, 0), (300, 2048 - 1215 - 300))),
        # the same window over a -60 dBFS noise floor: no exact ties, the screen settles everything
        "window, noise floor": np.pad(x, ((0, 0), (300, 2048 - 1215 - 300))) + floor,
    }
    for name, xx in cases.items():
        f, b = _dev(engine, xx.astype(np.float32), bnd)
        ref = engine.sync(f, b, keep_corr=True)
        k = (ref.npeaks & 0xFFFF).clamp(max=32)
        for fused in (True, False):                 # one kernel (screen row in LDS) / screen through HBM
            fast = engine.sync_fast(f, b, fused=fused)
            assert torch.equal(ref.y, fast.y) and torch.equal(fast.y.to(torch.float32), fast.y32)
            assert torch.equal(ref.thr, fast.thr), f"{name}: threshold differs"
            assert torch.equal(ref.npeaks, fast.npeaks), f"{name}: peak count / fallback flag differs"
            for i in range(xx.shape[0]):
                assert torch.equal(ref.peaks[i, :k[i]], fast.peaks[i, :k[i]]), (name, i, fused)
        err = (fast.corr32.double() - ref.corr).abs()
        ok_rows = torch.isfinite(fast.corr32).all(dim=1)
        assert float(err[ok_rows].max()) < 1e-5, float(err[ok_rows].max())            # well inside DELTA = 3e-5
        flagged = int((fast.flags != 0).sum())
        if name == "window, zero padded":
            assert flagged >= xx.shape[0] // 2, flagged
        else:                       # only the degenerate adversarial records may need the float64 redo
            assert flagged <= 12, (name, flagged, torch.unique(fast.flags, return_counts=True))
    # and against the CPU oracle directly
    ba, tpl, taps, ntaps, _ = pack_tables()
    f, b = _dev(engine, x, bnd)
    fast = engine.sync_fast(f, b)
    for i in range(0, x.shape[0], 7):
        yy = oracle.lfilter(ba[bnd[i], :9], ba[bnd[i], 9:], x[i])
        corr = oracle.ncc(yy, tpl[bnd[i]]); th, _, _ = oracle.cfar_threshold(corr)
        peaks, tot, fb = oracle.pick_peaks(corr, th)
        if not corr.any():
            continue
        kk = int(fast.npeaks[i]) & 0xFFFF
        assert th == float(fast.thr[i]) and bool(int(fast.npeaks[i]) >> 30) == fb
        assert list(fast.peaks[i, :kk].cpu().numpy()) == list(peaks[:kk])

def test_sync_fast_large_batch_property(engine):
    """65 536 records: fast path == float64 path on every record (thr, npeaks, peaks)."""
    frames, band, pn = _workload(1024)
    rng = np.random.default_rng(11)
    x = (frames + rng.normal(0, 0.2, frames.shape) * (np.arange(1024)[:, None] % 3 == 0)).astype(np.float32)
    f, b = _dev(engine, x, band)
    f = f.repeat(64, 1); b = b.repeat(64)
    ref = engine.sync(f, b, keep_corr=False)
    fast = engine.sync_fast(f, b)
    assert torch.equal(ref.thr, fast.thr) and torch.equal(ref.npeaks, fast.npeaks)
    k = (ref.npeaks & 0xFFFF).clamp(max=32)
    mask = torch.arange(32, device=engine.device)[None, :] < k[:, None]
    assert torch.equal(ref.peaks[mask], fast.peaks[mask])


@pytest.mark.parametrize("mode", ["front+decoders", "lanes", "lanes, several frames per wave", "grouped", "grouped, one lane per path"])
def test_decode_pipeline_equals_decode_batch(engine, mode):
    """The streaming pipeline returns, for every batch, exactly what decode_batch returns for it -- including when
    different batches are in flight: the round-1 arrangement (front-end stream + two list-decoder streams), the whole-chain
    lanes, those with the multi-frame list decoder forced (its launches share nothing but the GPU), and the grouped arrangement
    that bench.py runs (groups of three batches share one list-decoder launch: two full groups and an incomplete one; with the
    kernel the library picks for so few frames, and with the one-lane-per-path kernel the full-size groups get)."""
    from echoseal_amd.engine import DecodePipeline, GroupTicket
    if mode.startswith("grouped"):
        pipe = DecodePipeline(engine, list_size=8, lanes=2, scl_streams=2, group=3)
    else:
        pipe = DecodePipeline(engine, list_size=8) if mode == "front+decoders" else DecodePipeline(engine, list_size=8, lanes=3)
    if mode.endswith("per wave"):
        for e in pipe.scl_engs:
            e.set_option("scl_multi", 1)
    if mode.endswith("per path"):
        pipe._flush_lanes = 1
    batches = [_workload(256, noise=n, seed=11 + k, ctr0=1000 * k) for k, n in enumerate((0.0, 0.05, 0.2, 0.0, 0.4, 0.1, 0.0))]
    dev = [_dev(engine, *w) for w in batches]
    out = [pipe.submit(f, b, p, select=(mode != "front+decoders")) for f, b, p in dev]           # all enqueued back to back
    pipe.synchronize()
    engine.set_option("scl_multi", -1)
    for (f, b, p), (sy, llr, scl, done) in zip(dev, out):
        if isinstance(scl, GroupTicket):
            scl = scl.result()
        if mode != "front+decoders":
            for u, v in zip(scl.selected, engine.select(scl)):
                assert torch.equal(u, v)
        rs, rl, rc = engine.decode_batch(f, b, p, list_size=8)
        torch.cuda.synchronize()
        assert torch.equal(sy.thr, rs.thr) and torch.equal(sy.peaks, rs.peaks) and torch.equal(sy.npeaks, rs.npeaks)
        assert torch.equal(llr, rl)
        assert torch.equal(scl.ncand, rc.ncand) and torch.equal(scl.hard_info, rc.hard_info)
        assert torch.equal(scl.cand_info, rc.cand_info) and torch.equal(scl.cand_metric, rc.cand_metric)
        assert torch.equal(scl.cand_ok, rc.cand_ok)


def test_front_batch_equals_separate_calls(engine):
    """es_front_batch (band-pass -> fused sync -> LLR in one library call) == the three calls: float32 and int16 records, given starts."""
    frames, band, pn = _workload(200, noise=0.2, seed=9)
    f, b, p = _dev(engine, frames, band, pn)
    st = torch.arange(200, device=engine.device, dtype=torch.int32) % 3
    for x in (f, (f * 20000).to(torch.int16)):
        for start in (None, st):
            y, thr, peaks, npeaks, flags, llr = engine.front(x, b, p, start=start)
            y2, y32 = engine.bpf2(x, b)
            thr2, peaks2, npeaks2, flags2 = engine.sync_fused(y2, y32, b)
            llr2 = engine.llr(y2, b, p, start=start, variant=0)
            for u, v in ((y, y2), (thr, thr2), (peaks, peaks2), (npeaks, npeaks2), (flags, flags2), (llr, llr2)):
                assert torch.equal(u, v)
    with pytest.raises(ValueError):
        engine.front(f.double(), b, p)


def test_front_end_context_and_stream_budget(engine):
    """es_create(device, 0): a front-end context runs everything but the list decoder and says so; pipelines warn when more streams are
    alive than the HIP runtime has hardware queues."""
    import os
    import warnings
    from echoseal_amd._native import NativeError
    from echoseal_amd.engine import RxEngine, DecodePipeline, hw_queue_budget, pipeline_streams
    fe = RxEngine(engine.device, list_size_max=0)
    frames, band, pn = _workload(64, noise=0.1, seed=3)
    f, b, p = _dev(engine, frames, band, pn)
    y, thr, peaks, npeaks, flags, llr = fe.front(f, b, p)
    y2, thr2, peaks2, npeaks2, flags2, llr2 = engine.front(f, b, p)
    assert torch.equal(y, y2) and torch.equal(peaks, peaks2) and torch.equal(llr, llr2)
    with pytest.raises(NativeError, match="front-end context"):
        fe.scl(llr, list_size=8)
    assert hw_queue_budget() == int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))      # the environment's value, never one the module set
    keep = []
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        for _ in range(hw_queue_budget() // 2 + 2):
            keep.append(DecodePipeline(engine, list_size=4, lanes=2))
        assert any("hardware queues" in str(x.message) for x in w)
    del keep


def test_pipeline_on_given_streams(engine):
    """DecodePipeline(streams=...) runs its lanes on existing HIP streams (a process should not keep more than eight alive):
    same rows as decode_batch; a wrong number of streams is refused."""
    from echoseal_amd.engine import DecodePipeline
    st = [torch.cuda.Stream(engine.device) for _ in range(2)]
    pipe = DecodePipeline(engine, list_size=4, lanes=2, streams=st)
    assert pipe.lane_streams == st
    dev = [_dev(engine, *_workload(128, noise=n, seed=40 + k, ctr0=500 * k)) for k, n in enumerate((0.0, 0.3, 0.1))]
    out = [pipe.submit(f, b, p) for f, b, p in dev]
    pipe.synchronize()
    for (f, b, p), (sy, llr, scl, done) in zip(dev, out):
        rs, rl, rc = engine.decode_batch(f, b, p, list_size=4)
        torch.cuda.synchronize()
        assert torch.equal(llr, rl) and torch.equal(scl.cand_info, rc.cand_info) and torch.equal(scl.cand_metric, rc.cand_metric)
    with pytest.raises(ValueError):
        DecodePipeline(engine, list_size=4, lanes=3, streams=st)


def test_grouped_pipeline_full_size_groups(engine):
    """The arrangement bench.py's headline runs, at its size: 40 batches of 1 024 frames (frames generated on the device, a different
    noise realisation per batch), groups of 16 on four front-end streams and two list-decoder streams -- two full groups decoded by
    the one-lane-per-path kernel while the next group's front ends run, and an incomplete group of 8.  Every batch's rows equal
    decode_batch's for that batch."""
    from echoseal_amd.engine import DecodePipeline
    pipe = DecodePipeline(engine, list_size=8, lanes=4, scl_streams=2, group=16)
    clean, _ = engine.synthetic_frames(KEY, 0, 1024)
    sec = WatermarkEmbedder(KEY).sec
    pn, band = engine.schedule(sec._prng.sub_key, KEY, ctr0=0, n=1024)
    gen = torch.Generator(device=engine.device); gen.manual_seed(77)
    batches = []
    for k in range(40):
        sigma = (0.0, 0.05, 0.2, 0.5)[k % 4]
        batches.append((clean + sigma * torch.randn(clean.shape, generator=gen, device=engine.device, dtype=torch.float32)).contiguous() if sigma else clean)
    torch.cuda.synchronize()
    out = [pipe.submit(f, band, pn) for f in batches]                   # all enqueued back to back
    pipe.synchronize()
    for f, (sy, llr, ticket, _) in list(zip(batches, out))[::3]:
        scl = ticket.result()
        rs, rl, rc = engine.decode_batch(f, band, pn, list_size=8)
        torch.cuda.synchronize()
        assert torch.equal(sy.thr, rs.thr) and torch.equal(sy.peaks, rs.peaks) and torch.equal(sy.npeaks, rs.npeaks)
        assert torch.equal(llr, rl)
        for name in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok"):
            assert torch.equal(getattr(scl, name), getattr(rc, name)), name
    assert int((out[-1][2].result().ncand > 0).sum()) > 900             # (the list decoder did run: few frames pass the hard-decision CRC)


def _sealed_blobs(rng, n, key=KEY):
    """n 55-byte blobs: sealed ESAL payloads, a third of them corrupted, some with a wrong magic / counter."""
    from echoseal_amd.crypto import SecureChannel
    sec = SecureChannel(key)
    blobs = np.zeros((n, 55), np.uint8); ctrs = np.zeros(n, np.int64)
    for i in range(n):
        ctr = int(rng.integers(0, 2 ** 32))
        pt = (b"ESAL" if i % 7 else b"ESAX") + ctr.to_bytes(4, "big") + rng.bytes(19)
        b = bytearray(sec.seal(pt, nonce=rng.bytes(12)))
        if i % 3 == 0:
            b[int(rng.integers(0, 55))] ^= 1 << int(rng.integers(0, 8))
        blobs[i] = np.frombuffer(bytes(b), np.uint8)
        ctrs[i] = ctr if i % 5 else (ctr + 1) % 2 ** 32
    return sec, blobs, ctrs


def test_aead_check_kernel_vs_oracle(engine, oracle):
    """the GPU validator equals the oracle (RFC 8439 restatement) bit for bit: verdicts and plaintexts,
    flat [n,55] and grouped [B,L,55] layouts, counters above 2^31."""
    rng = np.random.default_rng(21)
    sec, blobs, ctrs = _sealed_blobs(rng, 4096)
    key = sec._aead._key
    want_ok, want_plain = oracle.validate_blobs(key, blobs, ctrs)
    ok, plain = engine.aead_check(key, torch.from_numpy(blobs).to(engine.device), torch.from_numpy(ctrs), want_plain=True)
    assert np.array_equal(ok.cpu().numpy(), want_ok) and np.array_equal(plain.cpu().numpy(), want_plain)
    assert 0 < int(want_ok.sum()) < len(want_ok)
    # grouped: 512 frames x 8 candidates, one counter per frame
    g = blobs.reshape(512, 8, 55); gc = ctrs[::8].copy()
    want_g, _ = oracle.validate_blobs(key, blobs, np.repeat(gc, 8))
    okg = engine.aead_check(key, torch.from_numpy(g).to(engine.device), torch.from_numpy(gc))
    assert np.array_equal(okg.cpu().numpy().reshape(-1), want_g)
    with pytest.raises(ValueError):
        engine.aead_check(key[:31], torch.from_numpy(blobs).to(engine.device), torch.from_numpy(ctrs))


@pytest.mark.parametrize("L", [8, 64])
def test_select_kernel_vs_oracle_and_host_rules(engine, oracle, L):
    """Candidate selection on the GPU == oracle == the host replay of rtwm/fastpolar.py:268-276,332-359
    (engine.select_payload), with validator None and with the AEAD validator.  The candidate lists are real list-decoder
    outputs with sealed blobs planted at chosen positions so that every branch is taken."""
    from echoseal_amd.engine import RxEngine, select_payload
    eng = engine if L <= engine.list_size_max else RxEngine(0, list_size_max=L)
    rng = np.random.default_rng(33 + L)
    B = 96
    llr = torch.from_numpy(np.clip(rng.normal(0, 3, (B, 1024)), -12, 12).astype(np.float32)).to(eng.device)
    res = eng.scl(llr, list_size=L, skip_if_hard_ok=False)
    from echoseal_amd.crypto import SecureChannel
    sec = SecureChannel(KEY)
    key = sec._aead._key
    true_ctr = rng.integers(0, 2 ** 32, B)
    blobs = np.stack([np.frombuffer(sec.seal(b"ESAL" + int(c).to_bytes(4, "big") + rng.bytes(19), nonce=rng.bytes(12)), np.uint8)
                      for c in true_ctr])
    ctrs = np.where(np.arange(B) % 12 >= 6, (true_ctr + 1) % 2 ** 32, true_ctr).astype(np.int64)   # second half-dozen: wrong counter
    ci = res.cand_info.cpu().numpy().copy(); co = res.cand_ok.cpu().numpy().copy()
    hi = res.hard_info.cpu().numpy().copy(); ho = res.hard_ok.cpu().numpy().copy()
    for f in range(B):
        mode = f % 6
        if mode == 0:   hi[f] = blobs[f]; ho[f] = 1                      # valid hard candidate
        elif mode == 1: ci[f, L // 2] = blobs[f]; co[f, L // 2] = 1; co[f, 1] = 1   # CRC-ok decoy first, valid one later
        elif mode == 2: co[f, :] = 0                                     # nothing passes CRC
        elif mode == 3: co[f, 3] = 1                                     # CRC-ok but never valid
        elif mode == 4: ci[f, 0] = blobs[f]; co[f, 0] = 0                # valid blob whose CRC flag is off: must be ignored
        else:           hi[f] = blobs[f]; ho[f] = 0; ci[f, L - 1] = blobs[f]; co[f, L - 1] = 1
    res.cand_info.copy_(torch.from_numpy(ci)); res.cand_ok.copy_(torch.from_numpy(co))
    res.hard_info.copy_(torch.from_numpy(hi)); res.hard_ok.copy_(torch.from_numpy(ho))
    cm = res.cand_metric.cpu().numpy(); nc = res.ncand.cpu().numpy()
    for use_key in (False, True):
        payload, ok, which = eng.select(res, key32=key if use_key else None, ctrs=torch.from_numpy(ctrs) if use_key else None)
        payload = payload.cpu().numpy(); ok = ok.cpu().numpy(); which = which.cpu().numpy()
        seen = set()
        for f in range(B):
            wp, wok, ww = oracle.select_validated(key if use_key else None, ctrs[f], hi[f], ho[f], ci[f], co[f], cm[f], nc[f])
            assert payload[f].tobytes() == wp and int(ok[f]) == wok and int(which[f]) == ww
            def val(p, c=int(ctrs[f])):
                pt = sec.open(p)
                return pt.startswith(b"ESAL") and int.from_bytes(pt[4:8], "big") == c
            hp, hok = select_payload(res, f, val if use_key else None)
            assert hp == wp and bool(hok) == (wok == 1)
            seen.add((wok, ww == -1))
        assert len(seen) >= 3


@pytest.mark.parametrize("L", [1, 2, 4, 8, 16, 24, 32])
def test_scl_multi_frames_per_wave(engine, oracle, L):
    """es_scl_multi.hip (16/L frames per wavefront; L = 32 as 32 paths x 2 lanes) returns exactly what the one-frame-per-wave kernel and the oracle
    return: random LLRs, clipped LLRs (exact ties), hard-decision hits mixed in (skipped frames inside a wave), a batch
    size that is not a multiple of the frames per wave, float32 and float64 inputs."""
    rng = np.random.default_rng(100 + L)
    B = 16 * 13 + 5
    llr = np.clip(rng.normal(0, 4, (B, 1024)), -12, 12).astype(np.float32)
    llr[::7] = np.clip(llr[::7] * 6, -12, 12)                       # heavily clipped rows
    info = rng.integers(0, 256, (B, 55), dtype=np.uint8)
    code = engine.polar_encode(torch.from_numpy(info).to(engine.device)).cpu().numpy()
    hit = np.arange(B) % 5 == 2                                     # rows whose hard decision passes the CRC
    llr[hit] = ((code[hit].astype(np.float32) * 2 - 1) * 3.0)
    for dtype in (torch.float32, torch.float64):
        x = torch.from_numpy(llr).to(engine.device).to(dtype)
        for skip in (True, False):
            engine.set_option("scl_multi", 0)
            ref = engine.scl(x, list_size=L, skip_if_hard_ok=skip)
            engine.set_option("scl_multi", 1)
            got = engine.scl(x, list_size=L, skip_if_hard_ok=skip)
            engine.set_option("scl_lanes", 1)                       # one lane per path, 64/L frames per wave (es_scl_wide.hip)
            got1 = engine.scl(x, list_size=L, skip_if_hard_ok=skip)
            engine.set_option("scl_lanes", 0)
            engine.set_option("scl_multi", -1)
            for name in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok"):
                assert torch.equal(getattr(ref, name), getattr(got, name)), (name, L, dtype, skip)
                assert torch.equal(getattr(ref, name), getattr(got1, name)), (name, L, dtype, skip, "one lane per path")
            assert bool(torch.all(got.hard_ok[torch.from_numpy(hit).to(engine.device)] == 1))
    for i in range(0, B, 41):
        if hit[i]:
            continue
        nn, ci, cm, cc = oracle.scl_list(llr[i].astype(np.float64), L)
        assert int(got.ncand[i]) == nn
        assert np.array_equal(np.packbits(ci[:nn], axis=1), got.cand_info[i, :nn].cpu().numpy())
        assert np.array_equal(cm[:nn], got.cand_metric[i, :nn].cpu().numpy())
        assert np.array_equal(cc[:nn], got.cand_ok[i, :nn].cpu().numpy())


@pytest.mark.parametrize("L", [2, 8, 24, 64, 256])
def test_scl_compacted_launch(L):
    """skip_if_hard_ok on the lane-per-path kernel: the hard-decision shortcut runs for every frame first, a one-block scan lists the frames
    that failed it and the list kernel decodes only those (a wave would otherwise carry the settled frames along as idle lanes).  Frames
    that pass and frames that do not, mixed at random / all / none, ragged batch sizes: the rows of the listed frames equal an uncompacted
    launch's, the settled frames read ncand = 0 and zero rows, hard_info / hard_ok are the same."""
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=256)
    eng.set_option("scl_multi", 1); eng.set_option("scl_lanes", 1)
    rng = np.random.default_rng(40 + L)
    info = rng.integers(0, 256, (600, 55), dtype=np.uint8)
    code = eng.polar_encode(torch.from_numpy(info).to(eng.device)).cpu().numpy().astype(np.float64)
    clean = (2.0 * code - 1.0) * 6.0                                                  # passes the hard decision
    noisy = np.clip(2.0 * (2.0 * code - 1.0 + rng.normal(0, 1.0, code.shape)), -12, 12)   # does not
    for B, share in ((1, 0.0), (1, 1.0), (7, 0.5), (8, 0.5), (9, 0.9), (65, 0.0), (130, 1.0), (600, 0.3), (600, 0.97)):
        if L > 64 and B > 130:
            continue
        pick = rng.random(B) < share
        x = np.where(pick[:, None], noisy[:B], clean[:B]).astype(np.float32)
        t = torch.from_numpy(x).to(eng.device)
        full = eng.scl(t, list_size=L, skip_if_hard_ok=False).check()
        comp = eng.scl(t, list_size=L, skip_if_hard_ok=True).check()
        assert torch.equal(full.hard_info, comp.hard_info) and torch.equal(full.hard_ok, comp.hard_ok), (B, share)
        hok = full.hard_ok.cpu().numpy().astype(bool)
        assert np.array_equal(hok, ~pick) or share in (0.5, 0.9, 0.3, 0.97), (B, share)     # (a noisy frame may pass by luck)
        took = torch.from_numpy(~hok).to(eng.device)
        assert torch.equal(comp.ncand[~took], torch.zeros_like(comp.ncand[~took])) and torch.equal(comp.ncand[took], full.ncand[took]), (B, share)
        for name in ("cand_info", "cand_metric", "cand_ok"):
            a, c = getattr(full, name), getattr(comp, name)
            assert torch.equal(a[took], c[took]), (name, B, share)
            assert not bool(c[~took].to(torch.float64).abs().sum().item()), (name, B, share)
    eng.close()


@pytest.mark.parametrize("L", [1, 8, 32])
def test_scl_softplus_fallback_ranges(engine, oracle, L):
    """Operands that leave the straight-line softplus of the list decoders: |t| >= 512 (sums of many +-12 LLRs, float64 LLRs of
    magnitude up to 400 -- exp underflows to subnormals and to zero): the hot loops only flag such lanes and redo the evaluation with
    the generic form outside the loop.  And 1 + e^t within 3 * 2^-20 below 2 (operands that differ by ~1e-7: fdlibm's |f| < 2^-20 corner,
    a select inside the straight-line form since round 3).  Every mapping must equal the oracle bit for bit."""
    rng = np.random.default_rng(900 + L)
    rows = []
    for k in range(24):
        kind = k % 6
        if kind == 0:                                   # all +-12: |g| doubles per level, 768 at depth 6
            v = rng.choice([-12.0, 12.0], 1024)
        elif kind == 1:                                 # near-equal halves at every stride: tiny non-zero differences / sums
            base = np.clip(rng.normal(0, 3, 1024), -12, 12)
            v = base.copy()
            for st in (512, 256, 128):
                idx = np.arange(1024)
                m = (idx // st) % 2 == 1
                v[m] = v[idx[m] - st] * rng.choice([-1.0, 1.0]) + rng.normal(0, 2e-7, int(m.sum()))
        elif kind == 2:                                 # big float64 magnitudes: sums beyond 708 and 745
            v = rng.normal(0, 150, 1024)
        elif kind == 3:                                 # a real codeword at magnitude 12 with a few flips
            info = rng.integers(0, 256, (1, 55), dtype=np.uint8)
            code = engine.polar_encode(torch.from_numpy(info).to(engine.device)).cpu().numpy()[0]
            v = (code * 2.0 - 1.0) * 12.0
            v[rng.choice(1024, 30, replace=False)] *= -1
        elif kind == 4:                                 # mixed: strong and tiny
            v = rng.choice([-300.0, -12.0, -1e-7, 1e-7, 12.0, 300.0], 1024)
        else:
            v = np.clip(rng.normal(0, 40, 1024), -400, 400)
        rows.append(v)
    llr = np.stack(rows)
    x = torch.from_numpy(llr).to(engine.device)          # float64 input
    outs = []
    for multi, lanes in ((0, 4), (1, 4), (1, 2), (1, 1)):
        engine.set_option("scl_multi", multi); engine.set_option("scl_lanes", lanes)
        try:
            outs.append(engine.scl(x, list_size=L, skip_if_hard_ok=False))
        finally:
            engine.set_option("scl_multi", -1); engine.set_option("scl_lanes", 0)
    for o in outs[1:]:
        for name in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_metric", "cand_ok"):
            assert torch.equal(getattr(outs[0], name), getattr(o, name)), (name, L)
    got = outs[-1]
    for i in range(llr.shape[0]):
        nn, ci, cm, cc = oracle.scl_list(llr[i], L)
        assert int(got.ncand[i]) == nn, i
        assert np.array_equal(np.packbits(ci[:nn], axis=1), got.cand_info[i, :nn].cpu().numpy()), i
        assert np.array_equal(cm[:nn].view(np.uint64), got.cand_metric[i, :nn].cpu().numpy().view(np.uint64)), i
        assert np.array_equal(cc[:nn], got.cand_ok[i, :nn].cpu().numpy()), i


def test_llr_shift_search_screen_is_exact(engine, oracle):
    """The LLR kernel scores only the shifts that a float64 exact-sum screen cannot rule out.  Winner, LLRs and BOTH
    reported scores (best, runner-up) must still equal the oracle, which scores every shift: clean and noisy frames,
    pure noise (flat score curve), constants (every shift ties), a click, huge and tiny amplitudes."""
    ba, tpl, taps, ntaps, _ = pack_tables()
    rng = np.random.default_rng(61)
    frames, band, pn = _workload(24, noise=0.0)
    x = frames.astype(np.float64).copy()
    x[4:8] += rng.normal(0, 0.5, x[4:8].shape)                      # noisy
    x[8:12] = rng.normal(0, 0.3, x[8:12].shape)                      # noise only
    x[12] = 0.25                                                     # constant: all shifts tie
    x[13] = 0.0; x[13, 700] = 1.0                                    # click
    x[14] *= 1e12; x[15] *= 1e-12; x[16] *= 1e-25
    x[17] = 0.0
    x[18] = np.sign(rng.normal(0, 1, 1215)) * 0.1                    # +-0.1: equal magnitudes everywhere
    x[19] = np.tile(rng.normal(0, 0.2, 27), 45)                      # period 27: repeating scores
    y, b, p = _dev(engine, x, band, pn)
    llr, bs, sc = engine.llr(y, b, p, want_diag=True)
    llr = llr.cpu().numpy(); bs = bs.cpu().numpy(); sc = sc.cpu().numpy()
    for i in range(len(x)):
        o, obs, best, second = oracle.llr(x[i], np.unpackbits(pn[i])[191:1215], taps[band[i], :ntaps[band[i]]])
        assert obs == int(bs[i]), i
        assert np.array_equal(o, llr[i]), i
        assert np.float32(best) == sc[i, 0] and np.float32(second) == sc[i, 1], (i, best, second, sc[i])


def test_schedule_kernel_vs_oracle(engine, oracle):
    """es_schedule_batch (AES-128 PN rows + HMAC-SHA256 band hop on the device) == oracle == the host code behind the
    broadcast schedule: explicit counters (including > 2^31), a contiguous range, and 2^20 counters spot-checked."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.dist import build_schedule
    for key in (KEY, b"\x00" * 32, bytes(range(32))):
        sec = SecureChannel(key)
        ctrs = [0, 1, 2, 3, 5, 255, 1024, 65535, 2 ** 31 + 5, 2 ** 32 - 1] + [int(c) for c in np.random.default_rng(9).integers(0, 2 ** 32, 300)]
        pn, band = engine.schedule(sec._prng.sub_key, key, torch.tensor(ctrs, dtype=torch.int64))
        wpn, wband = oracle.schedule_rows(sec._prng.sub_key, key, ctrs)
        assert np.array_equal(pn.cpu().numpy(), wpn) and np.array_equal(band.cpu().numpy(), wband)
    sec = SecureChannel(KEY)
    pn, band = engine.schedule(sec._prng.sub_key, KEY, ctr0=1000, n=4097)
    ref = build_schedule(KEY, range(1000, 1000 + 4097))
    assert np.array_equal(pn.cpu().numpy(), ref[:, :152]) and np.array_equal(band.cpu().numpy(), ref[:, 152])
    n = 1 << 20
    pn, band = engine.schedule(sec._prng.sub_key, KEY, ctr0=0, n=n)
    idx = np.random.default_rng(10).integers(0, n, 64)
    ref = build_schedule(KEY, [int(i) for i in idx])
    assert np.array_equal(pn[torch.from_numpy(idx).to(engine.device)].cpu().numpy(), ref[:, :152])
    assert np.array_equal(band[torch.from_numpy(idx).to(engine.device)].cpu().numpy(), ref[:, 152])
    with pytest.raises(ValueError):
        engine.schedule(b"short", KEY, ctr0=0, n=4)


@pytest.mark.parametrize("T", [63, 64, 70, 200, 1214, 1216, 2047, 2048, 3001, 4158])
def test_sync_fast_record_lengths(engine, T):
    """Record lengths around every boundary of the fast path (one lag, fewer than five lags, odd / even counts, the
    frame and window specialisations +-1, several correlation segments, the 4 096-lag maximum): thr, npeaks and peaks
    equal the all-float64 path.  Rows mix noise, a planted frame (when it fits), a tone and a constant."""
    rng = np.random.default_rng(T)
    B = 24
    x = rng.normal(0, 0.2, (B, T)).astype(np.float32)
    frames, band, _ = _workload(B)
    if T >= 1215:
        for i in range(0, B, 3):
            off = (i * 37) % (T - 1215 + 1)
            x[i, off:off + 1215] += frames[i]
    x[1] = np.sin(2 * np.pi * 9000 / 48000 * np.arange(T)).astype(np.float32)
    x[2] = 0.125
    f, b = _dev(engine, x, band)
    ref = engine.sync(f, b, keep_corr=False)
    fast = engine.sync_fast(f, b)
    assert torch.equal(ref.thr, fast.thr) and torch.equal(ref.npeaks, fast.npeaks)
    k = (ref.npeaks & 0xFFFF).clamp(max=32)
    mask = torch.arange(32, device=engine.device)[None, :] < k[:, None]
    assert torch.equal(ref.peaks[mask], fast.peaks[mask])


def test_frame_generator_equals_host_embedder(engine):
    """frames generated on the device (polar encode -> schedule -> chips -> band-pass -> peak rule) are
    bit-identical to WatermarkEmbedder.make_frames (itself pinned to the reference's frames in tests/test_host_api.py),
    for counters in every band, large counters, and both keys of the fixtures."""
    for key in (KEY, b"\x00" * 32):
        tx = WatermarkEmbedder(key)
        ctrs = list(range(40)) + [255, 256, 65535, 65536, 70000, 2 ** 31 + 7, 2 ** 32 - 1]
        payloads = synthetic_payloads(tx.sec, ctrs)
        want = tx.make_frames(ctrs, payloads)
        pl = torch.from_numpy(np.frombuffer(b"".join(payloads), np.uint8).reshape(len(ctrs), 55).copy())
        got = engine.make_frames(tx.sec, key, torch.tensor(ctrs, dtype=torch.int64), pl).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert len({band_index(key, c) for c in ctrs}) == 4
    # decode what was generated: the device-made frames go through the receive path like host-made ones
    tx = WatermarkEmbedder(KEY); ctrs = list(range(64))
    payloads = synthetic_payloads(tx.sec, ctrs)
    pl = torch.from_numpy(np.frombuffer(b"".join(payloads), np.uint8).reshape(64, 55).copy())
    frames = engine.make_frames(tx.sec, KEY, torch.tensor(ctrs), pl)
    pn, band = engine.schedule(tx.sec._prng.sub_key, KEY, ctr0=0, n=64)
    sy, llr, scl = engine.decode_batch(frames, band, pn, list_size=8)
    assert bool(torch.all(sy.peaks[:, 0] == 0))


def test_decode_batch_is_graph_capturable(engine):
    """After a warm-up call no entry point allocates or synchronises, so a whole decode_batch (band-pass, screen, exact
    picking + redo kernels, LLR on a side stream, list decoder) can be captured into a HIP graph; the replay on new
    input data gives what an eager call gives."""
    frames, band, pn = _workload(128, noise=0.1, seed=5)
    f, b, p = _dev(engine, frames, band, pn)
    for _ in range(2):
        engine.decode_batch(f, b, p, list_size=8)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = engine.decode_batch(f, b, p, list_size=8)
    frames2, _, _ = _workload(128, noise=0.3, seed=6)
    f.copy_(torch.from_numpy(frames2))                         # new samples in the captured input buffer
    g.replay()
    torch.cuda.synchronize()
    ref = engine.decode_batch(f, b, p, list_size=8)
    torch.cuda.synchronize()
    assert torch.equal(out[0].thr, ref[0].thr) and torch.equal(out[0].npeaks, ref[0].npeaks) and torch.equal(out[1], ref[1])
    assert torch.equal(out[2].cand_info, ref[2].cand_info) and torch.equal(out[2].cand_metric, ref[2].cand_metric)
    assert torch.equal(out[2].ncand, ref[2].ncand)


@pytest.mark.parametrize("fs_in", [44100, 22050, 96000, 47999, 8000])
def test_resample_kernel_equals_scipy(engine, oracle, fs_in):
    """es_resample_batch returns scipy.signal.resample_poly's values bit for bit (float32, float64 and
    int16 signals; single clip and batch), i.e. what the reference's resample_to hands to the detector."""
    from scipy.signal import resample_poly
    import math
    rng = np.random.default_rng(fs_in)
    g = math.gcd(fs_in, 48000); up, down = 48000 // g, fs_in // g
    for dtype in (np.float32, np.float64, np.int16):
        n = int(rng.integers(2000, 30000))
        x = rng.normal(0, 0.3, n)
        x = (x * 20000).astype(np.int16) if dtype == np.int16 else x.astype(dtype)
        ref = resample_poly(x, up, down)
        got = engine.resample(x, fs_in, 48000).cpu().numpy()
        assert got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8))
        assert np.array_equal(oracle.resample_poly(x, up, down).view(np.uint8), ref.view(np.uint8))
    xb = rng.normal(0, 0.2, (5, 4000)).astype(np.float32)
    gb = engine.resample(xb, fs_in, 48000).cpu().numpy()
    for i in range(5):
        assert np.array_equal(gb[i].view(np.uint8), resample_poly(xb[i], up, down).view(np.uint8))


def test_aead_seal_kernel(engine, oracle):
    """es_aead_seal_batch == SecureChannel.seal (host, RFC 8439-pinned) for random plaintexts and nonces; and what it
    seals opens with the device validator and with the oracle."""
    from echoseal_amd.crypto import SecureChannel
    rng = np.random.default_rng(77)
    sec = SecureChannel(KEY); key = sec._aead._key
    n = 2048
    ctrs = rng.integers(0, 2 ** 32, n)
    plain = np.zeros((n, 27), np.uint8)
    plain[:, :4] = np.frombuffer(b"ESAL", np.uint8)
    plain[:, 4:8] = ctrs.astype(">u4").view(np.uint8).reshape(n, 4)
    plain[:, 8:] = rng.integers(0, 256, (n, 19), dtype=np.uint8)
    nonces = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    blobs = engine.aead_seal(key, torch.from_numpy(nonces), torch.from_numpy(plain)).cpu().numpy()
    for i in range(0, n, 97):
        assert blobs[i].tobytes() == sec.seal(plain[i].tobytes(), nonce=nonces[i].tobytes())
    ok, pt = engine.aead_check(key, torch.from_numpy(blobs).to(engine.device), torch.from_numpy(ctrs.astype(np.int64)), want_plain=True)
    assert bool(torch.all(ok == 1)) and np.array_equal(pt.cpu().numpy(), plain)
    wok, wpt = oracle.validate_blobs(key, blobs[:64], ctrs[:64])
    assert wok.all() and np.array_equal(wpt, plain[:64])


def test_option_and_argument_errors(engine):
    """Error behaviour of the newer entry points: unknown / out-of-range options, mismatched shapes and key lengths raise
    (NativeError from the C ABI's negative return codes, ValueError from the host wrappers) and leave the engine usable."""
    from echoseal_amd._native import NativeError
    with pytest.raises(NativeError):
        engine.set_option("no_such_option", 1)
    with pytest.raises(NativeError):
        engine.set_option("scl_multi", 7)
    with pytest.raises(ValueError):
        engine.schedule(b"\x00" * 16, b"\x00" * 31, ctr0=0, n=4)
    with pytest.raises(ValueError):
        engine.aead_seal(b"\x00" * 32, torch.zeros((3, 12), dtype=torch.uint8), torch.zeros((4, 27), dtype=torch.uint8))
    with pytest.raises(ValueError):
        engine.aead_check(b"\x00" * 32, torch.zeros((3, 54), dtype=torch.uint8), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        engine.make_frames(__import__("echoseal_amd.crypto", fromlist=["SecureChannel"]).SecureChannel(KEY), KEY,
                           torch.arange(4), torch.zeros((3, 55), dtype=torch.uint8))
    engine.set_option("scl_multi", -1)
    pn, band = engine.schedule(b"\x01" * 16, KEY, ctr0=0, n=0)            # empty batches are fine
    assert pn.shape == (0, 152) and band.numel() == 0
    assert engine.resample(np.zeros(0, np.float32), 44100, 48000).numel() == 0


def test_device_softplus_bits(engine, oracle):
    """The device's log1p(exp(t)) -- straight-line form with the guard-free division (es_div_normal) and the generic
    fall-back -- against the HOST C library, bit for bit, on 3 million arguments over every range the decoder produces
    (es_math.h is also what the oracle compiles, but with `/`; this is the check of the device-only division)."""
    import ctypes
    m = ctypes.CDLL("libm.so.6")
    rng = np.random.default_rng(2026)
    t = np.concatenate([
        -np.abs(rng.normal(0, 6, 1_000_000)), -rng.uniform(0, 1.0, 500_000), -rng.uniform(0.85, 0.92, 200_000),
        -rng.uniform(15, 45, 300_000), -rng.uniform(0, 800, 300_000), -np.abs(rng.normal(0, 3000, 200_000)),
        -np.ldexp(rng.uniform(0.5, 1, 300_000), -rng.integers(0, 80, 300_000)),
        -(10.0 ** rng.uniform(-18, -4, 300_000)), -(2.86e-6 + rng.uniform(-1e-7, 1e-7, 50_000)),      # fdlibm's |f| < 2^-20 corner of log1p (a select
        -(1.1e-16 + rng.uniform(-1e-16, 2e-16, 50_000)),                                                #  in the straight-line form) and both its edges
        -np.arange(0, 24.0, 1.0 / 8192),                                            # a regular grid (clipped-LLR differences)
        np.array([0.0, -0.0, -0.8813735870195429, -0.881373587019543, -0.8813735870195432, -20.1, -20.101268236238414,
                  -37.42994775023705, -37.5, -511.9, -512.0, -745.2, -1e-300, -2.0 ** -54, -2.0 ** -55, -np.inf])])
    got = engine.softplus(torch.from_numpy(t).to(engine.device)).cpu().numpy()
    want = oracle.log1p_vec(oracle.exp_vec(t))                                      # == libm (tests/test_oracle_math.py)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    exp_, log1p_ = m.exp, m.log1p
    exp_.restype = log1p_.restype = ctypes.c_double; exp_.argtypes = log1p_.argtypes = [ctypes.c_double]
    idx = rng.integers(0, t.size, 20000)
    ref = np.array([log1p_(exp_(float(v))) for v in t[idx]])
    assert np.array_equal(got[idx].view(np.uint64), ref.view(np.uint64))


@pytest.mark.parametrize("T", [1215, 2048, 700, 63, 64, 190, 3000, 4158])
def test_sync_fused_equals_float64_path(engine, T):
    """es_sync_fused_batch (screen row in LDS, histogram shortcuts) == es_xcorr_batch + es_pick_batch, bit for bit:
    clean frames, noisy frames, pure noise, low-level noise (threshold does not saturate), silence, constants, spikes."""
    rng = np.random.default_rng(T)
    B = 160
    frames, band, _ = _workload(B)
    x = np.zeros((B, T), np.float32)
    m = min(T, 1215)
    x[:, :m] = frames[:, :m]
    x[32:64] += rng.normal(0, 0.05, (32, T)).astype(np.float32)                 # noisy frames
    x[64:96] = rng.normal(0, 0.3, (32, T)).astype(np.float32)                   # pure noise
    if T >= 400:
        x[96:112] = 0.0; x[96:112, 50:50 + min(m, T - 50)] = frames[96:112, :min(m, T - 50)]   # frame at an offset, silence around it
        x[112:120] = (1e-3 * rng.normal(0, 1, (8, T))).astype(np.float32); x[112:120, :m] += frames[112:120, :m]
    x[120:124] = 0.0                                                            # digital silence -> flagged, float64 redo
    x[124:128] = 0.25                                                           # constant
    x[128:132] = 0.0; x[128:132, T // 2] = 1.0                                  # one spike
    x[132:140] = np.round(rng.normal(0, 2, (8, T))).astype(np.float32)          # coarse integers: many exact ties
    x[140:150] = (1e-20 * rng.normal(0, 1, (10, T))).astype(np.float32)         # tiny amplitudes
    x[150:160] = (1e15 * rng.normal(0, 1, (10, T))).astype(np.float32)          # huge amplitudes
    f, b = _dev(engine, x, band)
    want = engine.sync(f, b, keep_corr=False)
    y, y32 = engine.bpf2(f, b)
    thr, peaks, npeaks, flags = engine.sync_fused(y, y32, b)
    assert torch.equal(thr, want.thr) and torch.equal(npeaks, want.npeaks)
    n = (want.npeaks & 0xFFFF).clamp(max=32)
    mask = torch.arange(32, device=engine.device)[None, :] < n[:, None]
    assert torch.equal(torch.where(mask, peaks, -1), torch.where(mask, want.peaks, -1))
    assert torch.all(peaks[~mask] == -1)
    if T >= 1215:                                                               # ordinary records never need the float64 redo
        assert int(flags[32:96].sum()) == 0                                     # (clean frames padded with digital silence do:
        assert T > 1215 or int(flags[:32].sum()) == 0                           #  hundreds of exactly equal correlations)


def test_sync_fused_full_size_properties(engine):
    """65 536 config-3 windows: fused == unfused (es_xcorr32_batch + es_pick_exact_batch) on every record."""
    from echoseal_amd import workloads as WL
    fr, _ = engine.synthetic_frames(KEY, 0, 16384)
    win, off = WL.c3_windows_device(fr.repeat(4, 1))
    sec_band = engine.schedule(WatermarkEmbedder(KEY).sec._prng.sub_key, KEY, ctr0=0, n=16384)[1].repeat(4)
    y, y32 = engine.bpf2(win, sec_band)
    a = engine.sync_fused(y, y32, sec_band)
    b = engine.pick_exact(engine.xcorr32(y32, sec_band), y, sec_band)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _decode_chunks(engine, frames, band, pn, chunk):
    outs = []
    for c0 in range(0, frames.shape[0], chunk):
        sy, llr, scl = engine.decode_batch(frames[c0:c0 + chunk], band[c0:c0 + chunk], pn[c0:c0 + chunk], list_size=8)
        payload, ok, which = engine.select(scl)
        outs.append((sy.peaks[:, 0].clone(), sy.npeaks.clone(), sy.thr.clone(), payload, ok, llr[:, ::64].clone()))
    return [torch.cat(t) for t in zip(*outs)]


def test_c4_shard_131072_properties(engine, oracle):
    """One BASELINE config-4 shard (2^20 frames / 8 GPUs = 131 072 clean frames, ctr 524288..): every frame syncs at
    offset 0 with the saturated threshold; results do not depend on how the shard is cut into launches; sampled frames
    equal the CPU oracle bit for bit (sync, LLR, SCL-8 list)."""
    n, c0 = 131072, 524288
    tx = WatermarkEmbedder(KEY)
    frames = torch.cat([engine.synthetic_frames(KEY, c0 + k, 32768)[0] for k in range(0, n, 32768)])
    pn, band = engine.schedule(tx.sec._prng.sub_key, KEY, ctr0=c0, n=n)
    a = _decode_chunks(engine, frames, band, pn, 131072)
    b = _decode_chunks(engine, frames, band, pn, 40000)             # ragged chunks
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    peak0, npk, thr, payload, ok, _ = a
    assert bool((peak0 == 0).all()) and bool((thr == 0.95).all()) and bool(((npk & 0xFFFF) >= 1).all())
    ba, tpl, taps, ntaps, _ = pack_tables()
    fh = frames.cpu().numpy(); bh = band.cpu().numpy(); ph = pn.cpu().numpy()
    sy, llr, _ = engine.decode_batch(frames[:64 * 2048:2048].contiguous(), band[:64 * 2048:2048].contiguous(), pn[:64 * 2048:2048].contiguous(), list_size=8)
    res = engine.scl(llr, list_size=8, skip_if_hard_ok=False)
    for j in range(0, 64, 9):
        i = j * 2048
        o = oracle.decode_frame(fh[i], ba[bh[i]], tpl[bh[i]], taps[bh[i], :ntaps[bh[i]]], np.unpackbits(ph[i])[:1215], L=8)
        assert np.array_equal(o["llr"], llr[j].cpu().numpy()) and o["thr"] == float(sy.thr[j])
        nn, ci, cm, cc = oracle.scl_list(o["llr"].astype(np.float64), 8)
        assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[j].cpu().numpy()) and np.array_equal(cm, res.cand_metric[j].cpu().numpy())


def test_c4_full_2pow20_properties(engine):
    """All 2^20 frames of BASELINE config 4 on one GPU (frames made on the device, 131 072 per launch): sync offset 0 and
    saturated threshold everywhere, and a second pass over a differently cut stream gives identical payloads / flags."""
    n = 1 << 20
    tx = WatermarkEmbedder(KEY)
    frames = torch.empty((n, 1215), dtype=torch.float32, device=engine.device)
    for k in range(0, n, 65536):
        frames[k:k + 65536] = engine.synthetic_frames(KEY, k, 65536)[0]
    pn, band = engine.schedule(tx.sec._prng.sub_key, KEY, ctr0=0, n=n)
    peak0, npk, thr, payload, ok, llr_s = _decode_chunks(engine, frames, band, pn, 131072)
    assert bool((peak0 == 0).all()) and bool((thr == 0.95).all())
    assert int(ok.numel()) == n and bool(torch.isfinite(llr_s).all()) and float(llr_s.abs().max()) <= 12.0
    lo, hi = 300000, 300000 + 98304                                 # a window that straddles launch boundaries of the first pass
    again = _decode_chunks(engine, frames[lo:hi], band[lo:hi], pn[lo:hi], 98304)
    assert torch.equal(again[3], payload[lo:hi]) and torch.equal(again[4], ok[lo:hi]) and torch.equal(again[5], llr_s[lo:hi])
    # the band of a counter is the device schedule's: equal to the host HMAC for sampled counters
    from echoseal_amd.utils import band_index
    for c in (0, 1, 65535, 65536, 999_999, n - 1):
        assert int(band[c]) == band_index(KEY, c)


def test_c5_surrogate_list_sweep_vs_oracle(engine, oracle):
    """BASELINE config 5 needs an MP3 codec; the image has none (MP3 itself: skipped).  The documented SURROGATE channel
    (echoseal_amd.workloads.lossy_channel: 16 kHz low-pass + level-shaped noise -- NOT MP3) takes its place: list size swept
    over 1 / 4 / 8 / 16, HIP == oracle on sync offsets, LLRs and (payload, ok) for every frame and list size."""
    from echoseal_amd import workloads as WL
    frames, band, pn, payloads = WL.c2_frames(range(96))
    lossy = WL.lossy_channel(frames)
    assert lossy.shape == frames.shape and np.isfinite(lossy).all() and not np.array_equal(lossy, frames)
    ba, tpl, taps, ntaps, _ = pack_tables()
    f, b, p = _dev(engine, lossy, band, pn)
    ref = [oracle.decode_frame(lossy[i], ba[band[i]], tpl[band[i]], taps[band[i], :ntaps[band[i]]], np.unpackbits(pn[i])[:1215], L=1)
           for i in range(96)]
    for L in (1, 4, 8, 16):
        sy, llr, scl = engine.decode_batch(f, b, p, list_size=L)
        payload, ok, which = engine.select(scl)
        payload = payload.cpu().numpy(); ok = ok.cpu().numpy(); llr_h = llr.cpu().numpy()
        for i in range(96):
            k = int(sy.npeaks[i]) & 0xFFFF
            assert list(sy.peaks[i, :k].cpu().numpy()) == list(ref[i]["peaks"][:k]) and np.array_equal(llr_h[i], ref[i]["llr"])
            info, okr, _ = oracle.polar_decode(ref[i]["llr"].astype(np.float64), L)
            assert np.packbits(info).tobytes() == payload[i].tobytes() and bool(okr) == (ok[i] == 1), (L, i)


def test_contexts_on_two_devices():
    """Kernel attributes (dynamic LDS above 64 KB for list size 256 and for the exact picker) are raised per context, i.e.
    per device: a context on a second GPU of the same process works like the first.  Needs two visible GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    from echoseal_amd.engine import RxEngine
    rng = np.random.default_rng(5)
    llr = np.clip(rng.normal(0, 3, (4, 1024)), -12, 12).astype(np.float32)
    x = rng.normal(0, 0.1, (4, 3000)).astype(np.float32); band = np.array([0, 1, 2, 3], np.uint8)
    outs = []
    for d in (0, 1):
        eng = RxEngine(d, list_size_max=256)
        r = eng.scl(torch.from_numpy(llr).to(eng.device), list_size=256, skip_if_hard_ok=False)
        f, b = torch.from_numpy(x).to(eng.device), torch.from_numpy(band).to(eng.device)
        y, y32 = eng.bpf2(f, b)
        p = eng.pick_exact(eng.xcorr32(y32, b), y, b)
        outs.append((r.cand_metric.cpu(), r.cand_info.cpu(), p[0].cpu(), p[1].cpu()))
    for u, v in zip(*outs):
        assert torch.equal(u, v)


def test_slab_guard_orders_geometries_across_streams():
    """One context, two streams, list-decoder launches of DIFFERENT slot geometry back to back (64-lane blocks of the short lists, 128-lane
    blocks of a 128-path list, the several-frames-per-wave kernel on the other slab): es_slab_enter / es_slab_leave order them on the device
    (hipStreamWaitEvent, no host wait), so every launch must return what it returns alone.  Without the guard the second launch carves the
    slab into other slots while the first is still using it."""
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=128)
    rng = np.random.default_rng(31)
    big = torch.from_numpy(np.clip(rng.normal(0, 3, (16384, 1024)), -12, 12).astype(np.float32)).to(eng.device)
    small = big[:96].contiguous()
    eng.set_option("scl_multi", 1); eng.set_option("scl_lanes", 1)
    ref8 = eng.scl(big, list_size=8, skip_if_hard_ok=False)
    ref128 = eng.scl(small, list_size=128, skip_if_hard_ok=False)
    eng.set_option("scl_lanes", 4)
    ref_m = eng.scl(big[:4096].contiguous(), list_size=8, skip_if_hard_ok=False)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(eng.device), torch.cuda.Stream(eng.device)
    for _ in range(3):
        eng.set_option("scl_lanes", 1)
        with torch.cuda.stream(sa):
            a = eng.scl(big, list_size=8, skip_if_hard_ok=False)            # ~5 ms of 64-lane blocks on the lane-per-path slab
        with torch.cuda.stream(sb):
            b = eng.scl(small, list_size=128, skip_if_hard_ok=False)        # 128-lane blocks on the same slab, another stream, at once
        with torch.cuda.stream(sa):
            c = eng.scl(big, list_size=8, skip_if_hard_ok=False)            # and back
        eng.set_option("scl_lanes", 4)
        with torch.cuda.stream(sb):
            m = eng.scl(big[:4096].contiguous(), list_size=8, skip_if_hard_ok=False)
        torch.cuda.synchronize()
        for got, want in ((a, ref8), (b, ref128), (c, ref8), (m, ref_m)):
            assert torch.equal(got.cand_info, want.cand_info) and torch.equal(got.cand_metric, want.cand_metric) and torch.equal(got.ncand, want.ncand)
    eng.set_option("scl_multi", -1); eng.set_option("scl_lanes", 0)


def test_captured_list_decode_keeps_its_frame_counter():
    """A list-decoder launch with skip_if_hard_ok draws its frames from a per-launch counter.  Recorded into a stream capture it takes one of
    the context's reserved counters for good (es_cursor_next), so a replay of the graph BESIDE eager launches of the same context -- which
    rotate over the other counters -- decodes exactly what the eager launch decodes.  (Round 3 handed every launch the next counter of one
    ring: a replay could meet an eager launch on the same counter.)"""
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=8)
    eng.set_option("scl_multi", 1); eng.set_option("scl_lanes", 1)          # the lane-per-path kernel: the one that draws frames
    rng = np.random.default_rng(77)
    info = torch.from_numpy(rng.integers(0, 256, (4096, 55), dtype=np.uint8)).to(eng.device)
    code = eng.polar_encode(info).to(torch.float32)
    clean = (2.0 * code - 1.0) * 6.0
    noisy = torch.from_numpy(np.clip(rng.normal(0, 3, (4096, 1024)), -12, 12).astype(np.float32)).to(eng.device)
    mix = torch.where(torch.from_numpy(rng.random(4096) < 0.5).to(eng.device)[:, None], noisy, clean).contiguous()   # half the frames pass the hard decision
    ref = eng.scl(mix, list_size=8, skip_if_hard_ok=True)
    other = eng.scl(noisy, list_size=8, skip_if_hard_ok=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(eng.device)
    with torch.cuda.stream(s):
        eng.scl(mix, list_size=8, skip_if_hard_ok=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.scl(mix, list_size=8, skip_if_hard_ok=True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(eng.device)
    for _ in range(4):
        g.replay()
        with torch.cuda.stream(side):                                        # eager launches of the same context beside the replay
            for _ in range(3):
                o2 = eng.scl(noisy, list_size=8, skip_if_hard_ok=True)
        torch.cuda.synchronize()
        assert torch.equal(out.ncand, ref.ncand) and torch.equal(out.cand_info, ref.cand_info) and torch.equal(out.cand_metric, ref.cand_metric)
        assert torch.equal(o2.cand_info, other.cand_info) and torch.equal(o2.ncand, other.ncand)
    assert int((ref.ncand == 0).sum()) > 1000 and int((ref.ncand == 8).sum()) > 1000
    eng.set_option("scl_multi", -1); eng.set_option("scl_lanes", 0)
