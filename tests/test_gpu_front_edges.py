"""The demodulator (es_llr_batch) and the header decoder (es_header_batch) against the CPU oracle, bit for bit, at their edges.

WatermarkDetector.verify() demodulates every candidate with both PN variants and tries the counters the header decoder picks, so
a subtle error in either kernel changes what the detector decodes.  These tests compare every output -- LLRs, chosen shift and
both scores of the demodulator; ok, value, score and chosen shift of the header -- with oracle.llr / oracle.decode_header:

  * test_every_payload_length: at five rates (both builds: 160-tap capacity at 58 500 Hz, the 576-tap build with its smallest
    filter at 58 870 Hz and at capacity at 211 790 Hz, plus 48 000 and 44 100), every payload length 1 .. 1 024 in all four
    bands, both variants, real frames cut by the window's end at several SNRs; the zero-output starts (no payload, start at or
    past the end, negative start); the header's length boundary, with its PN as one broadcast row and as per-record rows;
  * test_degenerate_content: silence, constants, spikes, periodic rows, alternation, 1e15 and 1e-20 amplitudes, noise;
  * test_*_device_filling: launches of at least three times each kernel's grid cap (computed from the device's CU count) of
    distinct config-3 records at their first and second detected peaks, so that every block runs its grid-stride loop;
  * test_sync_at_new_rates: the float64 and the fused sync paths at the rates whose band-pass designs no other test uses.

The oracle runs on a thread pool (oracle.map_records); workers compare and return only mismatch descriptors
(record, field, first differing index)."""
from collections import Counter

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.crypto import SecureChannel
from echoseal_amd.tables import pack_tables

KEY = b"\xAA" * 32
T = 2048
RATES = (48_000, 58_500, 58_870, 44_100, 211_790)
BUILD = {48_000: 160, 58_500: 160, 58_870: 576, 44_100: 576, 211_790: 576}     # the instantiation each rate's longest filter selects


def _report(mism, what):
    if mism:
        by = Counter(f for _, f, _ in mism)
        recs = sorted({r for r, _, _ in mism}, key=str)
        raise AssertionError(f"{what}: {len(mism)} mismatches in {len(recs)} records; by field {dict(by)}; "
                             f"first records {recs[:12]}; first descriptors {mism[:12]}")


def _engine(fs):
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, fs=fs, list_size_max=0)
    assert (int(eng._tables[3].max()) <= 160) == (BUILD[fs] == 160)
    return eng


def _cmp_llr(oracle, tabs, Y, rows, S, Bd, P, variant, L, BS, SC):
    """Worker for map_records: record i is row Y[rows[i]] demodulated from start S[i] in band Bd[i] with packed PN row P[i]."""
    _, _, taps, ntaps, _ = tabs
    sl = slice(191, 1215) if variant == 0 else slice(0, 1024)

    def cmp(lo, hi):
        out = []
        for i in range(lo, hi):
            st = int(S[i])
            if st < 0:                                          # no oracle frame for a negative start: the kernel defines zeros
                want, ws, w0, w1 = np.zeros(1024, np.float32), 0, -1.0, -1.0
            else:
                b = int(Bd[i])
                want, ws, w0, w1 = oracle.llr(Y[rows[i], st:st + 1215], np.unpackbits(P[i])[sl], taps[b, :ntaps[b]])
            d = oracle.first_diff(want, L[i])
            if d is not None:
                out.append((i, "llr", d))
            if int(BS[i]) != ws:
                out.append((i, "best_s", int(BS[i])))
            d = oracle.first_diff(np.array([w0, w1], np.float32), SC[i])
            if d is not None:
                out.append((i, "score", d))
        return out
    return cmp


def _cmp_header(oracle, tabs, Y, rows, S, Bd, H, OK, VAL, SCORE, BS):
    """Worker for map_records; H: packed header PN rows [n,16], or one row that every record shares."""
    _, _, taps, ntaps, _ = tabs

    def cmp(lo, hi):
        out = []
        for i in range(lo, hi):
            st = int(S[i])
            if st < 0:
                ok, val, score, ws = False, 0, 0.0, 0
            else:
                b = int(Bd[i])
                ok, val, score, ws = oracle.decode_header(Y[rows[i], st:], np.unpackbits(H[i if H.shape[0] > 1 else 0])[:128],
                                                          taps[b, :ntaps[b]])
            if int(OK[i]) != int(ok):
                out.append((i, "ok", int(OK[i])))
            if int(VAL[i]) != val:
                out.append((i, "val", int(VAL[i])))
            if oracle.first_diff(np.float32(score), SCORE[i]) is not None:
                out.append((i, "score", float(SCORE[i])))
            if int(BS[i]) != ws:
                out.append((i, "best_s", int(BS[i])))
        return out
    return cmp


def _run_llr(eng, y, band, pn, start, variant):
    l, bs, sc = eng.llr(y, band, pn, start=start, variant=variant, want_diag=True)
    torch.cuda.synchronize()
    return l.cpu().numpy(), bs.cpu().numpy(), sc.cpu().numpy()


def _run_header(eng, y, band, hdr, start):
    r = eng.header(y, band, hdr, start=start, want_diag=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in r]


@pytest.fixture(scope="module")
def frames(engine):
    """Device-made frames with their schedule (48 kHz chips: at the other rates the samples are what they are) -> host arrays."""
    n = 6144
    fr, _ = engine.synthetic_frames(KEY, 0, n)
    pn, band = engine.schedule(SecureChannel(KEY)._prng.sub_key, KEY, ctr0=0, n=n)
    torch.cuda.synchronize()
    return fr.cpu().numpy(), pn.cpu().numpy(), band.cpu().numpy()


def _length_rows(frames, seed):
    """Windows of T samples whose frame is cut by the window's end: start st = T - 191 - npl for every npl 1 .. 1 024 in every band
    (so that min(T - st, 1215) - 191 = npl), then the zero-output and header-boundary starts.  -> (win, start, band, pn)."""
    fr, pn, band = frames
    rng = np.random.default_rng(seed)
    edge = [T - 189, T - 190, T - 191, T - 192, T, T + 7, -1, -300]         # header cut-off at T - st = 191; llr npl = -1, 0
    W, S, Bd, Pn = [], [], [], []
    for b in range(4):
        ctrs = np.flatnonzero(band == b)
        assert ctrs.size >= 1024 + len(edge)
        for k, st in enumerate([T - 191 - npl for npl in range(1, 1025)] + edge):
            c = ctrs[k]
            o = min(max(st, 0), T - 1)
            w = np.zeros(T, np.float32)
            seg = fr[c][:T - o]
            w[o:o + seg.size] = seg
            snr_db = (-6.0, 0.0, 6.0, 20.0)[k % 4]
            rms = float(np.sqrt(np.mean(fr[c].astype(np.float64) ** 2)))
            w += (rng.standard_normal(T) * rms * 10 ** (-snr_db / 20)).astype(np.float32)
            W.append(w); S.append(st); Bd.append(b); Pn.append(pn[c])
    return np.stack(W), np.array(S, np.int32), np.array(Bd, np.uint8), np.stack(Pn)


@pytest.mark.parametrize("fs", RATES)
def test_every_payload_length(oracle, frames, fs):
    eng = _engine(fs)
    dev = eng.device
    tabs = pack_tables(fs)
    W, S, Bd, P = _length_rows(frames, seed=fs)
    n = W.shape[0]
    npl = np.minimum(T - S, 1215) - 191
    assert all(set(range(1, 1025)) <= set(npl[(Bd == b) & (S >= 0)].tolist()) for b in range(4))
    wd, bd, pd, sd = (torch.from_numpy(a).to(dev) for a in (W, Bd, P, S))
    y = eng.bpf(wd, bd)
    Y = y.cpu().numpy()
    rows = np.arange(n)
    zero = (npl <= 0) | (S < 0)                                  # the kernel's zero outputs, asserted directly as well
    assert set(npl[S >= 0][npl[S >= 0] <= 0].tolist()) >= {-1, 0} and (S == T).any() and (S > T).any() and (S < 0).any()
    for variant in (0, 1):
        L, BS, SC = _run_llr(eng, y, bd, pd, sd, variant)
        assert not L[zero].any() and not BS[zero].any() and (SC[zero] == -1.0).all()
        _report(oracle.map_records(_cmp_llr(oracle, tabs, Y, rows, S, Bd, P, variant, L, BS, SC), n),
                f"llr fs={fs} variant {variant}")
    rng = np.random.default_rng(fs + 1)
    hdr_one = np.packbits(SecureChannel(KEY).pn_bits(0, 128))[None, :]
    hdr_rows = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    cut = (S < 0) | (T - S < 191)
    assert set((T - S).tolist()) >= {189, 190, 191, 192}
    for H in (hdr_one, hdr_rows):
        OK, VAL, SCORE, HBS = _run_header(eng, y, bd, torch.from_numpy(H).to(dev), sd)
        assert not OK[cut].any() and not VAL[cut].any() and not SCORE[cut].any() and not HBS[cut].any()
        _report(oracle.map_records(_cmp_header(oracle, tabs, Y, rows, S, Bd, H, OK, VAL, SCORE, HBS), n),
                f"header fs={fs} hdr_pn rows {H.shape[0]}")
    assert len(eng.header(y[:2], bd[:2], torch.from_numpy(hdr_one).to(dev), start=sd[:2])) == 3     # no want_diag: as before
    eng.close()


def _degenerate_rows():
    """(name, builder(st, npl, rng) -> float64 [T]): rows the kernels see directly (no band-pass)."""
    t = np.arange(T)
    return [
        ("silence", lambda st, npl, r: np.zeros(T)),
        ("constant", lambda st, npl, r: np.full(T, 0.25)),
        ("negative_constant", lambda st, npl, r: np.full(T, -3.0)),
        ("spike_payload", lambda st, npl, r: np.where(t - st == 191 + npl // 2, 1.0, 0.0)),
        ("spike_header", lambda st, npl, r: np.where(t - st == 120, 1.0, 0.0)),
        ("period7", lambda st, npl, r: np.sin(2 * np.pi * t / 7.0)),
        ("period64", lambda st, npl, r: ((t % 64) < 32) - 0.5),
        ("period3", lambda st, npl, r: (t % 3) - 1.0),
        ("alternating", lambda st, npl, r: np.where(t % 2 == 0, 0.5, -0.5)),
        ("noise_1e15", lambda st, npl, r: 1e15 * r.standard_normal(T)),
        ("noise_1e-20", lambda st, npl, r: 1e-20 * r.standard_normal(T)),
        ("noise", lambda st, npl, r: r.standard_normal(T)),
    ]


@pytest.mark.parametrize("fs", RATES)
def test_degenerate_content(oracle, fs):
    """Rows where every shift ties (the first maximum must win), rows periodic within the shift range, extreme amplitudes:
    full frames and payloads of 1 .. 513 samples (201 .. 255: odd lengths whose half is above the filter memory, where the shift
    range is n // 2), the rows spread over the four bands, both kernels."""
    eng = _engine(fs)
    dev = eng.device
    tabs = pack_tables(fs)
    rng = np.random.default_rng(fs)
    Y, S, Bd, NM = [], [], [], []
    for k, (name, mk) in enumerate(_degenerate_rows()):
        for j, npl in enumerate((1024, 1, 2, 9, 10, 64, 201, 233, 255, 513)):
            st = 0 if npl == 1024 else T - 191 - npl
            Y.append(mk(st, npl, rng).astype(np.float32).astype(np.float64))
            S.append(st); Bd.append((k + j) % 4); NM.append(name)
    Y = np.stack(Y); S = np.array(S, np.int32); Bd = np.array(Bd, np.uint8)
    n = Y.shape[0]
    P = rng.integers(0, 256, (n, 152), dtype=np.uint8)
    H = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    y, bd, pd, sd, hd = (torch.from_numpy(a).to(dev) for a in (Y, Bd, P, S, H))
    rows = np.arange(n)
    for variant in (0, 1):
        L, BS, SC = _run_llr(eng, y, bd, pd, sd, variant)
        mism = oracle.map_records(_cmp_llr(oracle, tabs, Y, rows, S, Bd, P, variant, L, BS, SC), n, chunk=8)
        _report([(f"{i}:{NM[i]}", f, d) for i, f, d in mism], f"llr fs={fs} variant {variant}")
    OK, VAL, SCORE, HBS = _run_header(eng, y, bd, hd, sd)
    mism = oracle.map_records(_cmp_header(oracle, tabs, Y, rows, S, Bd, H, OK, VAL, SCORE, HBS), n, chunk=8)
    _report([(f"{i}:{NM[i]}", f, d) for i, f, d in mism], f"header fs={fs}")
    eng.close()


@pytest.fixture(scope="module")
def c3_records(engine):
    """Config-3 windows made on the device (workloads.c3_windows_device): two per demodulator block of the grid cap (num_cu x 64
    one-wave blocks; the header's cap, num_cu x 32, is half of it), so that records at the first and second detected peak of
    every window give four times the demodulator's cap."""
    from echoseal_amd import workloads as WL
    cu = torch.cuda.get_device_properties(engine.device).multi_processor_count
    n_win = 2 * cu * 64
    pn, band = engine.schedule(SecureChannel(KEY)._prng.sub_key, KEY, ctr0=0, n=n_win)
    clean = torch.cat([engine.synthetic_frames(KEY, c0, min(8192, n_win - c0))[0] for c0 in range(0, n_win, 8192)])
    win, _ = WL.c3_windows_device(clean, seed=35)
    del clean
    torch.cuda.synchronize()
    return dict(cu=cu, win=win, pn=pn, band=band, n_win=n_win)


def _device_filling_inputs(eng, c3, cap):
    """Band-pass and sync at the engine's rate; records = (window, first peak), then (window, second peak, else the first)."""
    sy = eng.sync_fast(c3["win"], c3["band"])
    p0 = sy.peaks[:, 0]
    p1 = torch.where(sy.peaks[:, 1] >= 0, sy.peaks[:, 1], p0)
    start = torch.cat([p0, p1]).contiguous()
    y2 = torch.cat([sy.y, sy.y]).contiguous()
    band2 = torch.cat([c3["band"], c3["band"]]).contiguous()
    pn2 = torch.cat([c3["pn"], c3["pn"]]).contiguous()
    torch.cuda.synchronize()
    Y = sy.y.cpu().numpy()
    del sy
    nw = c3["n_win"]
    rows = np.concatenate([np.arange(nw), np.arange(nw)])
    S, Bd, P = start.cpu().numpy(), band2.cpu().numpy(), pn2.cpu().numpy()
    distinct = np.unique(rows.astype(np.int64) * 4096 + S).size
    assert (S >= 0).all() and distinct >= 3 * cap, (distinct, cap)
    assert (np.minimum(T - S, 1215) - 191 < 1024).any()            # some frames are cut by the window's end
    return y2, band2, pn2, start, Y, rows, S, Bd, P


def _llr_device_filling(oracle, c3, fs, variants):
    eng = _engine(fs)
    tabs = pack_tables(fs)
    y2, band2, pn2, start, Y, rows, S, Bd, P = _device_filling_inputs(eng, c3, c3["cu"] * 64)
    for variant in variants:
        L, BS, SC = _run_llr(eng, y2, band2, pn2, start, variant)
        _report(oracle.map_records(_cmp_llr(oracle, tabs, Y, rows, S, Bd, P, variant, L, BS, SC), rows.size, chunk=256),
                f"llr device-filling fs={fs} variant {variant}")
        del L, BS, SC
    del y2
    eng.close()


def test_llr_device_filling_small_build_variant1(oracle, c3_records):
    """Variant 1 of the 160-tap build at 48 000 Hz (variant 0's grid-stride path is what the headline tests cover)."""
    _llr_device_filling(oracle, c3_records, 48_000, (1,))


def test_llr_device_filling_large_build(oracle, c3_records):
    """Both variants of the 576-tap build at capacity (211 790 Hz)."""
    _llr_device_filling(oracle, c3_records, 211_790, (0, 1))


@pytest.mark.parametrize("fs", [48_000, 211_790])
def test_header_device_filling(oracle, c3_records, fs):
    """The header decoder in both builds, on at least three times its grid cap (num_cu x 32 blocks) of distinct records."""
    eng = _engine(fs)
    tabs = pack_tables(fs)
    y2, band2, pn2, start, Y, rows, S, Bd, P = _device_filling_inputs(eng, c3_records, c3_records["cu"] * 32)
    H = np.packbits(SecureChannel(KEY).pn_bits(0, 128))[None, :]
    OK, VAL, SCORE, HBS = _run_header(eng, y2, band2, torch.from_numpy(H).to(eng.device), start)
    _report(oracle.map_records(_cmp_header(oracle, tabs, Y, rows, S, Bd, H, OK, VAL, SCORE, HBS), rows.size, chunk=256),
            f"header device-filling fs={fs}")
    del y2
    eng.close()


@pytest.mark.parametrize("fs", [58_500, 58_870, 211_790])
def test_sync_at_new_rates(oracle, c3_records, fs):
    """The float64 sync path (bpf -> xcorr -> pick) and the fused one (bpf2 -> sync_fused) against oracle.lfilter / ncc /
    cfar_threshold / pick_peaks on 48 config-3 windows, at the rates whose band-pass designs no other test uses."""
    eng = _engine(fs)
    ba, tpl, _, _, _ = pack_tables(fs)
    win, band = c3_records["win"][:48].contiguous(), c3_records["band"][:48].contiguous()
    sy = eng.sync(win, band)
    sf = eng.sync_fast(win, band)
    torch.cuda.synchronize()
    X, Bd = win.cpu().numpy(), band.cpu().numpy()
    got = {k: v.cpu().numpy() for k, v in dict(y=sy.y, corr=sy.corr, thr=sy.thr, pk=sy.peaks, npk=sy.npeaks, fy=sf.y,
                                                fthr=sf.thr, fpk=sf.peaks, fnpk=sf.npeaks).items()}
    mism = []
    for i in range(48):
        b = int(Bd[i])
        y = oracle.lfilter(ba[b, :9], ba[b, 9:], X[i])
        corr = oracle.ncc(y, tpl[b])
        thr, _, _ = oracle.cfar_threshold(corr)
        peaks, tot, fb = oracle.pick_peaks(corr, thr)
        for field, want, g in (("y", y, got["y"][i]), ("corr", corr, got["corr"][i]), ("thr", np.float64(thr), got["thr"][i]),
                               ("fused y", y, got["fy"][i]), ("fused thr", np.float64(thr), got["fthr"][i])):
            d = oracle.first_diff(want, g)
            if d is not None:
                mism.append((i, field, d))
        for pre, npk, pk in (("", got["npk"][i], got["pk"][i]), ("fused ", got["fnpk"][i], got["fpk"][i])):
            k = int(npk) & 0xFFFF
            if k != min(tot, 32) or bool((int(npk) >> 30) & 1) != fb or list(pk[:k]) != list(peaks[:k]):
                mism.append((i, pre + "peaks", k))
    _report(mism, f"sync fs={fs}")
    eng.close()
