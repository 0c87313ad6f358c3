"""GPU: decisions inside the kernels that the mutant audit (tests/mutants.py) found no test standing on.

Each test builds an input that sits on one comparison, constant or mask of a kernel, first shows on the CPU that it does (the value in
question restated in NumPy and tied to an output of the oracle or the host twin), then compares the kernel with that reference, bit for
bit.  The kernels and the boundaries:

  * es_header_kernel: margin == 0.5 exactly (`margin > 0.5f`), and a filter short enough for the floor of the guard to decide the shift
    (`guard < 8`): both under band tables of the test's own, a one-tap and a 40-tap matched filter, which the shipped designs never have;
  * plan_row: a header's low half above 0x7FFF (`(c & 0xFFFF) == lo16`), and the last 32-bit counter in the narrow window of the form
    with origins (`c <= 0xFFFFFFFF`);
  * es_acquire_mask_kernel: a record whose counter is the span's end itself (`c < ctr_hi`), next to one on the span's start;
  * validate_blob: a counter that differs from the sealed one in a single bit, every bit of the four bytes (`be_ctr == ctr`);
  * es_tx_finish_kernel: a peak of exactly 3.0 (`peak > 3.0`), under a pure gain in place of the band-pass."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd._native import ES_MAX_PEAKS
from echoseal_amd.identify import plan_reference
from echoseal_amd.scan import CTR_END, counter_estimate
from echoseal_amd.utils import band_index

FL = 1215
KEYS = [b"\xAA" * 32, b"\x5C" * 32, bytes(range(32))]


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


# ------------------------------------------------------------------------------------------------------------------- header decoder
@pytest.fixture(scope="module")
def short_filters(engine):
    """A front-end engine whose band 0 has the one-tap matched filter [1.0] and band 1 a 40-tap one -> (engine, taps of band 0, of band 1)."""
    from echoseal_amd.engine import RxEngine
    front = RxEngine(engine.device, list_size_max=0)
    ba, tpl, taps, ntaps, frozen = front.tables()
    taps, ntaps = taps.copy(), ntaps.copy()
    h40 = (np.random.default_rng(2024).standard_normal(40) * np.hanning(40)).astype(np.float32)
    taps[0] = 0.0; taps[0, 0] = 1.0; ntaps[0] = 1
    taps[1] = 0.0; taps[1, :40] = h40; ntaps[1] = 40
    front.set_tables(ba, tpl, taps, ntaps, frozen)
    yield front, taps[0, :1].copy(), h40
    torch.cuda.synchronize()
    front.close()


def _header(front, frames, band, pn_bits):
    n = len(frames)
    r = front.header(_dev(front, np.stack(frames)), _dev(front, np.full(n, band, np.uint8)), _dev(front, np.packbits(np.stack(pn_bits), axis=1)),
                     want_diag=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in r]


def _same_header(oracle, got, frames, pn_bits, taps):
    ok, val, score, best_s = got
    want = [oracle.decode_header(f, p, taps) for f, p in zip(frames, pn_bits)]
    for i, (wok, wval, wscore, ws) in enumerate(want):
        assert (int(ok[i]), int(val[i]), int(best_s[i])) == (int(wok), wval, ws) and oracle.first_diff(np.float32(wscore), score[i]) is None, \
            (i, int(ok[i]), int(val[i]), float(score[i]), int(best_s[i]), want[i])
    return want


def test_header_margin_of_exactly_one_half(oracle, short_filters):
    """Under the one-tap filter the despread header is the frame's own samples times the PN, so its 128 values can be chosen: 16 groups of
    (-8, -5, 2, 2, 2, 3, 3, 3) have group sums of +-2 and a mean square of 16, margin = mean|sum| / rms = 2 / 4 = 0.5 exactly, which is
    not `> 0.5`; with one value of one group raised by 1 the margin is above it.  Twelve sums are positive, so the margin alone decides."""
    front, delta, _ = short_filters
    group = np.array([-8, -5, 2, 2, 2, 3, 3, 3], np.float32)
    bits = np.array([1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])     # a 1 is a negative group sum
    rng = np.random.default_rng(11)
    frames, pns, margins = [], [], []
    for bump in (0.0, 1.0, -1.0):
        for perm in range(4):
            d = np.concatenate([(-1.0 if b else 1.0) * rng.permutation(group) for b in bits]).astype(np.float32)
            d[7 * 8 + 3] += np.float32(bump)                                # group 7 sums to +2: 3 or 1 with the bump
            pn = rng.integers(0, 2, 128).astype(np.uint8)
            f = np.zeros(FL)
            f[63:191] = d * (2.0 * pn - 1.0)
            frames.append(f); pns.append(pn)
            sums = d.reshape(16, 8).sum(axis=1, dtype=np.float32)
            rms = np.sqrt(np.float32(np.sum(d * d, dtype=np.float32) / np.float32(128))) + np.float32(1e-12)
            margins.append((np.float32(np.abs(sums).sum(dtype=np.float32) / np.float32(16)) / rms, int((sums > 0).sum())))
    # the boundary, on the CPU: integers, so every float32 sum is exact whatever its order
    assert all(m == np.float32(0.5) and npos == 12 for m, npos in margins[:4])
    assert all(m > np.float32(0.5) and npos == 12 for m, npos in margins[4:8]) and all(m < np.float32(0.5) for m, _ in margins[8:])
    want = _same_header(oracle, _header(front, frames, 0, pns), frames, pns, delta)
    assert [w[0] for w in want] == [False] * 4 + [True] * 4 + [False] * 4 and all(w[1] == 0x9088 and w[3] == 0 for w in want)


def test_header_guard_floor_decides_the_shift(oracle, short_filters):
    """A 40-tap filter has ntaps / 8 = 5, below the floor of 8 the guard is raised to.  The shift search is restated here for any guard
    (NumPy's float32 sums are the reference's own): with guard 8 it picks the oracle's shift on all 64 noise frames, and with guard 9 it
    picks another shift on several of them, by a clear margin."""
    front, _, h = short_filters
    assert len(h) // 8 < 8

    def search(frame, pn, guard):
        ntaps = len(h); mem = ntaps - 1; prefix = min(mem, 63); nfull = prefix + 128
        mf = np.convolve(frame[63 - prefix:63 - prefix + nfull].astype(np.float32).astype(np.float64), h.astype(np.float64))
        offset = mem + prefix
        ms = max(min(64 + prefix, 4 * ntaps), mem)
        wstart = max(offset - ms, 0)
        win = mf[wstart:min(len(mf), offset + 128 + ms)].astype(np.float32)
        sym = (2.0 * pn - 1.0).astype(np.float32)
        score = {s: abs(np.sum(win[offset - wstart + s + guard:offset - wstart + s + 128] * sym[guard:]))
                 for s in range(-ms, ms + 1) if 0 <= offset - wstart + s and offset - wstart + s + 128 <= len(win)}
        best = max(score.values())
        return min(s for s, v in score.items() if v == best), score

    rng = np.random.default_rng(2024)
    rng.standard_normal(40)                                                 # (the filter's draws)
    frames, pns = [], []
    for _ in range(64):
        frames.append(rng.standard_normal(FL))
        pns.append(rng.integers(0, 2, 128).astype(np.uint8))
    moved = 0                                                               # the boundary, on the CPU, before any launch
    for f, p in zip(frames, pns):
        s8, _ = search(f, p, 8)
        s9, sc9 = search(f, p, 9)
        assert s8 == oracle.decode_header(f, p, h)[3]                       # the restatement is the oracle's search
        moved += s9 != s8 and sc9[s9] - sc9[s8] > 0.1
    assert moved >= 5, moved
    _same_header(oracle, _header(front, frames, 1, pns), frames, pns, h)


# ------------------------------------------------------------------------------------------------------------------- planner
def _peak_rows(peaks_of_rows):
    """-> (peaks int32 [rows, 32], npeaks, hdr_base) of rows whose every peak fits."""
    rows = len(peaks_of_rows)
    peaks = np.full((rows, ES_MAX_PEAKS), -1, np.int32)
    npeaks = np.zeros(rows, np.int32)
    for r, p in enumerate(peaks_of_rows):
        peaks[r, :len(p)] = p; npeaks[r] = len(p)
    nfit = np.array([len(p) for p in peaks_of_rows])
    return peaks, npeaks, (np.cumsum(nfit) - nfit).astype(np.int32)


def _plan_rows(engine, peaks, npeaks, base, M, rowband, hok, hlo, hop, **at):
    res = engine.plan(_dev(engine, peaks), _dev(engine, npeaks), np.asarray(rowband, np.uint8), base, M, _dev(engine, hok), _dev(engine, hlo),
                      _dev(engine, hop), **at)
    torch.cuda.synchronize()
    slot, ctr = res.slot.cpu().numpy(), res.ctr.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    count, looked = res.count.cpu().numpy(), res.looked.cpu().numpy()
    return [(list(zip(slot[p, :count[p]].tolist(), ctr[p, :count[p]].tolist())), int(looked[p])) for p in range(len(count))]


def test_plan_header_gate_above_0x7fff(engine):
    """Peaks at counters 32 800, 32 900 and 100 of a 40 M-sample row, each with a decoded header.  The first states the low half 32 800,
    which has bit 15 set; the second states 132 = 32 900 - 32 768, a low half that only a 15-bit comparison finds in its window."""
    ests = [100, 32_800, 32_900]
    M = 33_100 * FL
    C = -(-M // FL) + 201
    hop = np.full((1, C), 2, np.uint8)                                       # every counter hops to the row's band
    hok = np.ones((1, 3), np.uint8)
    hlo = np.array([[100, 32_800, 132]], np.int32)
    peaks, npeaks, base = _peak_rows([[e * FL for e in ests]])
    want, looked = plan_reference(peaks[0], npeaks[0], M, 2, hok[0], hlo[0], hop[0])
    assert want == [(0, 100), (1, 32_800)] and looked == 3                  # the boundary: a gated counter >= 0x8000 found, 32 900 not taken for 132
    assert (32_900 & 0x7FFF) == 132 and all((c & 0xFFFF) != 132 for c in range(32_700, 33_101))
    assert _plan_rows(engine, peaks, npeaks, base, M, [2], hok, hlo, hop) == [(want, looked)]


def test_plan_at_last_counter_in_the_narrow_window(engine):
    """A stream whose frame 0 carries counter 2^32 - 3: without a header, the windows est - 3 .. est + 3 of its first three peaks end at the
    last counter 2^32 - 1, which is a candidate, and not beyond."""
    ctr0, pos0 = CTR_END - 3, 0
    T = 3 * FL + 3
    starts = [0, FL, 2 * FL]
    C = -(-T // FL) + 402
    hbase = counter_estimate(0, pos0, ctr0) - 200
    hop = np.full((1, 1, C), 1, np.uint8)
    hok = np.zeros((1, 3), np.uint8)
    hlo = np.zeros((1, 3), np.int32)
    peaks, npeaks, base = _peak_rows([starts])
    want, looked = plan_reference(peaks[0], npeaks[0], T, 1, hok[0], hlo[0], hop[0, 0], pos0=pos0, ctr0=ctr0, hop_base=hbase)
    assert [counter_estimate(s, pos0, ctr0) for s in starts] == [CTR_END - 3, CTR_END - 2, CTR_END - 1]
    for s in range(3):                                                      # the boundary: each narrow window ends at 2^32 - 1 exactly
        mine = [c for sl, c in want if sl == s]
        assert mine == list(range(CTR_END - 6 + s, CTR_END)) and len(mine) <= 7
    got = _plan_rows(engine, peaks, npeaks, base, T, [1], hok, hlo, hop, pos0=np.array([pos0], np.int64), ctr0=np.array([ctr0], np.int64),
                     hop_row=np.zeros(1, np.int32), hop_base=np.array([hbase], np.int64))
    assert got == [(want, looked)]


# ------------------------------------------------------------------------------------------------------------------- acquisition
def test_acquire_span_ends(engine):
    """Records whose only candidate could be the span's first counter (inside) or its end (outside), with the band that counter hops to."""
    from echoseal_amd import acquire as A
    ring = engine.keyring(KEYS)
    for span in ((70_001, (1 << 22) + 5), (3 * 65_536 + 40_000, 20 * 65_536 + 100)):
        lo, hi = span
        key = np.array([0, 1, 2, 0, 1, 2], np.int32)
        at = [lo, lo, lo, hi, hi, hi]
        ok = np.ones(6, np.uint8)
        lo16 = np.array([c & 0xFFFF for c in at], np.int32)
        band = np.array([band_index(KEYS[k], c) for k, c in zip(key, at)], np.uint8)
        want_mask, want_count, cands = A.mask_model(KEYS, key, ok, lo16, band, span)
        # the boundary: the start is a candidate of its records, the end is none of its records' although it hops to their band
        assert all(cands[p] and cands[p][0] == lo for p in range(3)) and all(hi not in cands[p] for p in range(3, 6))
        assert all(c < hi for cs in cands for c in cs) and hi & 0xFFFF != 0
        mask, count = engine.acquire_mask(ring, key, ok, lo16, band, span)
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy().view(np.uint32), want_mask) and np.array_equal(count.cpu().numpy(), want_count)


# ------------------------------------------------------------------------------------------------------------------- validator
def test_validator_rejects_every_single_bit_of_the_counter(engine, oracle):
    """A sealed blob checked against its own counter and against that counter with one bit flipped, for each of the 32 bits: the top byte
    and the sign bit decide as the low byte does."""
    from aead_edges import KEY
    from echoseal_amd.primitives import chacha20poly1305_encrypt
    rng = np.random.default_rng(77)
    for c in (0x01020304, 0, CTR_END - 1, 0x80000000):                      # a launch of 33 records per sealed counter
        pt = b"ESAL" + c.to_bytes(4, "big") + rng.bytes(19)
        nonce = rng.bytes(12)
        blob = nonce + chacha20poly1305_encrypt(KEY, nonce, pt)
        ctrs = np.array([c] + [c ^ (1 << b) for b in range(32)], np.int64)
        blobs = np.tile(np.frombuffer(blob, np.uint8), (33, 1))
        plains = np.tile(np.frombuffer(pt, np.uint8), (33, 1))
        want_ok = (ctrs == c).astype(np.uint8)
        o_ok, o_plain = oracle.validate_blobs(KEY, blobs, ctrs)
        assert np.array_equal(o_ok, want_ok) and np.array_equal(o_plain, plains) and int(want_ok.sum()) == 1
        assert sum((int(a) ^ c) >> 24 != 0 and (int(a) ^ c) & 0xFFFFFF == 0 for a in ctrs) == 8     # the boundary: equal in the low 24 bits
        ok, plain = engine.aead_check(KEY, _dev(engine, blobs), torch.from_numpy(ctrs), want_plain=True)
        assert np.array_equal(ok.cpu().numpy(), want_ok) and np.array_equal(plain.cpu().numpy(), plains), hex(c)


# ------------------------------------------------------------------------------------------------------------------- frame generator
def test_frame_generator_peak_of_exactly_three(engine, oracle):
    """peak = max|y| + 1e-12 rescales a frame when it is above 3.0, not when it equals it (echoseal_amd/embedder.py:120-123).  With the
    band-pass numerators replaced by a pure gain g the chips are +-g: g is the double for which g + 1e-12 == 3.0, then the next one up."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.embedder import WatermarkEmbedder
    from echoseal_amd.engine import RxEngine
    key = KEYS[1]
    g_eq = 3.0 - 1e-12
    while g_eq + 1e-12 < 3.0:
        g_eq = np.nextafter(g_eq, np.inf)
    while g_eq + 1e-12 > 3.0:
        g_eq = np.nextafter(g_eq, -np.inf)
    g_up = g_eq
    while g_up + 1e-12 == 3.0:
        g_up = np.nextafter(g_up, np.inf)
    assert g_eq + 1e-12 == 3.0 and g_up + 1e-12 > 3.0 and g_eq < 3.0        # the boundary: a peak of exactly 3.0, and the first above it
    ctr = np.array([0, 1, 65_535, 65_536, 1 << 31, CTR_END - 1, 7, 8], np.int64)
    pl = np.random.default_rng(5).integers(0, 256, (len(ctr), 55), dtype=np.uint8)
    tx = WatermarkEmbedder(key)
    chips = np.stack([tx._frame_symbols(int(c), bytes(p)) for c, p in zip(ctr, pl)]).astype(np.float32)
    front = RxEngine(engine.device, list_size_max=0)
    ba, tpl, taps, ntaps, frozen = front.tables()
    try:
        for g, scaled in ((g_eq, False), (g_up, True)):
            ba2 = np.zeros_like(ba)
            ba2[:, 0] = g; ba2[:, 9] = 1.0                                  # y[n] = g * x[n] in every band
            want = []
            for i in range(len(ctr)):
                y = oracle.lfilter(ba2[0, :9], ba2[0, 9:], chips[i])
                peak = float(np.max(np.abs(y))) + 1e-12
                assert (peak > 3.0) == scaled and (scaled or peak == 3.0)
                want.append((y * (1.0 / peak) if peak > 3.0 else y).astype(np.float32))
            assert np.all(np.abs(want[0]) == np.float32(1.0 if scaled else 3.0))
            front.set_tables(ba2, tpl, taps, ntaps, frozen)
            got = front.make_frames(SecureChannel(key), key, ctr, _dev(front, pl)).cpu().numpy()
            assert got.tobytes() == np.stack(want).tobytes(), (g, np.flatnonzero((got != np.stack(want)).any(axis=1)))
    finally:
        torch.cuda.synchronize()
        front.close()
