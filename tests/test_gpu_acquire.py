"""GPU: acquisition -- es_acquire_mask_batch and es_acquire_list_batch word for word against their host twin
(echoseal_amd/acquire.py), then WatermarkDetector.acquire / acquire_batch and LiveMonitor.acquire against a host walk built from the twin,
with the real demodulator and with one that answers clean only at a frame's own counter."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import acquire as A
from echoseal_amd.detector import FRAME_LEN, WatermarkDetector
from echoseal_amd.scan import CTR_END, counter_estimate
from echoseal_amd.utils import BAND_PLAN, band_index

KEYS = [b"\xAA" * 32, b"\x5C" * 32, bytes(range(32))]
W8, CM8, LIST = 3648, 1300, 8
PUSHES = (40, 1260, 1216, 1130, 1300, 1300)                                # DESIGN 4.17's lengths: n = 40 .. 6246, the window moves twice
ORIGIN = 70_000
SPAN = (0, 1 << 20)
POISON_W, POISON_C, POISON_R = 0x5A5A5A5A, -77, -78

# (span, records): the full span for three records only (the twin is 65 536 HMACs per record); unaligned ends; first and last high half
# cut by the low half on each side; H = 33 and H = 65 (a second and a third word, a second tile); the top of the range
SPANS = [((0, CTR_END), 3), ((70_001, (1 << 22) + 5), 40), ((3 * 65_536 + 40_000, 20 * 65_536 + 100), 40), ((65_536, 34 * 65_536), 40),
         ((0, 65 * 65_536), 40), ((CTR_END - (1 << 18), CTR_END), 40)]


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _records(seed, n):
    """n header records over a ring of three keys: random key, band and low half; records 3 and 11 not ok, 5 with a key index past the
    ring, 6 with a negative one, 7 with lo16 = 0, 8 with lo16 = 65 535, 9 and 10 with low halves that are none."""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 3, n).astype(np.int32)
    ok = np.ones(n, np.uint8)
    lo16 = rng.integers(0, 65_536, n).astype(np.int32)
    band = rng.integers(0, 4, n).astype(np.uint8)
    if n > 11:
        ok[[3, 11]] = 0
        key[5], key[6] = 3, -1
        lo16[7], lo16[8], lo16[9], lo16[10] = 0, 65_535, 65_536, -1
        ok[12] = 2                                                          # any non-zero byte is ok
    return key, ok, lo16, band


def _raw_mask(engine, kr, records, span, mask_t, count_t, **over):
    """One direct call of the C entry point into the caller's output tensors -> its return code; over: arguments replaced by name."""
    a = dict(ring=kr.ring, N=kr.n, key=_dev(engine, records[0]), ok=_dev(engine, records[1]), lo16=_dev(engine, records[2]),
             band=_dev(engine, records[3]), P=len(records[0]), lo=span[0], hi=span[1], mask=mask_t, count=count_t)
    a.update(over)
    p = lambda t: None if t is None else t.data_ptr()
    rc = engine._lib.es_acquire_mask_batch(engine._ctx, p(a["ring"]), a["N"], p(a["key"]), p(a["ok"]), p(a["lo16"]), p(a["band"]), a["P"], a["lo"],
                                           a["hi"], p(a["mask"]), p(a["count"]), engine._stream())
    torch.cuda.synchronize()
    return rc


def _raw_list(engine, mask_t, lo16_h, n, span, base_h, n_out, rec_t, ctr_t, **over):
    a = dict(mask=mask_t, lo16=_dev(engine, lo16_h), P=n, lo=span[0], hi=span[1], base=_dev(engine, np.asarray(base_h, np.int64)), total=n_out,
             rec=rec_t, ctr=ctr_t)
    a.update(over)
    p = lambda t: None if t is None else t.data_ptr()
    rc = engine._lib.es_acquire_list_batch(engine._ctx, p(a["mask"]), p(a["lo16"]), a["P"], a["lo"], a["hi"], p(a["base"]), a["total"], p(a["rec"]),
                                           p(a["ctr"]), engine._stream())
    torch.cuda.synchronize()
    return rc


def _poison(engine, shape, value):
    return torch.full(shape, value, dtype=torch.int32, device=engine.device)


@pytest.fixture(scope="module")
def ring(engine):
    return engine.keyring(KEYS)


@pytest.mark.parametrize("span, n", SPANS, ids=["full", "unaligned", "cut-ends", "H33", "H65", "top"])
def test_mask_and_list_equal_the_twin(engine, ring, span, n):
    rec = _records(1000 + n + span[0] % 997, n)
    key, ok, lo16, band = rec
    h0, H, W = A.span_words(span)
    want_mask, want_count, cands = A.mask_model(KEYS, key, ok, lo16, band, span)
    assert int(want_count.sum()) > 0                                        # the case does enumerate something
    if n > 11:
        assert not want_count[[3, 5, 6, 9, 10, 11]].any()
    if span[0] == 3 * 65_536 + 40_000:                                      # both ends cut by the low half, for some record each
        assert any(cs and cs[0] >> 16 == h0 for cs in cands) and any(lo16[p] < 40_000 and ok[p] for p in range(n))
        assert all(cs[0] >> 16 > h0 for p, cs in enumerate(cands) if cs and lo16[p] < 40_000)
        assert all(cs[-1] >> 16 < h0 + H - 1 for p, cs in enumerate(cands) if cs and lo16[p] >= 100)
    # the mask: every word of every row written, the row after the last untouched
    mask, count = _poison(engine, (n + 1, W), POISON_W), _poison(engine, (n + 1,), POISON_C)
    assert _raw_mask(engine, ring, rec, span, mask, count) == 0
    got_mask, got_count = mask.cpu().numpy().view(np.uint32), count.cpu().numpy()
    assert np.array_equal(got_mask[:n], want_mask) and np.array_equal(got_count[:n], want_count)
    assert (got_mask[n] == POISON_W).all() and got_count[n] == POISON_C
    m2, c2 = engine.acquire_mask(ring, key, ok, lo16, band, span)          # the engine call, and the same bits on a second run
    assert torch.equal(m2, mask[:n]) and torch.equal(c2, count[:n])
    # the list: a permuted order with gaps between the ranges, every third record skipped
    rng = np.random.default_rng(n)
    base, at = np.full(n, -1, np.int64), 1
    for p in rng.permutation(n).tolist():
        if p % 3 != 2:
            base[p] = at
            at += int(want_count[p]) + (p % 2)
    total = at + 3
    rec_o, ctr_o = _poison(engine, (total,), POISON_R), _poison(engine, (total,), POISON_W)
    assert _raw_list(engine, mask[:n].contiguous(), lo16, n, span, base, total, rec_o, ctr_o) == 0
    want_rec, want_ctr = np.full(total, POISON_R, np.int32), np.full(total, POISON_W, np.uint32)
    A.list_model(cands, base, want_rec, want_ctr)
    assert np.array_equal(rec_o.cpu().numpy(), want_rec) and np.array_equal(ctr_o.cpu().numpy().view(np.uint32), want_ctr)
    assert (want_rec == POISON_R).sum() >= 4 and (want_rec != POISON_R).any()
    # in order, every record: the flat list of a walk
    base = np.cumsum(want_count.astype(np.int64)) - want_count
    r3, c3 = engine.acquire_list(m2, lo16, span, base, int(want_count.sum()))
    assert r3.cpu().numpy().tolist() == [p for p, cs in enumerate(cands) for _ in cs]
    assert (c3.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist() == [c for cs in cands for c in cs]
    # an entry at or past `total` is never written: the last range cut short
    short = int(want_count.sum()) - 1
    rec_s, ctr_s = _poison(engine, (short + 2,), POISON_R), _poison(engine, (short + 2,), POISON_W)
    assert _raw_list(engine, m2, lo16, n, span, base, short, rec_s, ctr_s) == 0
    assert torch.equal(rec_s[:short], r3[:short]) and (rec_s[short:] == POISON_R).all() and (ctr_s[short:] == POISON_W).all()


def test_empty_spans_and_refusals_leave_the_poison(engine, ring):
    n = 40
    rec = _records(7, n)
    span = (70_001, (1 << 22) + 5)
    _, _, W = A.span_words(span)
    fresh_m, fresh_c = _poison(engine, (n, W), POISON_W), _poison(engine, (n,), POISON_C)
    lib, ctx = engine._lib, engine._ctx
    # a span without a counter that touches one high half: a row of one zero word each; spans that touch none: nothing is enqueued
    mask, count = _poison(engine, (n, 1), POISON_W), _poison(engine, (n,), POISON_C)
    assert _raw_mask(engine, ring, rec, (70_000, 70_000), mask, count) == 0 and not mask.any() and not count.any()
    for why, over in (("H = 0 at 0", dict(lo=0, hi=0)), ("H = 0 at an aligned counter", dict(lo=65_536, hi=65_536)), ("H = 0 at the end", dict(lo=CTR_END, hi=CTR_END)),
                      ("no records", dict(P=0)), ("no records, no ring", dict(P=0, N=0)), ("nothing at all", dict(P=0, ring=None, key=None, mask=None))):
        mask, count = fresh_m.clone(), fresh_c.clone()
        assert _raw_mask(engine, ring, rec, span, mask, count, **over) == 0, why
        assert torch.equal(mask, fresh_m) and torch.equal(count, fresh_c), why
    refused = [("P < 0", dict(P=-1)), ("N < 0", dict(N=-1)), ("no ring", dict(N=0)), ("lo < 0", dict(lo=-1)), ("hi > 2^32", dict(hi=CTR_END + 1)),
               ("reversed", dict(lo=span[1], hi=span[0])), ("grid", dict(P=1 << 31, lo=0, hi=CTR_END))]
    refused += [(f"null {k}", {k: None}) for k in ("ring", "key", "ok", "lo16", "band", "mask", "count")]
    for why, over in refused:
        mask, count = fresh_m.clone(), fresh_c.clone()
        assert _raw_mask(engine, ring, rec, span, mask, count, **over) != 0, why
        assert lib.es_last_error(ctx), why
        assert torch.equal(mask, fresh_m) and torch.equal(count, fresh_c), why
    # the list call
    m, c = engine.acquire_mask(ring, *rec, span)
    c = c.cpu().numpy().astype(np.int64)
    base, total = np.cumsum(c) - c, int(c.sum())
    assert total > 0
    fresh_r, fresh_k = _poison(engine, (total,), POISON_R), _poison(engine, (total,), POISON_W)
    for why, over in (("H = 0", dict(lo=0, hi=0)), ("no records", dict(P=0)), ("total = 0", dict(total=0)), ("every record skipped", dict(base=_dev(engine, np.full(n, -1, np.int64))))):
        r, k = fresh_r.clone(), fresh_k.clone()
        assert _raw_list(engine, m, rec[2], n, span, base, total, r, k, **over) == 0, why
        assert torch.equal(r, fresh_r) and torch.equal(k, fresh_k), why
    refused = [("P < 0", dict(P=-1)), ("total < 0", dict(total=-1)), ("lo < 0", dict(lo=-1)), ("hi > 2^32", dict(hi=CTR_END + 1)), ("reversed", dict(lo=9, hi=3)),
               ("grid", dict(P=1 << 31, lo=0, hi=CTR_END))]
    refused += [(f"null {k}", {k: None}) for k in ("mask", "lo16", "base", "rec", "ctr")]
    for why, over in refused:
        r, k = fresh_r.clone(), fresh_k.clone()
        assert _raw_list(engine, m, rec[2], n, span, base, total, r, k, **over) != 0, why
        assert lib.es_last_error(ctx), why
        assert torch.equal(r, fresh_r) and torch.equal(k, fresh_k), why


# ------------------------------------------------------------------------------------------------------------------- the feature
J = 1                                                                      # the key the clip and the stream are marked under


@pytest.fixture(scope="module")
def clip(engine):
    """6 000 samples of noise with frames embedded under key J from counter 70 000 -> (marked clip, the noise alone)."""
    rng = np.random.default_rng(21)
    host = (0.05 * rng.standard_normal((1, 6000))).astype(np.float32)
    return engine.embed(KEYS[J], host, ctr0=ORIGIN, seed=5).audio[0].cpu().numpy(), host[0]


def _detector(engine, trace=True):
    det = WatermarkDetector(KEYS[J], list_size=LIST, engine=engine)
    det._trace = [] if trace else None
    return det


def _host_walk(engine, audio, span, max_records=8):
    """acquire() as the twin states it, over the real outputs of engine.header: the records in acquire.record_order, each record's
    acquire.candidates ascending, decoded in one batch and walked by a fresh detector -> (Acquired fields or None, tries, records)."""
    det = _detector(engine)
    sc = det._scan_prepare([np.asarray(audio, np.float32)], det._band_order())[0]
    sel = sc.sel
    recs = A.record_order(sc.hdr[0][sel], sc.hdr[1][sel], sc.rows[sel], sc.starts[sel], 0, max_records) if sel.size else []
    tries = []
    for k in recs:
        j = int(sel[k])
        band = sc.bands[int(sc.rows[j])]
        tries += [(j, int(band[0]), int(sc.starts[j]), c) for c in A.candidates(KEYS[J], int(sc.hdr[1][j]), BAND_PLAN.index(band), span)]
    results = det._decode_pairs(sc.src, [t[0] for t in tries], [t[3] for t in tries]) if tries else []
    trace = []
    for (j, lo, start, ctr), blobs in zip(tries, results):
        trace.append((lo, start, ctr))
        if det._accept(blobs, ctr):
            return (A.origin_of(ctr, start), ctr, start, len(trace)), trace, len(recs)
    return None, trace, len(recs)


def _fields(acq):
    return None if acq is None else (acq.ctr0, acq.ctr, acq.start, acq.tried)


def test_acquire_equals_the_host_walk_with_the_real_demodulator(engine, clip):
    x, noise = clip
    clips = [x, x[:4900].copy(), noise]
    singles, traces = [], []
    for c in clips:
        want, trace, nrec = _host_walk(engine, c, SPAN)
        det = _detector(engine)
        got = det.acquire(c, 48_000, span=SPAN)
        print(f"clip of {c.size}: {nrec} records, {len(trace)} tries, found {want}")
        assert _fields(got) == want and det._trace == trace
        assert got is None or got.records == nrec
        singles.append(got); traces.append(trace)
    assert traces[0]                                                        # the marked clip has header records to search
    # fewer records: a prefix of the same walk
    want, trace, nrec = _host_walk(engine, x, SPAN, max_records=1)
    det = _detector(engine)
    assert _fields(det.acquire(x, 48_000, span=SPAN, max_records=1)) == want and det._trace == trace == traces[0][:len(trace)] and nrec <= 1
    # the batch call: the per-clip calls of one detector, in input order
    one, many = _detector(engine), _detector(engine)
    want = [one.acquire(c, 48_000, span=SPAN) for c in clips]
    assert many.acquire_batch(clips, 48_000, span=SPAN) == want == singles and many._trace == one._trace == sum(traces, [])
    assert many.session_nonce == one.session_nonce
    # int16 and another rate go through the front of verify_batch
    pcm = np.round(x * 32767.0).astype(np.int16)
    det = _detector(engine)
    got = det.acquire_batch([pcm, x[::2].copy()], [48_000, 24_000], span=SPAN)
    assert len(got) == 2 and det._trace is not None


class CleanAnswers:
    """The demodulator patched as tests/test_gpu_counters.py patches it: a candidate of key J whose counter is the true counter of the
    frame at its position -- truth(frame rows, frame columns) -> counters, -1 for none -- gets the clean code word of a blob sealed for
    that counter; every other candidate keeps its real LLR row.  The header decode is patched in the same places only: on this clip (noise
    at 0.05 against the mark) the real decode says ok at no peak with the low half of the counter at its position -- its answers on the
    marked clip are those on the noise alone --, so a peak whose row is the band of its position's counter gets ok and that counter's low
    half; every other peak keeps its real header."""

    def __init__(self, engine, truth):
        from echoseal_amd.crypto import SecureChannel
        self.engine, self.truth, self.sec = engine, truth, SecureChannel(KEYS[J])
        self.clean, self.sealed, self.asked, self.answered, self.headers = {}, {}, {}, 0, 0

    def __enter__(self):
        from echoseal_amd.polar_fast import encode
        eng = self.engine
        real_llr, real_sched, real_header = eng.llr, eng.schedule, eng.header

        def header(y, band, hdr_pn, **k):                                   # ok with the true low half where the row's band is the true counter's
            ok, val, score = real_header(y, band, hdr_pn, **k)
            want = self.truth(k["rows"].cpu().numpy().astype(np.int64), k["start"].cpu().numpy().astype(np.int64))
            b = band.cpu().numpy()
            hit = [i for i in range(want.size) if want[i] >= 0 and band_index(KEYS[J], int(want[i])) == int(b[i])]
            if hit:
                at = torch.tensor(hit, dtype=torch.int64, device=ok.device)
                ok[at] = 1
                val[at] = torch.tensor([int(want[i]) & 0xFFFF for i in hit], dtype=val.dtype, device=val.device)
                self.headers += len(hit)
            return ok, val, score

        def schedule(sub_key, band_key, **k):                               # a detector's own schedule: its key is the one it was built with
            c = np.asarray(torch.as_tensor(k["ctrs"]).cpu().numpy(), np.int64) & 0xFFFFFFFF
            self.asked = {"ctrs": c, "mine": band_key == KEYS[J]}
            return real_sched(sub_key, band_key, **k)

        def llr(y, band, pn, **k):
            out = real_llr(y, band, pn, **k)
            want = self.truth(k["rows"].cpu().numpy().astype(np.int64), k["start"].cpu().numpy().astype(np.int64))
            for i in np.flatnonzero(self.asked["ctrs"] == want) if self.asked["mine"] else ():
                c = int(want[i])
                if c not in self.clean:
                    self.sealed[c] = self.sec.seal(b"ESAL" + c.to_bytes(4, "big") + b"\x07" * 8 + bytes(11))
                    self.clean[c] = ((2.0 * encode(self.sealed[c]).astype(np.float32) - 1.0) * 6.0).astype(np.float32)
                out[int(i)] = torch.from_numpy(self.clean[c]).to(out.device)
                self.answered += 1
            return out
        eng.llr, eng.schedule, eng.header = llr, schedule, header
        return self

    def __exit__(self, *exc):
        del self.engine.llr, self.engine.schedule, self.engine.header


def test_acquire_finds_the_origin_of_a_clip_marked_from_70000(engine, clip):
    x, _ = clip
    truth = lambda rows, cols: ORIGIN + (2 * cols + FRAME_LEN) // (2 * FRAME_LEN)
    with CleanAnswers(engine, truth) as fake:
        det = _detector(engine)
        acq = det.acquire(x, 48_000, span=SPAN)
        assert acq is not None and fake.answered > 0
        want, trace, nrec = _host_walk(engine, x, SPAN)
        assert _fields(acq) == want and det._trace == trace and acq.records == nrec and acq.tried == len(trace)
        assert acq.ctr == ORIGIN + counter_estimate(acq.start) and acq.ctr in range(ORIGIN, ORIGIN + 5)      # a frame's true counter
        assert acq.ctr0 == A.origin_of(acq.ctr, acq.start) and abs(acq.ctr0 - ORIGIN) <= 1
        assert acq.blob == fake.sealed[acq.ctr] and fake.sec.open(acq.blob) == acq.plain and int.from_bytes(acq.plain[4:8], "big") == acq.ctr
        assert acq.band == BAND_PLAN[band_index(KEYS[J], acq.ctr)] and det._trace[-1] == (acq.band[0], acq.start, acq.ctr)
        assert _detector(engine).verify(x, 48_000, ctr0=acq.ctr0) is True and _detector(engine).verify(x, 48_000) is False
        # spans that hold none of the clip's counters
        for span in ((0, ORIGIN), (ORIGIN + 11, 1 << 20), (ORIGIN + 11, ORIGIN + 11)):
            assert _detector(engine).acquire(x, 48_000, span=span) is None
        # the narrowest span that holds the found counter finds it at once
        only = _detector(engine)
        got = only.acquire(x, 48_000, span=(acq.ctr, acq.ctr + 1))
        assert got is not None and (got.ctr, got.start, got.ctr0) == (acq.ctr, acq.start, acq.ctr0) and only._trace[-1][2] == acq.ctr


def test_live_acquire_sets_the_origin_of_the_marked_stream_only(engine):
    from echoseal_amd.monitor import window_start
    rng = np.random.default_rng(9)
    pushes = PUSHES + (1050,)                                               # n = 7 296: the window [3 648, 7 296) holds two whole frames
    n_all = sum(pushes) + 1 + 1300
    host = (0.05 * rng.standard_normal((2, n_all))).astype(np.float32)
    xs = [engine.embed(KEYS[J], host[:1], ctr0=ORIGIN, seed=12).audio[0].cpu().numpy(), host[1]]
    det = WatermarkDetector(KEYS[J], list_size=LIST, engine=engine)
    mon = det.open_streams(2, window_s=W8 / 48_000, chunk_max=CM8, trace=True)
    pos = 0
    for ln in pushes:
        assert mon.push([x[pos: pos + ln] for x in xs]) == [False, False]
        pos += ln
    tab = mon.table
    w0 = int(window_start(pos, W8))
    assert w0 == 3648 and [mon.origin(s) for s in range(2)] == [None, None]

    def truth(rows, cols):                                                  # history row 4 s + band, column -> the stream's absolute sample
        s = rows // 4
        a = tab.base_host[s] + cols
        return np.where(s == 0, ORIGIN + (2 * a + FRAME_LEN) // (2 * FRAME_LEN), -1)
    with CleanAnswers(engine, truth) as fake:
        assert mon.acquire(span=(0, ORIGIN)) == [None, None] and [mon.origin(s) for s in range(2)] == [None, None]
        got = mon.acquire(span=SPAN)
        assert fake.answered > 0
        a = got[0]
        assert a is not None and got[1] is None and mon.position(0) == pos
        assert a.ctr == ORIGIN + counter_estimate(a.start, w0) and a.ctr0 == A.origin_of(a.ctr, a.start, w0) and abs(a.ctr0 - ORIGIN) <= 1
        assert mon.origin(0) == a.ctr0 and mon.origin(1) is None
        assert mon.traces(0)[0][-1] == (a.band[0], a.start, a.ctr) and mon.session_nonce(0) == a.plain[8:16]
        assert mon.acquire(span=SPAN) == [None] and mon.acquire([1], span=SPAN) == [None]      # only stream 1 is left without an origin
        with pytest.raises(ValueError, match="already has a counter origin"):
            mon.acquire([0])
    # the next pushes plan as a monitor opened with that origin does (brought to the same position with the real demodulator)
    ref = WatermarkDetector(KEYS[J], list_size=LIST, engine=engine).open_streams(2, window_s=W8 / 48_000, chunk_max=CM8, trace=True, ctr0=[a.ctr0, None])
    at = 0
    for ln in pushes:
        ref.push([x[at: at + ln] for x in xs])
        at += ln
    assert np.array_equal(ref.table.base_host, tab.base_host) and np.array_equal(ref.table.n_host, tab.n_host)
    with CleanAnswers(engine, truth):
        for ln in (1, 1300):
            chunks = [x[pos: pos + ln] for x in xs]
            pos += ln
            g, r = mon.push(chunks), ref.push(chunks)
            assert not g[1] and not r[1] and g[0] == r[0]
            for s in range(2):
                assert mon.traces(s) == ref.traces(s), (ln, s)
            assert mon.traces(0)[0] and all(c >= ORIGIN - 201 for _b, _s, c in mon.traces(0)[0])
