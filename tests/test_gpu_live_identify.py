"""GPU: WatermarkIdentifier.open_streams / LiveIdentifier.push against the identifier's own clip path, and its memo against the host twin.

Per push and stream the yardstick is WatermarkIdentifier.identify on everything received while the window starts at 0, afterwards the
identifier's walk over a scan assembled from the calls that existed before the monitor (engine.xcorr + engine.pick) on the contiguous
slice y_whole[:, w0 : n].  The memo is followed call by call by echoseal_amd.memo.MemoModel: every probe answer, the table after every
push and the counts in `stats` are the twin's."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import memo as M
from echoseal_amd.engine import SyncResult
from echoseal_amd.identify import NB, WatermarkIdentifier
from echoseal_amd.monitor import window_start
from echoseal_amd.scan import SyncScan, fitting_peaks

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KEY = b"\xAA" * 32
KEYS = [KEY, b"\x5C" * 32, bytes(range(32))]
W8, CM8, LIST = 3648, 1300, 8
PUSHES = (40, 1260, 1216, 1130, 1300, 1300, 0)                             # n = 40, 1300, 2516, 3646 (w0 = 0), 4946, 6246 (w0 > 0), 6246 again
SLOTS = 1024                                                                # about what a push plans: many records lose their slot, many keep it


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _words(x):
    return _u64(x) if torch.is_tensor(x) else np.asarray(x, np.uint64)


@pytest.fixture(scope="module")
def streams(engine):
    """Three streams -- noise with frames embedded under key 0, a golden clip, plain noise -- and the band-pass of each whole stream."""
    rng = np.random.default_rng(9)
    n_all = sum(PUSHES)
    host = (0.05 * rng.standard_normal(n_all)).astype(np.float32)
    xs = [engine.embed(KEY, host[None, :], ctr0=0, seed=11).audio[0].cpu().numpy(),
          np.load(os.path.join(GOLD, "verify_trace.npz"))["clip"][:n_all].astype(np.float32), (0.1 * rng.standard_normal(n_all)).astype(np.float32)]
    y_all = engine.bpf(_dev(engine, np.repeat(np.stack(xs), NB, axis=0)), _dev(engine, np.tile(np.arange(NB, dtype=np.uint8), len(xs))))
    return xs, y_all


def _reference(engine, ident, x, y_whole, w0, n):
    """identify() of one stream's window by the calls that existed before live identification -> (matches, traces)."""
    ident.trace = True
    if w0 == 0:
        return ident.identify(x[:n], 48_000)
    ys = y_whole[:, w0:n].contiguous()
    thr, peaks, npeaks = engine.pick(engine.xcorr(ys, _dev(engine, np.arange(NB, dtype=np.uint8))))
    rows, starts = fitting_peaks(peaks, npeaks, [n - w0] * NB)
    out, traces = [[None] * len(ident.keys)], [[([], []) for _ in ident.keys]]
    ident._walk(SyncScan(SyncResult(ys, None, thr, peaks, npeaks), [n - w0], NB, rows, starts), out, traces)
    return out[0], traces[0]


class Twin:
    """Follows a LiveIdentifier's memo calls on the engine with a MemoModel: every probe answer is checked as it is given."""

    def __init__(self, engine, slots):
        self.engine, self.model = engine, M.MemoModel(slots)
        self.real = (engine.memo_probe, engine.memo_insert)
        self.reset()

    def reset(self):
        self.hits = self.misses = 0
        self.planned = []

    def __enter__(self):
        def probe(mem, k0, k1):
            hit = self.real[0](mem, k0, k1)
            want = self.model.probe(_words(k0), _words(k1))
            assert np.array_equal(hit.cpu().numpy().astype(bool), want)
            self.hits += int(want.sum()); self.misses += int((~want).sum())
            self.planned += list(zip(_words(k0).tolist(), _words(k1).tolist()))
            return hit

        def insert(mem, k0, k1):
            self.real[1](mem, k0, k1)
            self.model.insert(_words(k0), _words(k1))
        self.engine.memo_probe, self.engine.memo_insert = probe, insert
        return self

    def __exit__(self, *exc):
        del self.engine.memo_probe, self.engine.memo_insert


def _open(engine, n=3, slots=SLOTS, **kw):
    ident = WatermarkIdentifier(KEYS, list_size=LIST, engine=engine)
    return ident.open_streams(n, window_s=W8 / 48_000, chunk_max=CM8, trace=True, memo_slots=slots, **kw)


def test_pushes_equal_identify_and_the_memo_equals_its_twin(engine, streams):
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.polar_fast import encode
    xs, y_all = streams
    ref = WatermarkIdentifier(KEYS, list_size=LIST, engine=engine)
    live, plain = _open(engine), _open(engine, slots=0)
    assert live.table.window == W8 and list(live.table.bands) == [0, 1, 2, 3] and live.memo_slots == SLOTS and plain.memo_slots == 0
    pos, tried = 0, 0

    def push(twin, ln, sid=(0, 1, 2)):
        """One push of ln samples to streams sid of both identifiers, checked against the reference and the twin -> (matches, stats)."""
        twin.reset()
        chunks = [xs[s][pos: pos + ln] for s in sid]
        got, traces = live.push(chunks, list(sid))
        assert (got, traces) == plain.push(chunks, list(sid))               # the memo changes no answer and no trace
        n = pos + ln
        for i, s in enumerate(sid):
            w0 = int(window_start(n, W8))
            assert live.window(s) == (w0, n) and live.position(s) == n == live.received(s)
            want, want_tr = _reference(engine, ref, xs[s], y_all[NB * s: NB * s + NB], w0, n)
            assert got[i] == want, (s, n, got[i], want)
            assert traces[i] == want_tr, (s, n, [len(t[0]) for t in traces[i]], [len(t[0]) for t in want_tr])
        st = live.stats
        assert st["planned"] == st["decoded"] + st["skipped"] == len(twin.planned), (n, st)
        assert st["skipped"] == twin.hits and st["decoded"] == twin.misses, (n, st, twin.hits)
        assert plain.stats == {"planned": st["planned"], "decoded": st["planned"], "skipped": 0}
        if live._memo is not None:
            assert np.array_equal(_u64(live._memo.table), twin.model.table), n
            assert (live._memo.claim == -1).all()
        return got, traces, dict(st)

    with Twin(engine, SLOTS) as twin:
        for ln in PUSHES[:-1]:
            got, traces, st = push(twin, ln)
            pos += ln
            tried += sum(len(t[0]) for row in traces for t in row)
            assert all(m is None for row in got for m in row)               # the reference's DSP decodes nothing: every candidate failed
        assert tried > 20 * len(KEYS) and st["planned"] > 0
        # the same window again: whatever is decoded now was lost to a slot conflict, and the twin says how much that is
        before, last = set(twin.planned), dict(st)
        lost_then = int((~twin.model.probe(*(np.array(w, np.uint64) for w in zip(*twin.planned)))).sum())
        got, traces, st = push(twin, 0)
        assert set(twin.planned) == before and st["planned"] == last["planned"]
        assert st["skipped"] > 0 and st["decoded"] == twin.misses >= lost_then > 0      # (a rank's inserts may evict what a later rank asks for)
        assert st["decoded"] < st["planned"]

        # true positives: the demodulator's output replaced by the clean LLRs of a blob sealed under key j for the candidate's own counter
        j = 1
        sec, clean, sealed, asked = SecureChannel(KEYS[j]), {}, {}, {}
        real_llr, real_sched = engine.llr, engine.schedule_keyed

        def schedule_keyed(ring, key_idx, ctrs, **k):
            if k.get("want_pn", True):
                asked["ctrs"] = [int(c) & 0xFFFFFFFF for c in ctrs.tolist()]
            return real_sched(ring, key_idx, ctrs, **k)

        def llr(y, band, pn, **k):
            for c in asked["ctrs"]:
                if c not in clean:
                    sealed[c] = sec.seal(b"ESAL" + c.to_bytes(4, "big") + b"\x07" * 8 + bytes(11))
                    clean[c] = ((2.0 * encode(sealed[c]).astype(np.float32) - 1.0) * 6.0).astype(np.float32)
            return torch.from_numpy(np.stack([clean[c] for c in asked["ctrs"]])).to(engine.device)
        live.forget(); twin.model.clear()
        try:
            engine.llr, engine.schedule_keyed = llr, schedule_keyed
            got, traces, st = push(twin, 0)
        finally:
            engine.llr, engine.schedule_keyed = real_llr, real_sched
        assert st["skipped"] == 0 and st["decoded"] == st["planned"] > 0
        for s in range(3):
            assert [m is not None for m in got[s]] == [k == j for k in range(len(KEYS))], s
            m = got[s][j]
            assert m.key == j and m.variant == 0 and m.plain[:4] == b"ESAL" and int.from_bytes(m.plain[4:8], "big") == m.ctr
            assert m.blob == sealed[m.ctr] and sec.open(m.blob) == m.plain and traces[s][j][0][-1][1:] == (m.start, m.ctr) and len(traces[s][j][0]) == 1
        # the real demodulator again: what was cached under the fake one is forgotten, everything is decoded anew and fails
        live.forget(); twin.model.clear()
        got, traces, st = push(twin, 0)
        assert st["skipped"] == 0 and st["decoded"] == st["planned"] == last["planned"]
        assert all(m is None for row in got for m in row)


def test_a_reopened_slot_meets_no_stale_verdicts(engine, streams):
    """Stream 0 is pushed, closed, opened again as slot 0 and pushed the same samples.  Its records now carry epoch 1, so none of the old
    stream's verdicts is met: results and stats are those of an identifier that has never seen the samples.  That yardstick's slot is
    closed and opened once too before its first sample: with a direct-mapped table which records lose their slot to each other depends on
    the epoch in the record, and an insert replaces whatever a slot held, so with equal epochs the two memos evolve alike."""
    xs, _ = streams
    live, fresh = _open(engine), _open(engine, n=1)
    at = 0
    for ln in PUSHES[:5]:
        live.push([x[at: at + ln] for x in xs], [0, 1, 2])
        at += ln
    live.close([0])
    with pytest.raises(ValueError, match="closed"):
        live.push([xs[0][:10]], [0])
    assert len(live) == 2 and list(live.add(1)) == [0] and len(live) == 3 and live.position(0) == 0
    fresh.close([0])
    assert list(fresh.add(1)) == [0]
    at, skipped = 0, 0
    for ln in PUSHES:
        a, b = live.push([xs[0][at: at + ln]], [0]), fresh.push([xs[0][at: at + ln]], [0])
        at += ln
        assert a == b and live.stats == fresh.stats, (at, live.stats, fresh.stats)
        skipped += live.stats["skipped"]
    assert skipped > 0 and live.position(0) == at                           # (the last push repeats a window: the memo was in use)


def test_a_stream_at_44100_equals_an_at_rate_identifier_of_the_conditioned_chunks(engine):
    from scipy.signal import resample_poly
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"][:9_600].astype(np.float64)
    x = np.clip(np.round(resample_poly(clip, 147, 160) * 32768), -32768, 32767).astype(np.int16)
    live, yard = _open(engine, n=2, fs=[48_000, 44_100]), _open(engine, n=2)
    rt = engine.open_resampler([44_100], 48_000)
    other = (0.1 * np.random.default_rng(5).standard_normal(x.size)).astype(np.float32)
    with pytest.raises(ValueError, match="opened at 44100 Hz"):
        live.push([x[:10]], [1], fs=48_000)
    tried = 0
    for a in range(0, x.size, 1100):
        rows, counts = engine.resample_step(rt, [0], [x[a: a + 1100]])
        cond = rows[0, :int(counts[0])].cpu().numpy()
        assert cond.size <= CM8
        got = live.push([other[a: a + 1100], x[a: a + 1100]], [0, 1])
        want = yard.push([other[a: a + 1100], cond], [0, 1])
        assert got == want and live.stats == yard.stats, a
        assert live.position(1) == yard.position(1) and live.window(1) == yard.window(1)
        tried += sum(len(t[0]) for t in got[1][1])
    assert tried > 20 and live.rate(1) == 44_100 and live.received(1) == x.size and live.position(1) < x.size * 160 // 147 + 1
