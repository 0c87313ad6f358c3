"""GPU: counter origins -- es_plan_at_batch and es_hop_window_batch against their host twins, and the live identifier, the
live monitor and the clip calls with origins against a WatermarkDetector per key that plans on the host (WatermarkDetector._scan_plan
with the scan's pos0 and ctr0): a yardstick that shares nothing with the device planner."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import memo as M
from echoseal_amd._native import ES_MAX_PEAKS, ES_MAX_TRIES
from echoseal_amd.detector import FRAME_LEN, WatermarkDetector
from echoseal_amd.engine import SyncResult
from echoseal_amd.identify import NB, WatermarkIdentifier, plan_reference
from echoseal_amd.monitor import window_start
from echoseal_amd.scan import CTR_END, SyncScan, counter_estimate, fitting_peaks
from echoseal_amd.utils import BAND_PLAN, band_index

KEYS = [b"\xAA" * 32, b"\x5C" * 32, bytes(range(32))]
W8, CM8, LIST = 3648, 1300, 8
PUSHES = (40, 1260, 1216, 1130, 1300, 1300, 0)                             # n = 40, 1300, 2516, 3646 (w0 = 0), 4946, 6246 (w0 > 0), 6246 again
# ... and two more: 7296 fills the window [3648, 7296) without moving it, one sample more moves it to 4864 -- the one push here after which
# the window still holds more than a frame period of starts (4864 .. 6081) that the push before decoded
LIVE_PUSHES = PUSHES[:-1] + (1050, 1)
SLOTS = 1024
ORIGINS = (0, 70_000, None)                                                 # stream 2 gets stream 0's samples: origin 0 against no origin
POS_BIG = 1216 * 2 ** 30
T_MAX, C_AT = 3648, 406                                                    # ceil(3648 / 1215) + 402


def _dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _words(x):
    return _u64(x) if torch.is_tensor(x) else np.asarray(x, np.uint64)


# ------------------------------------------------------------------------------------------------------------------- planner alone
def _plan_case(rng, configs, N=3, rows=8):
    """Inputs of one es_plan_at_batch call: `rows` sync rows of 25 (or 32) peaks and up to T_MAX samples seen by N keys, row r at
    configs[r % len(configs)] = (pos0, ctr0), one hop row per config with the base the header states."""
    HR = len(configs)
    lens = np.array([3648, 3648, 2500, 1215, 1300, 3648, 3000, 3648][:rows], np.int32)
    hrow = (np.arange(rows) % HR).astype(np.int32)
    pos0 = np.array([configs[h][0] for h in hrow], np.int64)
    ctr0 = np.array([configs[h][1] for h in hrow], np.int64)
    bases = np.array([max(0, counter_estimate(0, p, c) - 200) for p, c in configs], np.int64)
    peaks = np.full((rows, ES_MAX_PEAKS), -1, np.int32)
    npeaks = np.zeros(rows, np.int32)
    rowband = rng.integers(0, 4, rows).astype(np.uint8)
    fits = []
    for r in range(rows):
        n = 32 if r == 5 else 25
        st = np.sort(rng.integers(0, lens[r] - 62, n))
        st[:3] = np.sort(rng.integers(0, max(1, lens[r] - FRAME_LEN + 1), 3))  # some that can hold a frame, also in the short rows
        st[-2:] = [lens[r] - FRAME_LEN, lens[r] - FRAME_LEN + 1]            # the last that fits and the first that does not
        peaks[r, :n] = np.sort(st)
        npeaks[r] = n | (int(r % 3 == 0) << 30)
        look = peaks[r, :25]
        fits.append(look[(look >= 0) & (look + FRAME_LEN <= lens[r])])
    nfit = np.array([f.size for f in fits])
    base = (np.cumsum(nfit) - nfit).astype(np.int32)
    P = int(nfit.sum())
    dens = np.array([0.95, 0.25, 0.9])[:N]                                  # dense, in between, and dense with gaps (below): lists that reach 400
    hop = np.where(rng.random((N, HR, C_AT)) < dens[:, None, None], rowband[0], (rowband[0] + 1 + rng.integers(0, 3, (N, HR, C_AT))) % 4).astype(np.uint8)
    for r in range(rows):                                                   # the last key: no band at all within +-3 of any estimate, so
        for st in fits[r]:                                                  # a peak without a header falls back to its +-200 window
            col = counter_estimate(int(st), int(pos0[r]), int(ctr0[r])) - int(bases[hrow[r]])
            hop[N - 1, hrow[r], max(0, col - 3): max(0, col + 4)] = 0xFF
    hok = (rng.random((N, P)) < 0.4).astype(np.uint8)
    hlo = rng.integers(0, 65536, (N, P)).astype(np.int32)
    for r in range(rows):
        for j, st in enumerate(fits[r]):
            est = counter_estimate(int(st), int(pos0[r]), int(ctr0[r]))
            for k in range(N):
                if rng.random() < 0.6:
                    c = est + int(rng.integers(-200, 201))
                    hlo[k, base[r] + j] = c & 0xFFFF
                    col = c - int(bases[hrow[r]])
                    if rng.random() < 0.7 and 0 <= col < C_AT and c < CTR_END:
                        hop[k, hrow[r], col] = rowband[r]
    return dict(peaks=peaks, npeaks=npeaks, rowband=rowband, base=base, lens=lens, hok=hok, hlo=hlo, hop=hop, pos0=pos0, ctr0=ctr0, hrow=hrow,
                bases=bases)


def _plan_at(engine, c, **over):
    a = {**c, **over}
    d = lambda v: _dev(engine, v)
    return engine.plan(d(a["peaks"]), d(a["npeaks"]), a["rowband"], a["base"], a["lens"], d(a["hok"]), d(a["hlo"]), d(a["hop"]), pos0=a["pos0"],
                       ctr0=a["ctr0"], hop_row=a["hrow"], hop_base=a["bases"])


def _check_plan_at(res, c, skip_rows=()):
    slot, ctr = res.slot.cpu().numpy(), res.ctr.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    count, looked = res.count.cpu().numpy(), res.looked.cpu().numpy()
    N, rows = c["hop"].shape[0], c["lens"].size
    st = {"cut": 0, "wide": 0, "nonempty": 0, "hdr": 0}
    for k in range(N):
        for r in range(rows):
            p, h = k * rows + r, int(c["hrow"][r])
            if r in skip_rows:
                assert count[p] == 0 and looked[p] == 0, (k, r)
                continue
            want, want_looked = plan_reference(c["peaks"][r], c["npeaks"][r], int(c["lens"][r]), int(c["rowband"][r]), c["hok"][k, c["base"][r]:],
                                               c["hlo"][k, c["base"][r]:], c["hop"][k, h], pos0=int(c["pos0"][r]), ctr0=int(c["ctr0"][r]),
                                               hop_base=int(c["bases"][h]))
            got = list(zip(slot[p, :count[p]].tolist(), ctr[p, :count[p]].tolist()))
            assert got == want and looked[p] == want_looked, (k, r, count[p], len(want), got[:4], want[:4])
            assert all(cc < CTR_END for _s, cc in got)
            st["cut"] += len(want) == ES_MAX_TRIES
            st["nonempty"] += bool(want)
            st["wide"] += any(sum(1 for s, _ in want if s == sl) > 7 for sl in {s for s, _ in want})
            st["hdr"] += any(c["hok"][k, c["base"][r] + j] for j in range(want_looked))
    return st


@pytest.mark.parametrize("configs", [((0, 0), (0, 1), (1216, 199)), ((0, 200), (2432, 201)), ((1216 * 37, 65_436), (0, 65_536), (1216, 65_436)),
                                      ((1216 * 150, CTR_END - 300), (POS_BIG, 0), (POS_BIG, 65_536))], ids=["low", "200", "0xffff", "ends"])
def test_plan_at_equals_the_twin(engine, configs):
    c = _plan_case(np.random.default_rng(len(configs) * 1000 + configs[0][1] % 997), configs)
    assert c["hop"].shape == (3, len(configs), C_AT) and c["peaks"].shape == (8, 32) and int(c["lens"].max()) == T_MAX
    res = _plan_at(engine, c)
    st = _check_plan_at(res, c)
    assert st["cut"] > 0 and st["wide"] > 0 and st["nonempty"] > 8 and st["hdr"] > 0, st
    if configs[0][1] == CTR_END - 300:                                      # windows that pass the last counter (the table goes on with bands) end at it
        top = (res.ctr.cpu().numpy().astype(np.int64) & 0xFFFFFFFF)[np.arange(ES_MAX_TRIES)[None, :] < res.count.cpu().numpy()[:, None]].max()
        assert top == CTR_END - 1 and counter_estimate(T_MAX - FRAME_LEN, *configs[0]) + 200 >= CTR_END
    # a hop row outside [0, HR) plans nothing for its rows, and changes nothing for the others
    hrow = c["hrow"].copy()
    hrow[1], hrow[6] = -1, len(configs)
    _check_plan_at(_plan_at(engine, c, hrow=hrow), c, skip_rows=(1, 6))


def _raw_plan(engine, c, out, *, ragged=False, **over):
    """One direct call of the C entry point into the caller's output tensors -> its return code."""
    a = {**c, **over}
    d = lambda v, dt: None if v is None else _dev(engine, np.asarray(v).astype(dt))
    u32 = lambda v: None if v is None else _dev(engine, np.asarray(v).astype(np.uint32).view(np.int32))      # uint32 words in an int32 tensor
    keep = [d(a["peaks"], np.int32), d(a["npeaks"], np.int32), d(a["rowband"], np.uint8), d(a["base"], np.int32), d(a["lens"], np.int32),
            d(a["hok"], np.uint8), d(a["hlo"], np.int32), d(a["hop"], np.uint8), d(a["pos0"], np.int64), u32(a["ctr0"]), d(a["hrow"], np.int32),
            u32(a["bases"])]
    p = lambda t: None if t is None else t.data_ptr()
    pk, npk, rb, hb, ln, hok, hlo, hop, pos0, ctr0, hrow, hbase = keep
    N, HR, C = a.get("N", c["hop"].shape[0]), a.get("HR", c["hop"].shape[1]), a.get("C", c["hop"].shape[2])
    rows, P = a.get("rows", c["lens"].size), c["hok"].shape[1]
    lib, ctx, st = engine._lib, engine._ctx, engine._stream()
    if ragged:
        rc = lib.es_plan_ragged_batch(ctx, p(pk), p(npk), p(rb), p(hb), rows, p(ln), T_MAX, p(hok), p(hlo), P, p(hop), N, C, *[p(o) for o in out], st)
    else:
        rc = lib.es_plan_at_batch(ctx, p(pk), p(npk), p(rb), p(hb), rows, p(ln), T_MAX, p(hok), p(hlo), P, p(hop), N, C, p(pos0), p(ctr0), p(hrow),
                                  p(hbase), HR, *[p(o) for o in out], st)
    torch.cuda.synchronize()
    return rc


def _poison(engine, pairs):
    return [torch.full((pairs, ES_MAX_TRIES), 0xA5, dtype=torch.uint8, device=engine.device),
            torch.full((pairs, ES_MAX_TRIES), 0x5A5A5A5A, dtype=torch.int32, device=engine.device),
            torch.full((pairs,), -77, dtype=torch.int32, device=engine.device), torch.full((pairs,), -78, dtype=torch.int32, device=engine.device)]


def test_plan_at_at_zero_is_plan_ragged_byte_for_byte_and_refusals_write_nothing(engine):
    c = _plan_case(np.random.default_rng(5), ((0, 0),))
    assert c["hop"].shape[1] == 1 and not c["pos0"].any() and not c["ctr0"].any() and not c["bases"].any()
    a, b = _poison(engine, 24), _poison(engine, 24)
    assert _raw_plan(engine, c, a) == 0 and _raw_plan(engine, c, b, ragged=True) == 0
    assert all(torch.equal(x, y) for x, y in zip(a, b))                     # entries past a pair's count keep the poison on both sides
    assert int(a[2].sum()) > 24 and (a[2] == ES_MAX_TRIES).any()
    fresh = [t.clone() for t in _poison(engine, 24)]
    for why, over in (("narrow", dict(C=C_AT - 1)), ("no hop row", dict(HR=0)), ("null pos0", dict(pos0=None)), ("null ctr0", dict(ctr0=None)),
                      ("null hop_row", dict(hrow=None)), ("null hop_base", dict(bases=None)), ("null hop", dict(hop=None)), ("null len", dict(lens=None)),
                      ("null peaks", dict(peaks=None))):
        out = _poison(engine, 24)
        assert _raw_plan(engine, c, out, **over) != 0, why
        assert engine._lib.es_last_error(engine._ctx), why
        assert all(torch.equal(x, y) for x, y in zip(out, fresh)), why
    for why, over in (("no rows", dict(rows=0)), ("no keys", dict(N=0))):   # nothing to do: nothing enqueued, not an error
        out = _poison(engine, 24)
        assert _raw_plan(engine, c, out, **over) == 0, why
        assert all(torch.equal(x, y) for x, y in zip(out, fresh)), why
    out = _poison(engine, 24)                                               # looked_dev is nullable, as for es_plan_batch
    assert _raw_plan(engine, c, out[:3] + [None]) == 0 and torch.equal(out[2], a[2]) and torch.equal(out[0], a[0])


# ------------------------------------------------------------------------------------------------------------------- hop window
def test_hop_window_equals_band_index(engine):
    ring = engine.keyring(KEYS)
    bases = [0, 65_500, CTR_END - 100]
    hop = engine.hop_window(ring, bases, C_AT).cpu().numpy()
    assert hop.shape == (len(KEYS), len(bases), C_AT)
    for k, key in enumerate(KEYS):
        for h, b in enumerate(bases):
            want = np.array([band_index(key, b + col) if b + col < CTR_END else 0xFF for col in range(C_AT)], np.uint8)
            assert np.array_equal(hop[k, h], want), (k, b)
    assert (hop[:, 2, 100:] == 0xFF).all() and (hop[:, 2, :100] < 4).all() and (hop[:, :2] < 4).all()
    # the same bands as the schedule of listed (key, counter) records
    kk = torch.arange(len(KEYS), dtype=torch.int32, device=engine.device).repeat_interleave(C_AT)
    cc = (torch.arange(C_AT, dtype=torch.int64, device=engine.device) + 65_500).repeat(len(KEYS))
    assert torch.equal(engine.schedule_keyed(ring, kk, cc, want_pn=False)[1].reshape(len(KEYS), C_AT).cpu(), torch.from_numpy(hop[:, 1]))
    # argument rules
    lib, ctx, st = engine._lib, engine._ctx, engine._stream()
    out = torch.full((len(KEYS), 1, 8), 0xA5, dtype=torch.uint8, device=engine.device)
    base = torch.zeros(1, dtype=torch.int32, device=engine.device)
    for args in ((ring.ring.data_ptr(), 3, None, 1, 8, out.data_ptr()), (None, 3, base.data_ptr(), 1, 8, out.data_ptr()),
                 (ring.ring.data_ptr(), 3, base.data_ptr(), 1, 8, None), (ring.ring.data_ptr(), -1, base.data_ptr(), 1, 8, out.data_ptr())):
        assert lib.es_hop_window_batch(ctx, *args, st) != 0
    for args in ((ring.ring.data_ptr(), 0, base.data_ptr(), 1, 8, out.data_ptr()), (ring.ring.data_ptr(), 3, base.data_ptr(), 0, 8, out.data_ptr()),
                 (None, 3, None, 1, 0, None)):
        assert lib.es_hop_window_batch(ctx, *args, st) == 0
    torch.cuda.synchronize()
    assert (out == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------------- live streams
@pytest.fixture(scope="module")
def streams(engine):
    """Three streams: noise with frames embedded under key 0 from counter 0, the same under key 1 from counter 70 000, and stream 0's
    samples again (opened without an origin); and the band-pass of each whole stream."""
    rng = np.random.default_rng(9)
    n_all = sum(LIVE_PUSHES)
    host = (0.05 * rng.standard_normal((2, n_all))).astype(np.float32)
    xs = [engine.embed(KEYS[0], host[:1], ctr0=0, seed=11).audio[0].cpu().numpy(), engine.embed(KEYS[1], host[1:], ctr0=70_000, seed=12).audio[0].cpu().numpy()]
    xs.append(xs[0].copy())
    y_all = engine.bpf(_dev(engine, np.repeat(np.stack(xs), NB, axis=0)), _dev(engine, np.tile(np.arange(NB, dtype=np.uint8), len(xs))))
    return xs, y_all


def _host_walk(engine, det, y_whole, w0, n, origin):
    """One fresh-state walk of detector `det` over the window [w0, n) of a stream whose whole band-pass is y_whole [4, n_all] (row = band
    index): peaks by the calls that existed before the monitor, the plan by WatermarkDetector._scan_plan on the host with (pos0, ctr0)
    -> (verdict, tries, header decodes)."""
    det.session_nonce, det._trace, det._hdr_trace = None, [], []
    if n - w0 < 63:
        return False, [], []
    order = det._band_order()
    band_ids = np.array([det._band_id(b) for b in order], np.uint8)
    ys = y_whole[torch.from_numpy(band_ids.astype(np.int64)).to(engine.device), w0:n].contiguous()
    thr, peaks, npeaks = engine.pick(engine.xcorr(ys, _dev(engine, band_ids)))
    rows, starts = fitting_peaks(peaks, npeaks, [n - w0] * NB)
    scan = det._scans_of(SyncScan(SyncResult(ys, None, thr, peaks, npeaks), [n - w0], NB, rows, starts), order, band_ids)[0]
    scan.ctr0, scan.pos0 = origin, (w0 if origin is not None else 0)
    ok = det._verify_scans([scan], [[0]], order)[0]
    return ok, det._trace, det._hdr_trace


@pytest.fixture(scope="module")
def yardstick(engine, streams):
    """Per push, stream and key: the host walk of a detector of that key over the stream's window."""
    _, y_all = streams
    dets = [WatermarkDetector(k, list_size=LIST, engine=engine) for k in KEYS]
    out, pos = [], 0
    for ln in LIVE_PUSHES:
        pos += ln
        w0 = int(window_start(pos, W8))
        out.append([[_host_walk(engine, d, y_all[NB * s: NB * s + NB], w0, pos, ORIGINS[s]) for d in dets] for s in range(3)])
        out[-1] = [[(ok, list(tr), list(ht)) for ok, tr, ht in row] for row in out[-1]]
    return out


class Twin:
    """Follows a LiveIdentifier's memo calls on the engine with a MemoModel: every probe answer is checked as it is given."""

    def __init__(self, engine, slots):
        self.engine, self.model = engine, M.MemoModel(slots)
        self.real = (engine.memo_probe, engine.memo_insert)
        self.reset()

    def reset(self):
        self.planned, self.hit = [], []

    def __enter__(self):
        def probe(mem, k0, k1):
            hit = self.real[0](mem, k0, k1)
            want = self.model.probe(_words(k0), _words(k1))
            assert np.array_equal(hit.cpu().numpy().astype(bool), want)
            self.planned += list(zip(_words(k0).tolist(), _words(k1).tolist()))
            self.hit += want.tolist()
            return hit

        def insert(mem, k0, k1):
            self.real[1](mem, k0, k1)
            self.model.insert(_words(k0), _words(k1))
        self.engine.memo_probe, self.engine.memo_insert = probe, insert
        return self

    def __exit__(self, *exc):
        del self.engine.memo_probe, self.engine.memo_insert


def _open(engine, slots=SLOTS, origins=ORIGINS):
    ident = WatermarkIdentifier(KEYS, list_size=LIST, engine=engine)
    kw = {} if origins is None else {"ctr0": list(origins)}
    return ident.open_streams(3, window_s=W8 / 48_000, chunk_max=CM8, trace=True, memo_slots=slots, **kw)


def test_live_identifier_with_origins_equals_the_host_walk_and_its_memo_the_twin(engine, streams, yardstick):
    xs, _ = streams
    live, plain = _open(engine), _open(engine, slots=0)
    assert [live.origin(s) for s in range(3)] == list(ORIGINS) and list(live.table.origin_host) == [0, 70_000, -1]
    pos, tried, moved, kept = 0, 0, 0, 0
    with Twin(engine, SLOTS) as twin:
        for t, ln in enumerate(LIVE_PUSHES):
            twin.reset()
            chunks = [x[pos: pos + ln] for x in xs]
            got, traces = live.push(chunks)
            assert (got, traces) == plain.push(chunks)                      # the memo changes no answer and no trace
            pos += ln
            w0 = int(window_start(pos, W8))
            for s in range(3):
                assert live.window(s) == (w0, pos)
                for k in range(len(KEYS)):
                    ok, tr, ht = yardstick[t][s][k]
                    assert (got[s][k] is not None) == ok, (t, s, k)
                    assert traces[s][k] == (tr, ht), (t, s, k, len(traces[s][k][0]), len(tr))
                    if ok:
                        assert (got[s][k].ctr, got[s][k].start) == (tr[-1][2], tr[-1][1])
            if w0 == 0:                                                     # origin 0 at position 0 plans what no origin plans
                assert got[0] == got[2] and traces[0] == traces[2], t
            tried += sum(len(tk[0]) for row in traces for tk in row)
            # the memo: stats and table are the twin's, and what it was asked holds the encoding of DESIGN 4.18
            st = live.stats
            hit = np.array(twin.hit, bool)
            assert st["planned"] == len(twin.planned) == st["decoded"] + st["skipped"] and st["skipped"] == int(hit.sum()), (t, st)
            assert plain.stats == {"planned": st["planned"], "decoded": st["planned"], "skipped": 0}
            if live._memo is not None:
                assert np.array_equal(_u64(live._memo.table), twin.model.table), t
            if twin.planned:
                key, row, epoch, a, field = M.unpack(*(np.array(w, np.uint64) for w in zip(*twin.planned)))
                sid = row // NB
                org = np.array([-1 if o is None else o for o in ORIGINS], np.int64)[sid]
                est = org + (2 * a + FRAME_LEN) // (2 * FRAME_LEN)
                assert (field[org >= 0] <= M.DELTA_MAX).all() and not epoch.any()
                ctr = np.where(org >= 0, est - 200 + field, field)
                named = sorted(zip(sid.tolist(), key.tolist(), (row % NB).tolist(), (a - w0).tolist(), ctr.tolist()))
                lo = {int(b[0]): j for j, b in enumerate(BAND_PLAN)}
                walked = sorted((s, k, lo[b], start, c) for s in range(3) for k in range(len(KEYS)) for (b, start, c) in traces[s][k][0])
                assert named == walked, t                                   # nothing validated: every planned candidate was tried
                skipped = [int(hit[sid == s].sum()) for s in range(3)]
                decoded = [int((~hit[sid == s]).sum()) for s in range(3)]
                print(f"push {t}: w0 = {w0}, n = {pos}, skipped per stream {skipped}, decoded per stream {decoded}")
                # The window moved on.  What an earlier push can have decoded of it are the starts in [w0, n_before - 1215]: none at
                # n = 4946, 84 samples at n = 6246 (one MI355X run: 5 and 1 candidates skipped for streams 0 and 1), more than a frame
                # period at n = 7297 -- there a stream with an origin must meet candidates it has decoded before.
                if w0 > int(window_start(pos - ln, W8)):
                    moved += 1
                    if pos - ln - FRAME_LEN - w0 >= FRAME_LEN:
                        kept += 1
                        assert skipped[0] > 0 and skipped[1] > 0, (t, skipped, decoded)
    assert moved == 3 and kept == 1 and tried > 20 * len(KEYS)
    assert all(c >= 70_000 - 200 for k in range(len(KEYS)) for (_b, _s, c) in traces[1][k][0]) and any(traces[1][k][0] for k in range(len(KEYS)))


def test_live_monitor_with_origins_equals_the_host_walk(engine, streams, yardstick):
    xs, _ = streams
    for k in (0, 1):
        det = WatermarkDetector(KEYS[k], list_size=LIST, engine=engine)
        mon = det.open_streams(3, window_s=W8 / 48_000, chunk_max=CM8, trace=True, ctr0=list(ORIGINS))
        assert [mon.origin(s) for s in range(3)] == list(ORIGINS)
        pos = 0
        for t, ln in enumerate(LIVE_PUSHES):
            got = mon.push([x[pos: pos + ln] for x in xs])
            pos += ln
            for s in range(3):
                ok, tr, ht = yardstick[t][s][k]
                assert not ok and got[s] == ok and mon.traces(s) == (tr, ht), (k, t, s)     # (nothing validates: no session nonce is ever set)
        mon.close([1])
        assert mon.origin(1) is None and list(mon.add(1, ctr0=5)) == [1] and mon.origin(1) == 5 and list(mon.add(1)) == [3] and mon.origin(3) is None


class CleanAnswers:
    """The demodulator patched as tests/test_gpu_live_identify.py patches it, but only where the counter is right: a candidate of key
    j whose counter is the true counter of the frame at its position -- truth(frame rows, frame columns) -> counters, -1 for none --
    gets the clean code word of a blob sealed for that counter; every other candidate keeps its real LLR row."""

    def __init__(self, engine, j, truth):
        from echoseal_amd.crypto import SecureChannel
        self.engine, self.j, self.truth, self.sec = engine, j, truth, SecureChannel(KEYS[j])
        self.clean, self.sealed, self.asked, self.answered = {}, {}, {}, 0

    def __enter__(self):
        from echoseal_amd.polar_fast import encode
        eng = self.engine
        real_llr, real_keyed, real_sched = eng.llr, eng.schedule_keyed, eng.schedule

        def schedule_keyed(ring, key_idx, ctrs, **k):
            if k.get("want_pn", True):
                self.asked = {"ctrs": np.asarray(ctrs.cpu().numpy(), np.int64) & 0xFFFFFFFF, "keys": np.asarray(key_idx.cpu().numpy(), np.int64)}
            return real_keyed(ring, key_idx, ctrs, **k)

        def schedule(sub_key, band_key, **k):                               # a detector's own schedule: its key is the one it was built with
            c = np.asarray(torch.as_tensor(k["ctrs"]).cpu().numpy(), np.int64) & 0xFFFFFFFF
            self.asked = {"ctrs": c, "keys": np.full(c.size, self.j if band_key == KEYS[self.j] else -1, np.int64)}
            return real_sched(sub_key, band_key, **k)

        def llr(y, band, pn, **k):
            out = real_llr(y, band, pn, **k)
            want = self.truth(k["rows"].cpu().numpy().astype(np.int64), k["start"].cpu().numpy().astype(np.int64))
            for i in np.flatnonzero((self.asked["keys"] == self.j) & (self.asked["ctrs"] == want)):
                c = int(want[i])
                if c not in self.clean:
                    self.sealed[c] = self.sec.seal(b"ESAL" + c.to_bytes(4, "big") + b"\x07" * 8 + bytes(11))
                    self.clean[c] = ((2.0 * encode(self.sealed[c]).astype(np.float32) - 1.0) * 6.0).astype(np.float32)
                out[int(i)] = torch.from_numpy(self.clean[c]).to(out.device)
                self.answered += 1
            return out
        eng.llr, eng.schedule_keyed, eng.schedule = llr, schedule_keyed, schedule
        return self

    def __exit__(self, *exc):
        del self.engine.llr, self.engine.schedule_keyed, self.engine.schedule


def test_a_stream_marked_from_70000_is_found_only_with_its_origin(engine, streams):
    xs, _ = streams
    j = 1
    live, blind = _open(engine), _open(engine, origins=None)
    assert [blind.origin(s) for s in range(3)] == [None] * 3
    pos = 0
    for ln in LIVE_PUSHES[:-1]:                                             # to n = 7296: the window [3648, 7296) holds two whole frame periods of starts
        live.push([x[pos: pos + ln] for x in xs]); blind.push([x[pos: pos + ln] for x in xs])
        pos += ln
    tab = live.table

    def truth(rows, cols):                                                  # history row 4 s + band, column -> the stream's absolute sample
        s = rows // NB
        a = tab.base_host[s] + cols
        return np.where(s == 1, 70_000 + (2 * a + FRAME_LEN) // (2 * FRAME_LEN), -1)
    ln = 0
    chunks = [x[pos: pos] for x in xs]
    live.forget(); blind.forget()                                           # (what the real demodulator failed on is not asked again otherwise)
    with CleanAnswers(engine, j, truth) as fake:
        got, traces = live.push(chunks)
        w0 = live.window(1)[0]
        mine = [(b, st, c, 70_000 + counter_estimate(w0 + st)) for (b, st, c) in traces[1][j][0]]
        print(f"stream 1, key {j}: {len(mine)} tries, {sum(c == t for _b, _s, c, t in mine)} at the frame's own counter, {fake.answered} answered")
        assert fake.answered > 0
        assert np.array_equal(blind.table.base_host, tab.base_host)
        nothing, _ = blind.push(chunks)
    w0, n = live.window(1)
    assert w0 > 0 and n == pos + ln
    m = got[1][j]
    assert m is not None and [e is not None for e in got[1]] == [k == j for k in range(len(KEYS))]
    assert m.ctr == 70_000 + counter_estimate(w0 + m.start) and m.key == j and m.blob == fake.sealed[m.ctr] and fake.sec.open(m.blob) == m.plain
    assert int.from_bytes(m.plain[4:8], "big") == m.ctr and traces[1][j][0][-1][1:] == (m.start, m.ctr)
    assert all(e is None for e in got[0] + got[2])
    assert all(e is None for row in nothing for e in row)                   # without the origin no candidate is the frame's counter


# ------------------------------------------------------------------------------------------------------------------- clips
def test_clips_with_origins(engine):
    rng = np.random.default_rng(21)
    j = 1
    host = (0.05 * rng.standard_normal((1, 6000))).astype(np.float32)
    x = engine.embed(KEYS[j], host, ctr0=70_000, seed=5).audio[0].cpu().numpy()
    clips, origins = [x, x[:4900].copy()], [70_000, None]
    ident = WatermarkIdentifier(KEYS, list_size=LIST, engine=engine)
    ident.trace = True
    got, traces = ident.identify_batch(clips, 48_000, origins)
    y = engine.bpf(_dev(engine, np.repeat(x[None], NB, axis=0)), _dev(engine, np.arange(NB, dtype=np.uint8)))
    for c, (clip, o) in enumerate(zip(clips, origins)):
        for k, key in enumerate(KEYS):
            det = WatermarkDetector(key, list_size=LIST, engine=engine)
            ok, tr, ht = _host_walk(engine, det, y, 0, clip.size, o)        # (a clip that is a prefix: its band-pass is the prefix of y)
            assert (got[c][k] is not None) == ok and traces[c][k] == (tr, ht), (c, k, len(traces[c][k][0]), len(tr))
            det2 = WatermarkDetector(key, list_size=LIST, engine=engine); det2._trace, det2._hdr_trace = [], []
            assert det2.verify(clip, 48_000, o) == ok and (det2._trace, det2._hdr_trace) == (tr, ht), (c, k)
        assert traces[c][j][0] and (min(t[2] for t in traces[c][j][0]) >= 70_000 - 200) == (o is not None)
    det = WatermarkDetector(KEYS[j], list_size=LIST, engine=engine)
    assert det.verify_batch(clips, 48_000, origins) == [got[0][j] is not None, got[1][j] is not None]
    # None for every clip is the call without the argument
    assert ident.identify_batch(clips, 48_000, [None, None]) == ident.identify_batch(clips, 48_000) == ident.identify_batch(clips, 48_000, None)
    plain = WatermarkDetector(KEYS[j], list_size=LIST, engine=engine); plain._trace = []
    same = WatermarkDetector(KEYS[j], list_size=LIST, engine=engine); same._trace = []
    assert plain.verify_batch(clips, 48_000) == same.verify_batch(clips, 48_000, [None, None]) and plain._trace == same._trace and plain._trace
    # true positives: the clip with the origin matches, the one without does not
    truth = lambda rows, cols: 70_000 + (2 * cols + FRAME_LEN) // (2 * FRAME_LEN)
    with CleanAnswers(engine, j, truth) as fake:
        got, traces = ident.identify_batch(clips, 48_000, origins)
        det = WatermarkDetector(KEYS[j], list_size=LIST, engine=engine)
        verdicts = det.verify_batch(clips, 48_000, origins)
    m = got[0][j]
    assert m is not None and m.ctr == 70_000 + counter_estimate(m.start) and m.blob == fake.sealed[m.ctr]
    assert [e is not None for e in got[0]] == [k == j for k in range(len(KEYS))] and all(e is None for e in got[1])
    assert verdicts == [True, False]
