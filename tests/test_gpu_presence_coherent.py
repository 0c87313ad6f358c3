"""GPU: the coherent presence test -- es_mf_rows_batch and es_coherent_score_batch bit for bit (uint64 views) against their
host twin (echoseal_amd/presence.py) on the very arrays the kernels read, every refusal with its outputs unwritten, and
WatermarkDetector.presence_coherent / presence_coherent_batch field for field against the twin on the downloaded rows."""
from unittest import mock

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector

FL, TILE, CT, CHUNK = 1215, nat.ES_MF_TILE, nat.ES_COH_TILE, nat.ES_HOP_ORIGINS
POISON_F, POISON_I = -777.25, -77
D_CLIP = (0.2, 2.0, 7, 108)                                                 # clip D of DESIGN 4.23 (tests/test_presence_coherent_host.py)
SMALL = dict(span=(0, 16), decoys=8)


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the rows
def _rows_equal_twin(engine, y, lens, bands, tables=None):
    g, c = pr.mf_tables(tables=tables or engine.tables())
    out = [torch.full(y.shape, POISON_F, dtype=torch.float64, device=engine.device) for _ in range(3)]
    got = [t.cpu().numpy() for t in engine.mf_rows(_dev(engine, y), lens, bands, out=out)]
    want = pr.mf_rows_model(y, lens, bands, g, c)
    for a, w in zip(got, want):
        here = ~np.isnan(w)
        assert np.array_equal(_bits(a[here]), _bits(w[here])) and (a[~here] == POISON_F).all()        # written where defined, and nowhere else
    return got, want


def test_rows_equal_the_twin_around_the_window_and_the_tile_edge(engine):
    """Per band (four filter lengths): lengths W - 1, W, W + 1, those that put the last start and the last m on a tile's last and
    next first output, a record shorter than its filter, and NaN past every length."""
    g, _ = pr.mf_tables(tables=engine.tables())
    lens, bands = [], []
    for b in range(4):
        L, W = len(g[b]), 190 + len(g[b])
        lens += [W - 1, W, W + 1, W + TILE - 2, W + TILE - 1, W + TILE, L + TILE - 1, L + TILE, L + 2 * TILE + 1, L - 1, 0]
        bands += [b] * 11
    T = max(lens) + 7
    y = np.random.default_rng(80).standard_normal((len(lens), T))
    for r, n in enumerate(lens):
        y[r, n:] = np.nan                                                   # what must never be read
    got, want = _rows_equal_twin(engine, y, lens, bands)
    assert np.isfinite(got[1][1, 0]) and got[1][0, 0] == POISON_F and np.isfinite(got[0][0, 0]) and (got[0][9] == POISON_F).all()
    assert all(np.isnan(w).any() and not np.isnan(w).all() for w in want)


def test_rows_of_a_long_record_a_zero_row_and_clamped_lengths(engine):
    T = 5 * TILE + 321
    y = np.random.default_rng(81).standard_normal((4, T))
    y[1] = 0.0
    got, _ = _rows_equal_twin(engine, y, [T, T, 10 ** 9, -4], [0, 1, 2, 3])
    assert not got[0][1, :T - 115].any() and not got[2][1, :T - 305].any() and (got[2][0, :T - 320] > 0).all()     # the silent record: d == 0
    assert (got[0][3] == POISON_F).all()
    one = engine.mf_rows(_dev(engine, y[2:3]), [T], [2])                    # a record alone gives its rows of the batch; new rows are zero-filled
    assert np.array_equal(_bits(one[0].cpu().numpy()[0, :T - 122]), _bits(got[0][2, :T - 122])) and not one[1].cpu().numpy()[0, T - 312:].any()
    with pytest.raises(ValueError):
        engine.mf_rows(_dev(engine, y), [T] * 3, [0, 1, 2, 3])


def test_rows_with_550_taps_the_large_instantiation(engine):                       # (the fixture: skipped without a GPU)
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=0, fs=44_100)
    try:
        g, _ = pr.mf_tables(tables=eng.tables())
        L = max(len(t) for t in g)
        band = [len(t) for t in g].index(L)
        assert L == 550 and L > nat.ES_MAX_TAPS_FAST
        lens = [190 + L + TILE + 3, 190 + L, L + 1]
        y = np.random.default_rng(82).standard_normal((3, lens[0] + 2))
        for r, n in enumerate(lens):
            y[r, n:] = np.nan
        _rows_equal_twin(eng, y, lens, [band, band, (band + 1) % 4])
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- the score
def _case(seed, nslots, K, n_origins, negative=False):
    """Random M, A, D for len(nslots) clips, T a little above what the largest J needs; key rows from real keys."""
    rng = np.random.default_rng(seed)
    J = max(max(nslots), 1)
    T = 190 + FL * J + 5
    M = rng.standard_normal((4 * len(nslots), T))
    A = -np.abs(rng.standard_normal(M.shape)) * 40 - 50 if negative else rng.standard_normal(M.shape) * 8
    D = np.abs(rng.standard_normal(M.shape)) + 0.5
    hop = rng.integers(0, 4, (K, n_origins + J - 1)).astype(np.uint8)
    return M, A, D, hop


@pytest.fixture(scope="module")
def ring3(engine):
    keys = [PC.KEY] + pr.decoy_keys(2)
    ring = engine.keyring(keys)
    u = pr.header_signs(keys)
    assert np.array_equal(pr.ring_signs(ring.hdr_pn.cpu().numpy()), u)      # ring bytes 272 .. 287 are the twin's signs
    return ring, u


def _score_equals_twin(engine, ring3, M, A, D, nslot, phases, hop, lo, n_origins):
    ring, u = ring3
    got = [t.cpu().numpy() for t in engine.coherent_score(_dev(engine, M), _dev(engine, A), _dev(engine, D), nslot, np.asarray(phases, np.int32),
                                                          ring, _dev(engine, hop), lo, n_origins)]
    want = pr.coherent_score_model(M, A, D, nslot, phases, u, hop, lo, n_origins)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    return got


@pytest.fixture(scope="module")
def score_cases():
    out = {}
    for J in (1, CT - 1, CT, CT + 1, 63, 64, 65):
        c = _case(100 + J, [J, J // 2], 3, 257)
        for a in c:
            a.setflags(write=False)
        out[J] = c
    return out


@pytest.mark.parametrize("J", [1, CT - 1, CT, CT + 1, 63, 64, 65])
@pytest.mark.parametrize("n_origins", [1, 63, 64, 65, 257])
def test_score_equals_the_twin(engine, ring3, score_cases, n_origins, J):
    """Slot counts around the LDS tile of 16 slots and around 64; origins around a wave and past one block; lo such that the windows
    cross a multiple of 256 and of 65 536."""
    M, A, D, hop = score_cases[J]
    rng = np.random.default_rng(10 * n_origins + J)
    lo = 65536 * 3 - 20 - J // 2
    score, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [J, J // 2], rng.integers(0, FL, (2, 3)), hop[:, :n_origins + J - 1], lo, n_origins)
    assert np.isfinite(score[0]).all() and (origin[0] >= 0).all() and (origin[0] < n_origins).all() and (rank[0] >= 0).all()
    if J == 1:
        assert np.isneginf(score[1]).all() and (origin[1] == -1).all() and (rank[1] == -1).all()        # the second clip has no slot


@pytest.mark.parametrize("P, n_origins", [(1, 65), (1215, 3)])
def test_score_over_one_phase_and_over_all(engine, ring3, P, n_origins):
    M, A, D, hop = _case(120 + P, [3], 3, n_origins)
    phases = [np.random.default_rng(121).permutation(FL)[:P]]
    _score_equals_twin(engine, ring3, M, A, D, [3], phases, hop, 250, n_origins)           # counters 250 .. cross 256


def test_planted_ties_the_lower_origin_then_the_earlier_entry(engine, ring3):
    """m == 0 makes every header sum zero: N = a, and origins whose windows hop alike tie exactly, in a block and across blocks."""
    J, n = 3, CHUNK + 60
    T = 190 + FL * J
    M = np.zeros((4, T))
    A, D = np.full((4, T), -3.0), np.full((4, T), 2.0)                      # all scores negative: the best does not start at 0
    A[3] = -1.0
    hop = np.zeros((3, n + J - 1), np.uint8)
    hop[0, :] = np.arange(n + J - 1) % 2 * 3                                # key 0: origins of one parity share a window
    hop[1, 5:8] = 3; hop[1, CHUNK + 4:CHUNK + 7] = 3                        # key 1: origins 5 and 260, one per block
    hop[2, 100:103] = 3; hop[2, 200:203] = 3                                # key 2: origins 100 and 200 of one block
    score, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [J], [[17, 17]], hop, 1000, n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [0, 0, 0] and score[0, 1] == score[0, 2] == -0.5       # (key 0: odd origins hop 3, 0, 3)
    A[3, 17::FL] = -7.0                                                     # phase 17 is worse now; 18 named twice: the earlier entry
    _, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [J], [[17, 18, -1, 18, FL]], hop, 1000, n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [1, 1, 1]


def test_all_scores_negative_and_a_silent_window(engine, ring3):
    M, A, D, hop = _case(130, [CT + 1, 2], 3, 65, negative=True)
    D[:, 40] = 0.0                                                          # slot 0 of phase 40: the term is +0.0
    score, origin, _ = _score_equals_twin(engine, ring3, M, A, D, [CT + 1, 2], [[40, 3], [40, 1214]], hop, 7, 65)
    assert (score < 0).all() and (origin >= 0).all()


def test_missing_counters_no_slot_no_origin_and_no_phase(engine, ring3):
    M, A, D, hop = _case(131, [5, 0], 3, CHUNK + 20)
    n = CHUNK + 20
    hop[0, 100] = 0xFF                                                      # key 0: origins 96 .. 100 are out
    hop[1, n + 3] = 0xFF                                                    # key 1: the last column, touched by the last origin alone
    hop[2, :] = 0xFF                                                        # key 2: nothing to score
    score, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [5, 0], [[40, 7], [1, 2]], hop, 2 ** 32 - n - 4, n)
    assert origin[0, 0] not in range(96, 101) and origin[0, 0] >= 0 and 0 <= origin[0, 1] != n - 1
    assert np.isneginf(score[0, 2]) and origin[0, 2] == -1 and rank[0, 2] == -1
    assert np.isneginf(score[1]).all() and (origin[1] == -1).all()          # J == 0
    score, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [5, 5], [[40, 7], [1, 2]], hop, 0, 0)          # an empty span
    assert np.isneginf(score).all() and (origin == -1).all() and (rank == -1).all()
    score, origin, rank = _score_equals_twin(engine, ring3, M, A, D, [5, 99], [[-1, FL], [FL + 7, 6]], hop, 0, n)   # no phase; nslot clamped
    assert np.isneginf(score[0]).all() and (origin[0] == -1).all() and (rank[1, :2] == 1).all()


def test_two_runs_give_the_same_bits_and_both_calls_record_into_a_graph(engine, ring3):
    ring, _ = ring3
    T = 190 + 3 * FL + 400
    y = _dev(engine, np.random.default_rng(140).standard_normal((4, T)))
    lens, bands = _dev(engine, np.full(4, T, np.int32)), _dev(engine, np.arange(4, dtype=np.uint8))
    ns, ph = _dev(engine, np.array([3], np.int32)), _dev(engine, np.array([[5, 700, 1214]], np.int32))
    hop = _dev(engine, np.random.default_rng(141).integers(0, 4, (3, 300 + 2)).astype(np.uint8))
    out = [torch.zeros((4, T), dtype=torch.float64, device=engine.device) for _ in range(3)]

    def run():
        rows = engine.mf_rows(y, lens, bands, out=out)
        return [*rows, *engine.coherent_score(*rows, ns, ph, ring, hop, 65000, 300)]
    a = [t.clone() for t in run()]
    b = run()
    assert all(torch.equal(x, z) for x, z in zip(a, b)) and bool((a[4] >= 0).all())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = run()
    torch.cuda.synchronize()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, z) for x, z in zip(got, a))


# ---------------------------------------------------------------------------------------------------------------- refusals
def _raw(engine, name, order, args, **over):
    a = dict(args)
    a.update(over)
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                 # noqa: E731
    rc = getattr(engine._lib, name)(engine._ctx, *[p(a[k]) for k in order], engine._stream())
    torch.cuda.synchronize()
    return rc


ROWS_ORDER = ("y", "rows", "T", "len", "band", "m", "a", "d")
SCORE_ORDER = ("m", "a", "d", "rows", "T", "nslot", "B", "phase", "P", "ring", "hop", "K", "Ccols", "lo", "n_origins", "score", "origin", "rank", "scratch")


@pytest.fixture(scope="module")
def small(engine, ring3):
    """Calls that work: eight records of two slots; two clips, three keys, 300 origins (two chunks), two list entries."""
    T = 190 + 2 * FL + 140
    d = engine.device
    full = lambda shape, dt: torch.empty(shape, dtype=dt, device=d)         # noqa: E731
    y = np.random.default_rng(150).standard_normal((8, T))
    return dict(y=_dev(engine, y), rows=8, T=T, len=_dev(engine, np.full(8, T, np.int32)), band=_dev(engine, np.tile(np.arange(4, dtype=np.uint8), 2)),
                m=full((8, T), torch.float64), a=full((8, T), torch.float64), d=full((8, T), torch.float64),
                nslot=_dev(engine, np.array([2, 2], np.int32)), B=2, phase=_dev(engine, np.array([[1, 2], [3, 4]], np.int32)), P=2, ring=ring3[0].ring,
                hop=_dev(engine, np.random.default_rng(151).integers(0, 4, (3, 301)).astype(np.uint8)), K=3, Ccols=301, lo=9, n_origins=300,
                score=full((2, 3), torch.float64), origin=full((2, 3), torch.int64), rank=full((2, 3), torch.int32),
                scratch=full(3 * 2 * 3 * 2, torch.int64))


ROWS_REFUSALS = [dict(y=None), dict(len=None), dict(band=None), dict(m=None), dict(a=None), dict(d=None), dict(rows=-1), dict(T=-1), dict(T=1 << 31),
                 dict(rows=1 << 30, T=1 << 20)]
SCORE_REFUSALS = [dict(m=None), dict(a=None), dict(d=None), dict(nslot=None), dict(phase=None), dict(ring=None), dict(hop=None), dict(score=None),
                  dict(origin=None), dict(rank=None), dict(scratch=None), dict(rows=-8), dict(T=-1), dict(B=-2), dict(K=-3), dict(Ccols=-1),
                  dict(n_origins=-1), dict(rows=7), dict(Ccols=300), dict(n_origins=301), dict(P=0), dict(P=1216), dict(P=-1), dict(T=1 << 31),
                  dict(n_origins=1 << 40, Ccols=(1 << 40) + 1), dict(K=1 << 30, n_origins=1 << 10, Ccols=(1 << 10) + 1)]


@pytest.mark.parametrize("over", ROWS_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_rows_refusals_write_nothing(engine, small, over):
    for k in "mad":
        small[k].fill_(POISON_F)
    assert _raw(engine, "es_mf_rows_batch", ROWS_ORDER, small, **over) == nat.ES_EINVAL
    assert all((small[k] == POISON_F).all() for k in "mad")
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_mf_rows_batch")


def test_the_accepted_calls_and_the_empty_ones(engine, small, ring3):
    for k in "mad":
        small[k].fill_(POISON_F)
    small["score"].fill_(POISON_F)
    assert _raw(engine, "es_mf_rows_batch", ROWS_ORDER, small, rows=0) == 0 and _raw(engine, "es_mf_rows_batch", ROWS_ORDER, small, T=0) == 0
    assert _raw(engine, "es_coherent_score_batch", SCORE_ORDER, small, B=0) == 0 and _raw(engine, "es_coherent_score_batch", SCORE_ORDER, small, K=0) == 0
    assert all((small[k] == POISON_F).all() for k in "mad") and (small["score"] == POISON_F).all()
    assert _raw(engine, "es_mf_rows_batch", ROWS_ORDER, small) == 0 and _raw(engine, "es_coherent_score_batch", SCORE_ORDER, small) == 0
    g, c = pr.mf_tables(tables=engine.tables())
    T = small["T"]
    M, A, D = pr.mf_rows_model(small["y"].cpu().numpy(), [T] * 8, list(range(4)) * 2, g, c)
    got = [small[k].cpu().numpy() for k in "mad"]
    for a, w in zip(got, (M, A, D)):
        assert np.array_equal(_bits(a[~np.isnan(w)]), _bits(w[~np.isnan(w)])) and (a[np.isnan(w)] == POISON_F).all()
    want = pr.coherent_score_model(*got, [2, 2], [[1, 2], [3, 4]], ring3[1], small["hop"].cpu().numpy(), 9, 300)
    assert np.array_equal(_bits(small["score"].cpu().numpy()), _bits(want[0])) and np.array_equal(small["origin"].cpu().numpy(), want[1])
    assert np.array_equal(small["rank"].cpu().numpy(), want[2]) and (want[1] >= 0).all()


@pytest.mark.parametrize("over", SCORE_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_score_refusals_write_nothing(engine, small, over):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I); small["scratch"].fill_(POISON_I)
    assert _raw(engine, "es_coherent_score_batch", SCORE_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert (small["scratch"] == POISON_I).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_coherent_score_batch")


# ---------------------------------------------------------------------------------------------------------------- end to end
def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases) == (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


def _coherent_and_rows(engine, clip, fs=48_000, **kw):
    """presence_coherent() of one clip and the band-passed rows that call downloaded."""
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    nonce = det.session_nonce
    got = det.presence_coherent(clip, fs, **kw)
    (ids, y, sizes), = det._presence_rows
    assert ids == [0] and y.shape[0] == 4 and det.session_nonce is nonce and det._trace is None
    return got, y, int(sizes[0])


@pytest.fixture(scope="module")
def clip_d():
    with mock.patch.dict(PC.CLIPS, {"D": D_CLIP}):
        return PC.marked("D")


def test_presence_coherent_is_the_twin_and_finds_clip_D(engine, oracle, clip_d):
    got, y, n = _coherent_and_rows(engine, clip_d, **SMALL)
    assert n == clip_d.size
    _same(got, pr.coherent_model(y, n, PC.KEY, **SMALL))
    assert got.detected and (got.ctr, got.phase, got.ctr0, got.frames) == (*PC.FOUND, 1, 78) and got.null.shape == (8,) and len(got.phases) == FL
    print(f"clip D: own {got.score:.4f}, decoy max {got.null.max():.4f}, median {np.median(got.null):.4f}")
    ba = engine.tables()[0]
    x = np.ascontiguousarray(clip_d, np.float32)                            # the rows are the oracle's: the CPU verdicts are the GPU's
    assert np.array_equal(_bits(y[:, :n]), _bits(np.stack([oracle.lfilter(ba[b, :9], ba[b, 9:], x) for b in range(4)])))
    old = WatermarkDetector(PC.KEY, list_size=8, engine=engine).presence(clip_d, 48_000, span=(0, 64), phases=8, decoys=32)
    assert not old.detected                                                 # the preamble test on the same clip


def test_presence_coherent_finds_clip_A_with_the_origin_known(engine):
    clip = PC.cached("marked", "A")
    got, y, n = _coherent_and_rows(engine, clip, ctr0=1, decoys=5)
    _same(got, pr.coherent_model(y, n, PC.KEY, span=(1, 3), decoys=5))
    assert got.detected and (got.ctr, got.phase) == PC.FOUND and got.null.shape == (5,)


def test_the_cheap_mode_searches_the_folds_list(engine):
    clip = PC.cached("marked", "A")
    got, y, n = _coherent_and_rows(engine, clip, phases=8, **SMALL)
    plist = WatermarkDetector(PC.KEY, list_size=8, engine=engine).presence(clip, 48_000, phases=8, **SMALL).phases
    assert got.phases == plist and len(plist) == 8
    _same(got, pr.coherent_model(y, n, PC.KEY, phases=plist, **SMALL))
    assert got.detected and (got.ctr, got.phase) == PC.FOUND


def test_presence_coherent_batch_is_the_single_calls(engine, clip_d):
    from scipy.signal import resample_poly
    a = PC.cached("marked", "A")
    clips = [clip_d[:30_000], (resample_poly(a[:30_000], 147, 160) * 32768 * 20).astype(np.int16), a[:320 + FL - 1]]
    rates = [48_000, 44_100, 48_000]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    batch = det.presence_coherent_batch(clips, rates, phases=8, **SMALL)
    assert batch[2] is None and batch[0] is not None and batch[1] is not None and batch[0].frames == (30_000 - 320) // FL
    for clip, fs, got in zip(clips, rates, batch):
        _same(got, det.presence_coherent(clip, fs, phases=8, **SMALL))
    assert det.presence_coherent_batch([], 48_000) == []
