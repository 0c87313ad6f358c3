"""GPU: the presence test -- es_phase_fold_batch and es_hop_score_batch bit for bit (uint64 views) against their host twin
(echoseal_amd/presence.py) on the very rows the kernels read, the hop rows of the decoy ring against utils.band_index, every refusal with
its outputs unwritten, and WatermarkDetector.presence / presence_batch field for field against the twin on the downloaded rows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector

FL, TILE, CHUNK = 1215, nat.ES_HOP_TILE, nat.ES_HOP_ORIGINS
POISON_F, POISON_I = -777.25, -77


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)       # (a copy: the shared rows are read-only)


def _rows(seed, nlags, stride, negative=False):
    """Four random rows per clip in (-1, 1), NaN in every column at or past the clip's nlag."""
    rng = np.random.default_rng(seed)
    corr = rng.uniform(-1.0, 1.0, (4 * len(nlags), stride))
    if negative:
        corr = -np.abs(corr) - 0.25
    for b, n in enumerate(nlags):
        corr[4 * b:4 * b + 4, max(n, 0):] = np.nan
    return corr


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _score_equals_twin(engine, corr, nlag, phases, hop, n_origins):
    got = [t.cpu().numpy() for t in engine.hop_score(_dev(engine, corr), nlag, np.asarray(phases, np.int32), _dev(engine, hop), n_origins)]
    want = pr.score_model(corr, nlag, phases, hop, n_origins)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    return got


# ---------------------------------------------------------------------------------------------------------------- the fold
def test_fold_equals_the_twin_at_every_slot_count(engine):
    """nlag 1214 (no slot), 1215, 2 * 1215 + 7 and 5 * 1215 in one call, stride above every nlag, NaN in the padding."""
    nlag = [1214, FL, 2 * FL + 7, 5 * FL]
    corr = _rows(11, nlag, 5 * FL + 3)
    got = engine.phase_fold(_dev(engine, corr), nlag).cpu().numpy()
    want = pr.fold_model(corr, nlag)
    assert got.shape == (4, FL) and np.array_equal(_bits(got), _bits(want))
    assert not got[0].any() and np.isfinite(got).all() and np.abs(got[1:]).min() > 0
    one = engine.phase_fold(_dev(engine, corr[8:12]), [nlag[2]]).cpu().numpy()             # a clip alone gives its row of the batch
    assert np.array_equal(_bits(one[0]), _bits(got[2]))


def test_fold_of_negative_rows_and_clamped_lags(engine):
    corr = _rows(12, [3 * FL] * 3, 3 * FL, negative=True)
    nlag = [3 * FL, 10 ** 9, -4]                                            # clamped to [0, stride]
    got = engine.phase_fold(_dev(engine, corr), nlag).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(pr.fold_model(corr, nlag)))
    assert (got[:2] < -0.7).all() and not got[2].any()                      # a maximum of negatives, not of negatives and 0


# ---------------------------------------------------------------------------------------------------------------- the score
@pytest.fixture(scope="module")
def score_rows():
    """Per J: two clips (J slots and about half of them) in rows of stride > nlag, shared by the cases and left unchanged."""
    out = {}
    for J in (1, TILE - 1, TILE, TILE + 1):
        nlag = [J * FL + 5, (J // 2) * FL + 1214]
        corr = _rows(20 + J, nlag, J * FL + 9)
        corr.setflags(write=False)
        out[J] = (corr, nlag)
    return out


@pytest.mark.parametrize("J", [1, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("n_origins", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("P", [1, 3, 1215])
def test_score_equals_the_twin(engine, score_rows, P, n_origins, J):
    corr, nlag = score_rows[J]
    rng = np.random.default_rng(1000 * P + 10 * n_origins + J)
    if P == 1215:                                                           # every phase, shuffled; one clip keeps the twin quick
        corr, nlag = corr[:4], nlag[:1]
        phases = [rng.permutation(FL)]
    else:
        phases = rng.integers(0, FL, (2, P))
    hop = rng.integers(0, 4, (3, n_origins + J - 1)).astype(np.uint8)
    score, origin, rank = _score_equals_twin(engine, corr, nlag, phases, hop, n_origins)
    assert np.isfinite(score[0]).all() and (origin[0] >= 0).all() and (origin[0] < n_origins).all() and (rank[0] >= 0).all()
    if len(nlag) > 1 and J == 1:
        assert np.isneginf(score[1]).all() and (origin[1] == -1).all() and (rank[1] == -1).all()        # the second clip has no slot


def test_identical_windows_the_lower_origin_wins_in_a_block_and_across_blocks(engine):
    J, n = 3, CHUNK + 60
    nlag = [J * FL]
    corr = np.full((4, J * FL + 4), -0.5)
    corr[3, :J * FL] = 0.9                                                  # band 3 is where the mark is, at every lag
    corr[:, J * FL:] = np.nan
    hop = np.zeros((3, n + J - 1), np.uint8)
    hop[0, :] = np.arange(n + J - 1) % 2 * 3                                # key 0: origins of one parity share a window, in and across blocks
    hop[1, 5:8] = 3; hop[1, CHUNK + 4:CHUNK + 7] = 3                        # key 1: origins 5 and 260, one per block
    hop[2, 100:103] = 3; hop[2, 200:203] = 3                                # key 2: origins 100 and 200 of one block
    score, origin, rank = _score_equals_twin(engine, corr, nlag, [[17]], hop, n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [0, 0, 0]
    assert score[0, 1] == score[0, 2] == (0.9 + 0.9 + 0.9) / 3


def test_a_phase_named_twice_the_earlier_entry_wins(engine):
    nlag = [4 * FL]
    corr = _rows(31, nlag, 4 * FL + 2)
    hop = np.random.default_rng(32).integers(0, 4, (3, 70 + 3)).astype(np.uint8)
    fold = pr.fold_model(corr, nlag)[0]
    best = int(np.argmax(fold))
    score, origin, rank = _score_equals_twin(engine, corr, nlag, [[best, best, best]], hop, 70)
    assert rank[0].tolist() == [0, 0, 0]
    _, _, rank = _score_equals_twin(engine, corr, nlag, [[(best + 1) % FL, best, best]], hop, 70)
    assert set(rank[0].tolist()) <= {0, 1}


def test_all_scores_negative_the_best_does_not_start_at_zero(engine):
    nlag = [(TILE + 1) * FL, 2 * FL]
    corr = _rows(33, nlag, (TILE + 1) * FL + 1, negative=True)
    hop = np.random.default_rng(34).integers(0, 4, (3, 65 + TILE)).astype(np.uint8)
    score, origin, _ = _score_equals_twin(engine, corr, nlag, np.random.default_rng(35).integers(0, FL, (2, 3)), hop, 65)
    assert (score < -0.25).all() and (origin >= 0).all()


def test_the_last_lag_is_read_and_nothing_past_it(engine):
    J = TILE
    nlag = [J * FL]
    corr = _rows(36, nlag, J * FL + 8)                                      # NaN from column nlag on
    corr[:, J * FL - 1] = 0.999                                             # phase 1214 of the last slot: the last lag
    hop = np.random.default_rng(37).integers(0, 4, (3, 9 + J - 1)).astype(np.uint8)
    score, _, _ = _score_equals_twin(engine, corr, nlag, [[1214, 0]], hop, 9)
    assert np.isfinite(score).all()
    moved = corr.copy(); moved[:, J * FL - 1] = -0.999
    other, _, _ = _score_equals_twin(engine, moved, nlag, [[1214, 0]], hop, 9)
    changed = pr.score_model(corr, nlag, [[1214]], hop, 9)[0] != pr.score_model(moved, nlag, [[1214]], hop, 9)[0]
    assert changed.all() and np.isfinite(other).all()                       # the lag does enter every sum of phase 1214


def test_a_missing_counter_excludes_exactly_the_windows_that_touch_it(engine):
    J, n = 5, CHUNK + 20
    nlag = [J * FL]
    corr = _rows(38, nlag, J * FL)
    hop = np.random.default_rng(39).integers(0, 4, (3, n + J - 1)).astype(np.uint8)
    corr[:, :] = np.where(np.isnan(corr), corr, -0.5)
    for j in range(J):                                                      # key 0: the best window would be the one at origin 98 ...
        corr[hop[0, 98 + j], 40 + FL * j] = 0.9
    free = _score_equals_twin(engine, corr, nlag, [[40]], hop, n)
    assert free[1][0, 0] == 98
    hop[0, 100] = 0xFF                                                      # ... which holds column 100: origins 96 .. 100 are out
    hop[1, n + J - 2] = 0xFF                                                # key 1: the last column, touched by the last origin alone
    hop[2, :] = 0xFF                                                        # key 2: nothing to score
    score, origin, rank = _score_equals_twin(engine, corr, nlag, [[40]], hop, n)
    assert origin[0, 0] not in range(96, 101) and origin[0, 0] >= 0 and origin[0, 1] != n - 1
    assert np.isneginf(score[0, 2]) and origin[0, 2] == -1 and rank[0, 2] == -1
    only = hop.copy(); only[1, :] = 0xFF; only[1, n - 1:] = 2               # key 1: the last origin alone has a whole window
    _, origin, _ = _score_equals_twin(engine, corr, nlag, [[40]], only, n)
    assert origin[0, 1] == n - 1


def test_no_slot_no_origin_and_no_phase_give_nothing(engine):
    corr = _rows(40, [1214, 2 * FL], 2 * FL)
    hop = np.random.default_rng(41).integers(0, 4, (3, 12)).astype(np.uint8)
    score, origin, rank = _score_equals_twin(engine, corr, [1214, 2 * FL], [[3, 4], [5, 6]], hop, 11)
    assert np.isneginf(score[0]).all() and (origin[0] == -1).all() and (rank[0] == -1).all() and (origin[1] >= 0).all()
    score, origin, rank = _score_equals_twin(engine, corr, [1214, 2 * FL], [[3, 4], [5, 6]], hop, 0)          # an empty span
    assert np.isneginf(score).all() and (origin == -1).all() and (rank == -1).all()
    score, origin, rank = _score_equals_twin(engine, corr, [2 * FL, 2 * FL], [[-1, FL], [FL + 7, 6]], hop, 11)  # entries that are no phase
    assert np.isneginf(score[0]).all() and (origin[0] == -1).all() and (rank[1] == 1).all()


def test_two_runs_give_the_same_bits(engine):
    nlag = [7 * FL + 3]
    corr = _rows(42, nlag, 7 * FL + 3)
    hop = _dev(engine, np.random.default_rng(43).integers(0, 4, (3, 600 + 6)).astype(np.uint8))
    d = _dev(engine, corr)
    a = [t.cpu().numpy() for t in engine.hop_score(d, nlag, [[3, 1000, 77]], hop, 600)]
    b = [t.cpu().numpy() for t in engine.hop_score(d, nlag, [[3, 1000, 77]], hop, 600)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    f = engine.phase_fold(d, nlag).cpu().numpy()
    assert f.tobytes() == engine.phase_fold(d, nlag).cpu().numpy().tobytes()


def test_both_calls_record_into_a_graph(engine):
    """Neither call allocates, copies or synchronises: with device inputs they record into a stream capture, and a replay gives the
    eager bits."""
    nlag = [3 * FL + 11]
    d = _dev(engine, _rows(44, nlag, 3 * FL + 11))
    nl, ph = _dev(engine, np.array(nlag, np.int32)), _dev(engine, np.array([[5, 700]], np.int32))
    hop = _dev(engine, np.random.default_rng(45).integers(0, 4, (3, 300 + 2)).astype(np.uint8))
    want = [engine.phase_fold(d, nl), *engine.hop_score(d, nl, ph, hop, 300)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = [engine.phase_fold(d, nl), *engine.hop_score(d, nl, ph, hop, 300)]
    torch.cuda.synchronize()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and bool((got[2] >= 0).all())


# ---------------------------------------------------------------------------------------------------------------- refusals
def _raw(engine, name, order, args, **over):
    a = dict(args)
    a.update(over)
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                 # noqa: E731
    rc = getattr(engine._lib, name)(engine._ctx, *[p(a[k]) for k in order], engine._stream())
    torch.cuda.synchronize()
    return rc


FOLD_ORDER = ("corr", "rows", "stride", "nlag", "B", "fold")
SCORE_ORDER = ("corr", "rows", "stride", "nlag", "B", "phase", "P", "hop", "K", "Ccols", "n_origins", "score", "origin", "rank", "scratch")


@pytest.fixture(scope="module")
def small(engine):
    """A call that works: two clips of two slots, three keys, 300 origins (two chunks), two list entries."""
    corr = _rows(50, [2 * FL, 2 * FL], 2 * FL)
    d = engine.device
    return dict(corr=_dev(engine, corr), rows=8, stride=2 * FL, nlag=_dev(engine, np.array([2 * FL, 2 * FL], np.int32)), B=2,
                phase=_dev(engine, np.array([[1, 2], [3, 4]], np.int32)), P=2, hop=_dev(engine, np.random.default_rng(51).integers(0, 4, (3, 301)).astype(np.uint8)),
                K=3, Ccols=301, n_origins=300, fold=torch.empty((2, FL), dtype=torch.float64, device=d),
                score=torch.empty((2, 3), dtype=torch.float64, device=d), origin=torch.empty((2, 3), dtype=torch.int64, device=d),
                rank=torch.empty((2, 3), dtype=torch.int32, device=d), scratch=torch.empty(3 * 2 * 3 * 2, dtype=torch.int64, device=d))


FOLD_REFUSALS = [dict(corr=None), dict(nlag=None), dict(fold=None), dict(rows=-1), dict(stride=-1), dict(B=-1), dict(rows=7), dict(stride=1 << 31),
                 dict(B=1 << 29, rows=1 << 31)]
SCORE_REFUSALS = [dict(corr=None), dict(nlag=None), dict(phase=None), dict(hop=None), dict(score=None), dict(origin=None), dict(rank=None),
                  dict(scratch=None), dict(rows=-8), dict(stride=-1), dict(B=-2), dict(K=-3), dict(Ccols=-1), dict(n_origins=-1), dict(rows=7),
                  dict(Ccols=300), dict(n_origins=301), dict(P=0), dict(P=1216), dict(P=-1), dict(stride=1 << 31),
                  dict(n_origins=1 << 40, Ccols=(1 << 40) + 1), dict(K=1 << 30, n_origins=1 << 10, Ccols=(1 << 10) + 1)]


@pytest.mark.parametrize("over", FOLD_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_fold_refusals_write_nothing(engine, small, over):
    small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_phase_fold_batch", FOLD_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["fold"] == POISON_F).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_phase_fold_batch")


@pytest.mark.parametrize("over", SCORE_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_score_refusals_write_nothing(engine, small, over):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I); small["scratch"].fill_(POISON_I)
    assert _raw(engine, "es_hop_score_batch", SCORE_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert (small["scratch"] == POISON_I).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_hop_score_batch")


def test_the_accepted_call_and_the_empty_ones(engine, small):
    small["score"].fill_(POISON_F); small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_hop_score_batch", SCORE_ORDER, small, B=0) == 0 and _raw(engine, "es_hop_score_batch", SCORE_ORDER, small, K=0) == 0
    assert _raw(engine, "es_phase_fold_batch", FOLD_ORDER, small, B=0) == 0
    assert (small["score"] == POISON_F).all() and (small["fold"] == POISON_F).all()
    assert _raw(engine, "es_hop_score_batch", SCORE_ORDER, small) == 0 and _raw(engine, "es_phase_fold_batch", FOLD_ORDER, small) == 0
    corr, hop = small["corr"].cpu().numpy(), small["hop"].cpu().numpy()
    want = pr.score_model(corr, [2 * FL] * 2, [[1, 2], [3, 4]], hop, 300)
    assert np.array_equal(_bits(small["score"].cpu().numpy()), _bits(want[0])) and np.array_equal(small["origin"].cpu().numpy(), want[1])
    assert np.array_equal(_bits(small["fold"].cpu().numpy()), _bits(pr.fold_model(corr, [2 * FL] * 2)))
    with pytest.raises(ValueError):
        engine.phase_fold(small["corr"], [1, 2, 3])                         # three clips need twelve rows


# ---------------------------------------------------------------------------------------------------------------- hop rows of the decoys
@pytest.mark.parametrize("lo, cols", [(0, 90), (2 ** 32 - 20, 40)])
def test_hop_rows_of_the_decoy_ring_are_band_index(engine, lo, cols):
    keys = [PC.KEY] + pr.decoy_keys(4)
    hop = engine.hop_window(engine.keyring(keys), [lo], cols).cpu().numpy()
    assert hop.shape == (5, 1, cols) and np.array_equal(hop[:, 0, :], pr.hop_model(keys, lo, cols))
    assert (hop[:, 0, :min(cols, 2 ** 32 - lo)] < 4).all() and (hop[:, 0, 2 ** 32 - lo:] == 0xFF).all()


# ---------------------------------------------------------------------------------------------------------------- end to end
def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases) == (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


def _presence_and_twin(engine, clip, key, **kw):
    """presence() of one clip and the twin on the rows that call downloaded."""
    det = WatermarkDetector(key, list_size=8, engine=engine)
    det._presence_rows = []
    nonce = det.session_nonce
    got = det.presence(clip, 48_000, **kw)
    (ids, corr, nlag), = det._presence_rows
    assert ids == [0] and corr.shape[0] == 4 and int(nlag[0]) == clip.size - 62 and det.session_nonce is nonce and det._trace is None
    ctr0 = kw.pop("ctr0", None)
    if ctr0 is not None:
        kw["span"] = (ctr0, ctr0 + 2)
    _same(got, pr.presence_model(corr, int(nlag[0]), key, **kw))
    return got


@pytest.mark.parametrize("name", list(PC.CLIPS))
def test_presence_is_the_twin_and_finds_the_mark(engine, name):
    clip = PC.cached("marked", name)
    p = _presence_and_twin(engine, clip, PC.KEY, span=PC.SPAN, phases=8, decoys=32)
    assert p.detected and (p.ctr, p.phase, p.ctr0, p.frames) == (*PC.FOUND, 1, 78) and p.null.shape == (32,)
    print(f"clip {name}: own {p.score:.4f}, decoy max {p.null.max():.4f}, median {np.median(p.null):.4f}")
    q = _presence_and_twin(engine, clip, PC.KEY, ctr0=1, phases=3, decoys=5)               # the origin known: span (1, 3)
    assert q.detected and (q.ctr, q.phase) == PC.FOUND and q.score == p.score and q.null.shape == (5,)
    assert not _presence_and_twin(engine, clip, PC.OTHER_KEY, span=PC.SPAN, phases=8, decoys=32).detected
    assert not _presence_and_twin(engine, PC.cached("unmarked", name), PC.KEY, span=PC.SPAN, phases=8, decoys=32).detected


def test_the_rows_are_the_oracles(engine, oracle):
    """The correlation rows presence() reads are oracle.ncc over oracle.lfilter, bit for bit: the CPU verdicts of
    tests/test_presence_host.py are the GPU's."""
    clip = PC.cached("marked", "B")
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    det.presence(clip, 48_000, span=PC.SPAN)
    want, nlag = PC.oracle_rows(oracle, clip)
    assert np.array_equal(_bits(det._presence_rows[0][1][:, :nlag]), _bits(want))


def test_presence_batch_is_the_single_calls(engine):
    from scipy.signal import resample_poly
    a = PC.cached("marked", "A")
    clips = [a, a[:40_000], resample_poly(a, 147, 160).astype(np.float32), a[:1000], (a[:30_000] * 32768).astype(np.int16)]
    rates = [48_000, 48_000, 44_100, 48_000, 48_000]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    batch = det.presence_batch(clips, rates, span=PC.SPAN, phases=8, decoys=32)
    assert batch[3] is None and batch[0].detected and batch[1].detected and batch[1].frames == (40_000 - 62) // FL
    for clip, fs, got in zip(clips, rates, batch):
        _same(got, det.presence(clip, fs, span=PC.SPAN, phases=8, decoys=32))
    mixed = det.presence_batch(clips[:2], 48_000, [1, None], span=PC.SPAN, phases=8, decoys=32)      # an origin for the first clip alone
    _same(mixed[0], det.presence(clips[0], 48_000, 1, phases=8, decoys=32))
    _same(mixed[1], batch[1])
    assert det.presence_batch([], 48_000) == []
