"""GPU: the presence test on live windows -- es_warp_fold_at_batch and es_warp_score_at_batch bit for bit (uint64 views)
against their host twin (presence.window_rows, then warp_fold_model / warp_score_model on the record's hop row) on one shared table of
rows that is NaN everywhere but each record's own lags; records that are not addressable; both identities of the header; every refusal
with its outputs unwritten; capture and replay; and LiveMonitor.presence, LiveIdentifier.presence and WatermarkIdentifier.presence_batch
field for field against presence.live_model on the downloaded history, against the clip call and against each other."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

FL, SEG, TILE, CHUNK, HB = 1215, 1216, nat.ES_HOP_TILE, nat.ES_HOP_ORIGINS, nat.ES_WARP_HB
POISON_F, POISON_I = -777.25, -77
ROWS, PERM = 9, (6, 2, 7, 0)                                                # a band -> row map that is no identity and skips rows
SKEWS = (0, 3, -3)


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ramp(J, e):
    j = np.arange(J, dtype=np.int64)
    return (2 * j * e + J) // (2 * J) if J else j


@pytest.fixture(scope="module")
def noise():
    """Random rows in (-1, 1), made once and left unchanged; every test masks a copy with NaN."""
    a = np.random.default_rng(250).uniform(-1.0, 1.0, (ROWS, 66 * FL + SEG + 40))
    a.setflags(write=False)
    return a


def _table(noise, stride, recs):
    """corr [ROWS, stride]: NaN everywhere except columns [col, col + nlag) (clamped to the table) of each addressable record's four rows."""
    corr = np.full((ROWS, stride), np.nan)
    for rows4, col, nlag in recs:
        if 0 <= col <= stride and all(0 <= r < ROWS for r in rows4):
            n = min(max(nlag, 0), stride - col)
            for r in rows4:
                corr[r, col:col + n] = noise[r, col:col + n]
    return corr


def _twin(corr, recs, warp, nwarp, nslot, hyp, hop, hop_row, n_origins):
    """Record by record: the block the kernels may read as a clip of its own, through the models of the clip calls."""
    folds, scores = [], []
    K, HR = hop.shape[0], hop.shape[1]
    for b, (rows4, col, nlag) in enumerate(recs):
        block = pr.window_rows(corr, rows4, col, nlag)
        tab = (np.asarray(warp)[b:b + 1], [nwarp[b]], [nslot[b]])
        folds.append(pr.warp_fold_model(block, [block.shape[1]], *tab)[0])
        if 0 <= hop_row[b] < HR:
            scores.append([a[0] for a in pr.warp_score_model(block, [block.shape[1]], *tab, np.asarray(hyp)[b:b + 1], hop[:, hop_row[b]], n_origins)])
        else:
            scores.append([np.full(K, -np.inf), np.full(K, -1, np.int64), np.full(K, -1, np.int32)])
    return np.stack(folds), [np.stack([s[i] for s in scores]) for i in range(3)]


def _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, hop_row, n_origins):
    d = _dev(engine, corr)
    rows4, col, nlag = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    warp = np.asarray(warp, np.int32)
    fold = engine.warp_fold_at(d, rows4, col, nlag, warp, nwarp, nslot).cpu().numpy()
    got = [t.cpu().numpy() for t in engine.warp_score_at(d, rows4, col, nlag, warp, nwarp, nslot, np.asarray(hyp, np.int32), _dev(engine, hop),
                                                         hop_row, n_origins)]
    want_fold, want = _twin(corr, recs, warp, nwarp, nslot, hyp, hop, hop_row, n_origins)
    assert fold.dtype == np.float64 and fold.shape == want_fold.shape and np.array_equal(_bits(fold), _bits(want_fold)), (fold, want_fold)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    return fold, got


def _case(J, H, n_origins, HR, B, seed):
    """B records of J slots (record b has b slots fewer, at least one) under the three rows of SKEWS, H entries, three keys."""
    rng = np.random.default_rng(seed)
    nslot = [max(J - b, 1) for b in range(B)]
    warp = np.stack([np.stack([np.pad(_ramp(n, e), (0, J - n)) for e in SKEWS]) for n in nslot])
    hyp = np.stack([rng.integers(0, 3, (B, H)), rng.integers(0, FL, (B, H))], axis=2)
    hop = rng.integers(0, 4, (3, HR, n_origins + J - 1)).astype(np.uint8)
    return warp, [3] * B, nslot, hyp, hop


# ---------------------------------------------------------------------------------------------------------------- against the twin
@pytest.mark.parametrize("where", ["0", "1", "1216", "end"])
def test_records_at_every_column_equal_the_twin(engine, noise, where):
    """Three records in one call: a permuted band -> row map, and two records that share rows and overlap.  Everything of the table
    that is not some record's own lags is NaN, the columns before `col` included: a stray read shows in the bits."""
    J, stride = 3, 5 * FL + SEG
    nlag = J * FL + 7
    col = {"0": 0, "1": 1, "1216": SEG, "end": stride - nlag}[where]
    recs = [(PERM, col, nlag), ((1, 3, 4, 5), col, 2 * FL + 3), ((3, 1, 5, 4), min(col + 700, stride - 2 * FL), 2 * FL)]
    corr = _table(noise, stride, recs)
    assert np.isnan(corr[8]).all() and np.isnan(corr[PERM[0], col + nlag:]).all() and (col == 0 or np.isnan(corr[:, :col]).all())
    warp, nwarp, nslot, hyp, hop = _case(J, HB + 1, CHUNK + 1, 3, 3, 300 + col)
    fold, (score, origin, rank) = _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, [2, 0, 1], CHUNK + 1)
    assert np.isfinite(fold).all() and np.isfinite(score).all() and (origin >= 0).all() and (rank >= 0).all()
    assert not np.array_equal(fold[1], fold[2])                             # the overlapping records are two records


@pytest.mark.parametrize("J", [1, TILE - 1, TILE, TILE + 1])
def test_score_equals_the_twin_at_the_slot_tile(engine, noise, J):
    assert (TILE, HB) == (64, 8)
    stride = noise.shape[1]
    recs = [(PERM, SEG, J * FL + 11), ((0, 1, 2, 3), 1, (J + 1) * FL)]
    corr = _table(noise, stride, recs)
    warp, nwarp, nslot, hyp, hop = _case(J, 2, 5, 2, 2, 400 + J)
    _, (score, origin, _) = _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, [1, 0], 5)
    assert np.isfinite(score).all() and (origin >= 0).all()


@pytest.mark.parametrize("H", [1, HB, HB + 1])
@pytest.mark.parametrize("n_origins", [1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_score_equals_the_twin_at_the_block_and_chunk_edges(engine, noise, n_origins, H):
    stride = 4 * FL + SEG
    recs = [(PERM, SEG, 3 * FL + 5), ((8, 5, 3, 1), 2, 2 * FL + 1214)]
    corr = _table(noise, stride, recs)
    warp, nwarp, nslot, hyp, hop = _case(3, H, n_origins, 2, 2, 1000 * H + n_origins)
    _, (score, origin, rank) = _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, [0, 1], n_origins)
    assert np.isfinite(score).all() and (origin < n_origins).all() and (rank < H).all()


def test_hop_rows_give_each_record_its_own_winner(engine, noise):
    """HR = 3, and one record named four times under hop rows 0, HR - 1, -1 and HR: the two inside the table win at different origins,
    the two outside score nothing."""
    stride, HR = 4 * FL, 3
    recs = [(PERM, 5, 3 * FL)] * 4
    corr = _table(noise, stride, recs)
    warp, nwarp, nslot, hyp, hop = _case(3, 2, 40, HR, 4, 77)
    nslot, warp[:], hyp[:] = [3] * 4, warp[0], hyp[0]
    _, (score, origin, rank) = _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, [0, HR - 1, -1, HR], 40)
    assert np.isfinite(score[:2]).all() and not np.array_equal(origin[0], origin[1]) and not np.array_equal(_bits(score[0]), _bits(score[1]))
    assert np.isneginf(score[2:]).all() and (origin[2:] == -1).all() and (rank[2:] == -1).all()


def test_records_that_are_not_addressable_read_nothing(engine, noise):
    """A row index of -1 and of `rows`, col = stride + 1 and col = -1: no lags -- zeros in the usable fold rows, nothing scored -- beside
    a record whose nlag reaches past the stride and is clamped, and one whose col is the stride itself."""
    stride = 3 * FL + 9
    recs = [((0, 1, 2, -1), 0, 2 * FL), ((0, 1, ROWS, 3), 0, 2 * FL), (PERM, stride + 1, 2 * FL), (PERM, -1, 2 * FL),
            (PERM, 9, 1 << 30), (PERM, stride, 2 * FL), ((-(1 << 62), 1, 2, 3), 1 << 62, 2 * FL)]
    corr = _table(noise, stride, recs)
    B = len(recs)
    warp, nwarp, nslot, hyp, hop = _case(2, 3, 7, 1, B, 78)
    nslot = [2] * B
    fold, (score, origin, rank) = _equals_twin(engine, corr, recs, warp, nwarp, nslot, hyp, hop, [0] * B, 7)
    for b in (0, 1, 2, 3, 5, 6):
        assert not fold[b].any() and np.isneginf(score[b]).all() and (origin[b] == -1).all() and (rank[b] == -1).all()
    assert np.isfinite(fold[4]).all() and fold[4].all() and np.isfinite(score[4]).all()             # clamped to stride - col = 3 * 1215: served


def test_a_table_holding_the_ends_of_int32_is_judged_before_it_is_read(engine, noise):
    stride = 3 * FL + SEG
    recs = [(PERM, SEG, 3 * FL)] * 2
    corr = _table(noise, stride, recs)
    lo, hi = -(1 << 31), (1 << 31) - 1
    warp = np.array([[[0, 0, 0], [0, lo, 0], [0, 0, hi]], [[hi, 0, 0], [0, 0, 0], [0, 0, lo]]], np.int64)
    hyp = np.array([[(0, 5), (1, 5), (2, 5)], [(0, 6), (1, 6), (2, 6)]])
    hop = np.random.default_rng(79).integers(0, 4, (2, 1, 12)).astype(np.uint8)
    fold, (score, _, rank) = _equals_twin(engine, corr, recs, warp, [3, 3], [3, 3], hyp, hop, [0, 0], 10)
    assert np.isneginf(fold[0, 1:]).all() and np.isneginf(fold[1, 0]).all() and np.isneginf(fold[1, 2]).all()
    assert np.isfinite(fold[0, 0]).all() and np.isfinite(fold[1, 1]).all() and (rank[0] == 0).all() and (rank[1] == 1).all() and np.isfinite(score).all()


# ---------------------------------------------------------------------------------------------------------------- identities
def test_both_identities_of_the_header(engine, noise):
    """row[b][band] = 4 b + band, col = 0, HR = 1, hop_row = 0: the bits of warp_fold / warp_score; with D = 1, zeros and
    nslot = nlag / 1215 also those of phase_fold / hop_score."""
    nlag = [(TILE + 1) * FL + 11, 3 * FL]
    stride = nlag[0]
    corr = np.array(noise[:8, :stride])
    for b, n in enumerate(nlag):
        corr[4 * b:4 * b + 4, n:] = np.nan
    d = _dev(engine, corr)
    rows4, col = [[0, 1, 2, 3], [4, 5, 6, 7]], [0, 0]
    rng = np.random.default_rng(80)
    nslot = [TILE, 3]
    warp = np.stack([np.stack([np.pad(_ramp(n, e), (0, TILE + 1 - n)) for e in SKEWS]) for n in nslot]).astype(np.int32)
    hyp = np.stack([rng.integers(0, 3, (2, HB + 3)), rng.integers(0, FL, (2, HB + 3))], axis=2)
    hop = _dev(engine, rng.integers(0, 4, (3, 300 + TILE)).astype(np.uint8))
    a = engine.warp_fold_at(d, rows4, col, nlag, warp, [3, 3], nslot).cpu().numpy()
    assert a.tobytes() == engine.warp_fold(d, nlag, warp, [3, 3], nslot).cpu().numpy().tobytes() and np.isfinite(a[0]).all()
    got = [t.cpu().numpy() for t in engine.warp_score_at(d, rows4, col, nlag, warp, [3, 3], nslot, hyp, hop, [0, 0], 300)]
    want = [t.cpu().numpy() for t in engine.warp_score(d, nlag, warp, [3, 3], nslot, hyp, hop, 300)]
    assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)) and (got[1] >= 0).all()
    zeros, rigid = np.zeros((2, 1, TILE + 1), np.int32), [n // FL for n in nlag]
    f = engine.warp_fold_at(d, rows4, col, nlag, zeros, [1, 1], rigid).cpu().numpy()
    assert f[:, 0].tobytes() == engine.phase_fold(d, nlag).cpu().numpy().tobytes()
    phases = rng.integers(0, FL, (2, HB + 3))
    got = [t.cpu().numpy() for t in engine.warp_score_at(d, rows4, col, nlag, zeros, [1, 1], rigid, np.stack([np.zeros_like(phases), phases], axis=2),
                                                         hop, [0, 0], 300)]
    want = [t.cpu().numpy() for t in engine.hop_score(d, nlag, phases, hop, 300)]
    assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)) and (got[1] >= 0).all()


def _graph_inputs(engine, noise):
    recs = [(PERM, SEG, 3 * FL + 11), ((1, 3, 4, 5), 3, 2 * FL + 5)]
    d = _dev(engine, _table(noise, 4 * FL + SEG, recs))
    i32, i64 = (lambda a: _dev(engine, np.array(a, np.int32))), (lambda a: _dev(engine, np.array(a, np.int64)))      # noqa: E731
    warp, nwarp, nslot, hyp, hop = _case(3, HB + 2, 600, 2, 2, 81)
    return (d, i64([r[0] for r in recs]), i64([r[1] for r in recs]), i32([r[2] for r in recs]), i32(warp), i32(nwarp), i32(nslot)), i32(hyp), \
        _dev(engine, hop), i32([1, 0])


def test_two_runs_give_the_same_bits(engine, noise):
    tab, hyp, hop, hop_row = _graph_inputs(engine, noise)
    a = [engine.warp_fold_at(*tab), *engine.warp_score_at(*tab, hyp, hop, hop_row, 600)]
    b = [engine.warp_fold_at(*tab), *engine.warp_score_at(*tab, hyp, hop, hop_row, 600)]
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b)) and bool(torch.isfinite(a[1]).all())


def test_both_calls_record_into_a_graph(engine, noise):
    """Neither call allocates, copies or synchronises: with device inputs they record into a stream capture, and a replay gives the
    eager bits."""
    tab, hyp, hop, hop_row = _graph_inputs(engine, noise)
    want = [engine.warp_fold_at(*tab), *engine.warp_score_at(*tab, hyp, hop, hop_row, 600)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = [engine.warp_fold_at(*tab), *engine.warp_score_at(*tab, hyp, hop, hop_row, 600)]
    torch.cuda.synchronize()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and bool((got[2] >= 0).all()) and bool(torch.isfinite(got[0]).all())


# ---------------------------------------------------------------------------------------------------------------- refusals
def _raw(engine, name, order, args, **over):
    a = dict(args)
    a.update(over)
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                 # noqa: E731
    rc = getattr(engine._lib, name)(engine._ctx, *[p(a[k]) for k in order], engine._stream())
    torch.cuda.synchronize()
    return rc


FOLD_ORDER = ("corr", "rows", "stride", "row", "col", "nlag", "B", "warp", "nwarp", "nslot", "D", "Jw", "fold")
SCORE_ORDER = ("corr", "rows", "stride", "row", "col", "nlag", "B", "warp", "nwarp", "nslot", "D", "Jw", "hyp", "H", "hop", "K", "HR", "Ccols",
               "hop_row", "n_origins", "score", "origin", "rank", "scratch")


@pytest.fixture(scope="module")
def small(engine, noise):
    """A call that works: two records of two slots under two rows, three keys with two hop rows, 300 origins (two chunks), two entries."""
    recs = [(PERM, 3, 2 * FL + 1), ((1, 3, 4, 5), 0, 2 * FL + 1)]
    corr = _table(noise, 2 * FL + 4, recs)
    d = engine.device
    i32, i64 = (lambda a: _dev(engine, np.array(a, np.int32))), (lambda a: _dev(engine, np.array(a, np.int64)))      # noqa: E731
    return dict(recs=recs, corr=_dev(engine, corr), rows=ROWS, stride=2 * FL + 4, row=i64([r[0] for r in recs]), col=i64([3, 0]),
                nlag=i32([2 * FL + 1, 2 * FL + 1]), B=2, warp=i32([[[0, 0], [0, 1]]] * 2), nwarp=i32([2, 2]), nslot=i32([2, 2]), D=2, Jw=2,
                hyp=i32([[(0, 1), (1, 2)], [(1, 3), (0, 4)]]), H=2,
                hop=_dev(engine, np.random.default_rng(51).integers(0, 4, (3, 2, 301)).astype(np.uint8)), K=3, HR=2, Ccols=301, hop_row=i32([1, 0]),
                n_origins=300, fold=torch.empty((2, 2, FL), dtype=torch.float64, device=d), score=torch.empty((2, 3), dtype=torch.float64, device=d),
                origin=torch.empty((2, 3), dtype=torch.int64, device=d), rank=torch.empty((2, 3), dtype=torch.int32, device=d),
                scratch=torch.empty(3 * 2 * 3 * 2, dtype=torch.int64, device=d))


FOLD_REFUSALS = [dict(corr=None), dict(row=None), dict(col=None), dict(nlag=None), dict(warp=None), dict(nwarp=None), dict(nslot=None), dict(fold=None),
                 dict(rows=-1), dict(stride=-1), dict(B=-1), dict(D=-1), dict(Jw=-1), dict(stride=1 << 31), dict(rows=1 << 31), dict(B=1 << 28),
                 dict(D=1 << 29)]
SCORE_REFUSALS = [dict(corr=None), dict(row=None), dict(col=None), dict(nlag=None), dict(warp=None), dict(nwarp=None), dict(nslot=None), dict(hyp=None),
                  dict(hop=None), dict(hop_row=None), dict(score=None), dict(origin=None), dict(rank=None), dict(scratch=None), dict(rows=-8),
                  dict(stride=-1), dict(B=-2), dict(D=-1), dict(Jw=-1), dict(H=-1), dict(K=-3), dict(Ccols=-1), dict(n_origins=-1), dict(HR=0),
                  dict(HR=-1), dict(HR=1 << 31), dict(Ccols=300), dict(n_origins=301), dict(Jw=3), dict(H=0), dict(H=1 << 31), dict(D=1 << 31),
                  dict(stride=1 << 31), dict(rows=1 << 31), dict(n_origins=1 << 40, Ccols=(1 << 40) + 1),
                  dict(K=1 << 30, n_origins=1 << 10, Ccols=(1 << 10) + 1)]


@pytest.mark.parametrize("over", FOLD_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_fold_refusals_write_nothing(engine, small, over):
    small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_warp_fold_at_batch", FOLD_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["fold"] == POISON_F).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_warp_fold_at_batch")


@pytest.mark.parametrize("over", SCORE_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_score_refusals_write_nothing(engine, small, over):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I); small["scratch"].fill_(POISON_I)
    assert _raw(engine, "es_warp_score_at_batch", SCORE_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert (small["scratch"] == POISON_I).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_warp_score_at_batch")


def test_the_accepted_call_and_the_empty_ones(engine, small):
    small["score"].fill_(POISON_F); small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_warp_score_at_batch", SCORE_ORDER, small, B=0) == 0 and _raw(engine, "es_warp_score_at_batch", SCORE_ORDER, small, K=0) == 0
    assert _raw(engine, "es_warp_fold_at_batch", FOLD_ORDER, small, B=0) == 0 and _raw(engine, "es_warp_fold_at_batch", FOLD_ORDER, small, D=0) == 0
    assert (small["score"] == POISON_F).all() and (small["fold"] == POISON_F).all()
    assert _raw(engine, "es_warp_score_at_batch", SCORE_ORDER, small) == 0 and _raw(engine, "es_warp_fold_at_batch", FOLD_ORDER, small) == 0
    corr, hop, warp, hyp = (small[k].cpu().numpy() for k in ("corr", "hop", "warp", "hyp"))
    fold, want = _twin(corr, small["recs"], warp, [2, 2], [2, 2], hyp, hop, [1, 0], 300)
    assert np.array_equal(_bits(small["score"].cpu().numpy()), _bits(want[0])) and np.array_equal(small["origin"].cpu().numpy(), want[1])
    assert np.array_equal(small["rank"].cpu().numpy(), want[2]) and np.array_equal(_bits(small["fold"].cpu().numpy()), _bits(fold))
    with pytest.raises(ValueError):
        engine.warp_fold_at(small["corr"], small["row"][:, :3], small["col"], small["nlag"], small["warp"], [2, 2], [2, 2])       # four rows per record
    with pytest.raises(ValueError):
        engine.warp_score_at(small["corr"], small["row"], small["col"], small["nlag"], small["warp"], [2, 2], [2, 2], small["hyp"], small["hop"],
                             [0], 300)                                      # one hop row per record


# ---------------------------------------------------------------------------------------------------------------- the public calls
def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases, p.skew, p.drift_ppm, p.hypotheses) == \
               (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases, q.skew, q.drift_ppm, q.hypotheses)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


def _feed(mon, streams, clips, cuts):
    """Continue the streams with their clips cut at `cuts`: every piece but the last through the engine's tick alone (what push does
    first), the last through push itself."""
    edges = [0, *cuts]
    for a, b in zip(edges[:-1], edges[1:]):
        mon.engine.monitor_step(mon.table, streams, [c[a:b] for c in clips])
    return mon.push([c[edges[-1]:] for c in clips], streams)


def test_a_stream_shorter_than_its_window_is_the_clip_call(engine):
    """Clip A pushed in uneven chunks into a five-second window: w0 = 0, so the window is the whole stream and the verdict is
    WatermarkDetector.presence on it, field for field, null included -- what tests/test_gpu_presence.py pins."""
    clip = PC.cached("marked", "A")
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    mon = det.open_streams(2)
    _feed(mon, [0], [clip], [20_000, 20_007, 44_007, 68_000, 91_999])
    assert mon.window(0) == (0, clip.size) and mon.table.base_host[0] == 0
    want = det.presence(clip, 48_000, span=PC.SPAN)
    got = mon.presence([0], span=PC.SPAN)
    _same(got[0], want)
    assert want.detected and (want.ctr, want.phase, want.ctr0) == (*PC.FOUND, 1) and want.null.shape == (32,)
    assert mon.presence(span=PC.SPAN)[1] is None and mon.origin(0) is None  # stream 1 has received nothing; a verdict sets no origin
    _same(mon.presence([0], span=PC.SPAN, drift_ppm=300)[0], det.presence(clip, 48_000, span=PC.SPAN, drift_ppm=300))


WINDOW = 8 * SEG
KEYS3 = [PC.OTHER_KEY, PC.KEY, bytes(range(64, 96))]


def _moved(table):
    return dict(n=table.n_host.copy(), base=table.base_host.copy(), origin=table.origin_host.copy(), corr=table.corr_hist.cpu().numpy().tobytes(),
                y=table.y_hist.cpu().numpy().tobytes())


@pytest.fixture(scope="module")
def slid(engine):
    """Two monitors fed alike, until their windows have slid and their rows have been moved down: stream 0 with its counter origin
    (the clip's frame at sample 438 carries counter 1), stream 1 the same audio without one, stream 2 unmarked audio, stream 3 too short
    for a slot, stream 4 closed."""
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    a, u = PC.cached("marked", "A")[:30_000], PC.cached("unmarked", "A")[:30_000]
    mons = []
    for _ in range(2):
        mon = det.open_streams(5, window_s=WINDOW / 48_000, chunk_max=4000, ctr0=[1, None, None, None, None])
        _feed(mon, [0, 1, 2], [a, a, u], [4000, 7999, 8000, 12_000, 15_111, 19_000, 23_000, 26_500])
        mon.push([a[:1000]], [3])
        mon.close([4])
        mons.append(mon)
    tab = mons[0].table
    assert tab.window == WINDOW and mons[0].window(0) == (17 * SEG, 30_000) and (tab.base_host[:3] > 0).all()      # slid, and moved down at least once
    return det, mons[0], mons[1], tab.corr_hist.cpu().numpy()


def _model(tab, hist, s, key=PC.KEY, **kw):
    w0 = int(-(-max(int(tab.n_host[s]) - tab.window, 0) // SEG) * SEG)
    return pr.live_model(hist, s, tab.bands, int(tab.base_host[s]), w0, int(tab.n_host[s]), key,
                         origin=None if tab.origin_host[s] < 0 else int(tab.origin_host[s]), **kw)


def test_a_slid_window_is_the_twin_on_the_history(engine, slid):
    det, mon, _, hist = slid
    tab = mon.table
    before = _moved(tab)
    with_origin = mon.presence([0], span=PC.SPAN)[0]
    _same(with_origin, _model(tab, hist, 0, span=PC.SPAN))
    assert with_origin.frames == 7 and with_origin.ctr in (18, 19) and with_origin.ctr0 == pr.origin_of(with_origin.ctr, with_origin.phase, 17 * SEG)
    without = mon.presence([1], span=PC.SPAN)[0]
    _same(without, _model(tab, hist, 1, span=PC.SPAN))
    assert 0 <= without.ctr < 64 and without.frames == 7
    calls, real = [], engine._call
    engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        both = mon.presence(span=PC.SPAN)
    finally:
        del engine._call
    assert len(both) == 4 and both[3] is None                               # the four open streams; stream 3 has no whole slot
    _same(both[0], with_origin); _same(both[1], without); _same(both[2], _model(tab, hist, 2, span=PC.SPAN))
    assert calls.count("es_warp_fold_at_batch") == 1 and calls.count("es_hop_window_batch") == 1
    assert 1 <= calls.count("es_warp_score_at_batch") <= 2 and set(calls) == {"es_warp_fold_at_batch", "es_hop_window_batch", "es_warp_score_at_batch"}
    sub = mon.presence([2, 0], span=PC.SPAN, phases=3, decoys=5)            # a subset, in the caller's order
    _same(sub[0], _model(tab, hist, 2, span=PC.SPAN, phases=3, decoys=5)); _same(sub[1], _model(tab, hist, 0, phases=3, decoys=5))
    drift = mon.presence([1, 0], span=PC.SPAN, drift_ppm=300)
    _same(drift[0], _model(tab, hist, 1, span=PC.SPAN, drift_ppm=300)); _same(drift[1], _model(tab, hist, 0, drift_ppm=300))
    assert drift[0].hypotheses is not None and len(drift[0].hypotheses) == 8
    with pytest.raises(ValueError, match="closed"):
        mon.presence([4])
    after = _moved(tab)
    assert all(np.array_equal(before[k], after[k]) if isinstance(before[k], np.ndarray) else before[k] == after[k] for k in before)
    assert [mon.origin(s) for s in range(4)] == [1, None, None, None]


def test_a_push_after_presence_is_the_push_of_a_monitor_never_asked(engine, slid):
    det, mon, twin, _ = slid
    mon.presence(span=PC.SPAN)
    nxt = PC.cached("marked", "A")[30_000:33_000]
    got, want = mon.push([nxt, nxt], [0, 1]), twin.push([nxt, nxt], [0, 1])
    assert got == want and mon.traces(0) == twin.traces(0) and mon.session_nonce(0) == twin.session_nonce(0)
    a, b = _moved(mon.table), _moved(twin.table)
    assert all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k] for k in a)


def test_live_identifier_entry_k_is_the_live_monitor_of_key_k(engine):
    a = PC.cached("marked", "A")[:30_000]
    cuts = [4000, 7999, 11_999, 15_111, 19_000, 23_000, 26_500]
    ident = WatermarkIdentifier(KEYS3, list_size=8, engine=engine)
    live = ident.open_streams(3, window_s=WINDOW / 48_000, chunk_max=4000, memo_slots=0, ctr0=[1, None, None])
    for lo, hi in zip([0, *cuts], [*cuts, a.size]):
        engine.monitor_step(live.table, [0, 1], [a[lo:hi], a[lo:hi]])
    stats = dict(live.stats)
    got = live.presence(span=PC.SPAN)
    assert len(got) == 3 and got[2] is None and all(len(g) == 3 for g in got[:2]) and live.stats == stats
    for k, key in enumerate(KEYS3):
        mon = WatermarkDetector(key, list_size=8, engine=engine).open_streams(3, window_s=WINDOW / 48_000, chunk_max=4000, ctr0=[1, None, None])
        for lo, hi in zip([0, *cuts], [*cuts, a.size]):
            engine.monitor_step(mon.table, [0, 1], [a[lo:hi], a[lo:hi]])
        want = mon.presence(span=PC.SPAN)
        _same(got[0][k], want[0]); _same(got[1][k], want[1])
        assert want[2] is None and sorted(mon.table.bands.tolist()) == [0, 1, 2, 3]
    calls, real = [], engine._call
    engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        live.presence([1], span=PC.SPAN)
    finally:
        del engine._call
    assert calls == ["es_warp_fold_at_batch", "es_hop_window_batch", "es_warp_score_at_batch"]     # one score launch covers all keys


def test_identifier_entry_k_is_the_detector_of_key_k(engine):
    from scipy.signal import resample_poly
    a = PC.cached("marked", "A")
    clips = [a[:40_000], (resample_poly(a[:30_000].astype(np.float64), 147, 160) * 32768).astype(np.int16), a[:1000]]
    rates = [48_000, 44_100, 48_000]
    ident = WatermarkIdentifier(KEYS3, list_size=8, engine=engine)
    got = ident.presence_batch(clips, rates, span=PC.SPAN)
    drift = ident.presence_batch(clips, rates, [1, None, None], span=PC.SPAN, phases=4, decoys=7, drift_ppm=300)
    assert got[2] is None and drift[2] is None
    for k, key in enumerate(KEYS3):
        det = WatermarkDetector(key, list_size=8, engine=engine)
        want = det.presence_batch(clips, rates, span=PC.SPAN)
        want_drift = det.presence_batch(clips, rates, [1, None, None], span=PC.SPAN, phases=4, decoys=7, drift_ppm=300)
        for c in range(2):
            _same(got[c][k], want[c]); _same(drift[c][k], want_drift[c])
    _same(ident.presence(clips[0], 48_000, span=PC.SPAN)[1], got[0][1])
