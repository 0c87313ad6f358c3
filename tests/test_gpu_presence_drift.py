"""GPU: the presence test under sample-clock drift -- es_warp_fold_batch and es_warp_score_batch bit for bit (uint64 views)
against their host twin (presence.warp_fold_model / warp_score_model) on the very rows and tables the kernels read, at the edges of the
hypothesis block (ES_WARP_HB), the slot tile and the origin chunk; unusable rows; a table of zeros against the rigid calls; every
refusal with its outputs unwritten; capture and replay; and WatermarkDetector.presence(..., drift_ppm=...) field for field against the
twin on the downloaded rows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector

FL, TILE, CHUNK, HB = 1215, nat.ES_HOP_TILE, nat.ES_HOP_ORIGINS, nat.ES_WARP_HB
POISON_F, POISON_I = -777.25, -77


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)       # (a copy: the shared rows are read-only)


def _rows(seed, nlags, stride, negative=False):
    """Four random rows per clip in (-1, 1), NaN in every column at or past the clip's nlag."""
    corr = np.random.default_rng(seed).uniform(-1.0, 1.0, (4 * len(nlags), stride))
    if negative:
        corr = -np.abs(corr) - 0.25
    for b, n in enumerate(nlags):
        corr[4 * b:4 * b + 4, max(n, 0):] = np.nan
    return corr


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ramp(J, e):
    """Offsets of a grid that ends e samples off the rigid one: j e / J rounded half up, as presence.skew_table has them."""
    j = np.arange(J, dtype=np.int64)
    return (2 * j * e + J) // (2 * J) if J else j


def _fold_equals_twin(engine, corr, nlag, warp, nwarp, nslot):
    got = engine.warp_fold(_dev(engine, corr), nlag, np.asarray(warp, np.int32), nwarp, nslot).cpu().numpy()
    want = pr.warp_fold_model(corr, nlag, warp, nwarp, nslot)
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), (got, want)
    return got


def _score_equals_twin(engine, corr, nlag, warp, nwarp, nslot, hyp, hop, n_origins):
    got = [t.cpu().numpy() for t in engine.warp_score(_dev(engine, corr), nlag, np.asarray(warp, np.int32), nwarp, nslot,
                                                      np.asarray(hyp, np.int32), _dev(engine, hop), n_origins)]
    want = pr.warp_score_model(corr, nlag, warp, nwarp, nslot, hyp, hop, n_origins)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    return got


# ---------------------------------------------------------------------------------------------------------------- the fold
@pytest.mark.parametrize("D", [1, 2, 5])
def test_fold_equals_the_twin_at_every_slot_count(engine, D):
    """nlag 1215, 2 * 1215 + 7 and 5 * 1215 in one call under D rows of positive and negative offsets, NaN past every nlag; then rows
    made unusable at the first slot, at the last slot and by nwarp, which must come out -inf without a NaN being read."""
    nlag = [FL, 2 * FL + 7, 5 * FL]
    corr = _rows(60 + D, nlag, 5 * FL + 3)
    J = [1, 2, 4]                                                           # a slot less than 5 * 1215 holds: room for the offsets
    skews = [0, -3, 3, -1214, 1214][:D]
    warp = np.zeros((3, D, 4), np.int64)
    for b in (1, 2):
        warp[b] = [np.pad(_ramp(J[b], e if b == 2 else e % 8 if e > 0 else -(-e % 8)), (0, 4 - J[b])) for e in skews]
    got = _fold_equals_twin(engine, corr, nlag, warp, [D] * 3, J)
    assert np.isfinite(got).all() and np.abs(got).min() > 0
    if D > 1:
        assert not np.array_equal(got[2, 0], got[2, 1]) and (warp[2, 1] <= 0).all() and warp[2, 1, 3] == -2
    if D == 5:
        assert warp[2, 3].tolist() == [0, -303, -607, -910] and warp[2, 4, 3] == 911 and warp[1, 2].tolist() == [0, 2, 0, 0]
    bad = warp.copy()
    bad[0, 0, 0] = 1                                                        # clip 0: one sample past its only slot's room
    bad[1, 0, 0] = -1                                                       # clip 1, row 0: before lag 0 at the first slot
    bad[2, D - 1, 3] = FL + 1                                               # clip 2, last row: past the clip at the last slot
    nwarp = [D, D, D] if D == 1 else [D, D - 1, D]
    out = _fold_equals_twin(engine, corr, nlag, bad, nwarp, J)
    assert np.isneginf(out[0, 0]).all() and np.isneginf(out[1, 0]).all() and np.isneginf(out[2, D - 1]).all()
    if D > 1:
        assert np.isneginf(out[1, D - 1]).all() and np.array_equal(_bits(out[2, :D - 1]), _bits(got[2, :D - 1]))
        assert np.array_equal(_bits(out[0, 1:]), _bits(got[0, 1:]))
    wild = np.full_like(warp, 2 ** 31 - 1); wild[:, :, 1::2] = -2 ** 31     # whatever the table holds, nothing outside the rows is read
    assert np.isneginf(_fold_equals_twin(engine, corr, nlag, wild, [D] * 3, J)).all()
    none = _fold_equals_twin(engine, corr, nlag, wild, [D, 0, D], [0, 2, -7])                       # J == 0: zeros in every usable row
    assert not none[0].any() and not none[2].any() and np.isneginf(none[1]).all()


def test_fold_walks_more_slots_than_one_table_tile(engine):
    """The offsets pass through LDS 256 slots at a time: 300 slots, an unusable slot in the second tile alone."""
    J = 300
    nlag = [J * FL + 40, J * FL + 40]
    corr = _rows(66, nlag, J * FL + 40)
    warp = np.stack([np.stack([_ramp(J, 0), _ramp(J, 40), _ramp(J, -40)])] * 2)
    warp[1, 2, 299] = 41
    got = _fold_equals_twin(engine, corr, nlag, warp, [3, 3], [J, J])
    assert np.isfinite(got[0]).all() and np.isfinite(got[1, :2]).all() and np.isneginf(got[1, 2]).all()


# ---------------------------------------------------------------------------------------------------------------- the score
SCORE_J = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 2)
SKEWS = (0, 5, -5)


@pytest.fixture(scope="module")
def score_rows():
    """Per J: two clips (J slots and about half of them) in rows of stride > nlag and their table of three rows (skews 0, +5, -5), shared
    by the cases and left unchanged."""
    out = {}
    for J in SCORE_J:
        nlag = [J * FL + 5, (J // 2) * FL + 1214]
        corr = _rows(70 + J, nlag, J * FL + 9)
        corr.setflags(write=False)
        nslot = [J, max((nlag[1] - 5) // FL, 0)]
        warp = np.stack([np.stack([np.pad(_ramp(n, e), (0, J - n)) for e in SKEWS]) for n in nslot])
        out[J] = (corr, nlag, warp, [3, 3], nslot)
    return out


@pytest.mark.parametrize("J", SCORE_J)
@pytest.mark.parametrize("n_origins", [1, CHUNK - 1, CHUNK, CHUNK + 1])
@pytest.mark.parametrize("H", [1, HB - 1, HB, HB + 1, 2 * HB + 1])
def test_score_equals_the_twin(engine, score_rows, H, n_origins, J):
    assert SCORE_J == (1, 63, 64, 65, 130)
    corr, nlag, warp, nwarp, nslot = score_rows[J]
    rng = np.random.default_rng(1000 * H + 10 * n_origins + J)
    hyp = np.stack([rng.integers(0, 3, (2, H)), rng.integers(0, FL, (2, H))], axis=2)
    hop = rng.integers(0, 4, (3, n_origins + J - 1)).astype(np.uint8)
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, nwarp, nslot, hyp, hop, n_origins)
    assert np.isfinite(score[0]).all() and (origin[0] >= 0).all() and (origin[0] < n_origins).all() and (rank[0] >= 0).all()
    if J == 1:
        assert np.isneginf(score[1]).all() and (origin[1] == -1).all() and (rank[1] == -1).all()        # the second clip has no slot


def _flat(J, pad=4):
    """A clip whose band 3 holds 0.9 at every lag and the others -0.5, with a table of the rigid row and a row one sample late."""
    corr = np.full((4, J * FL + pad), -0.5)
    corr[3, :J * FL + 1] = 0.9
    corr[:, J * FL + 1:] = np.nan
    return corr, [J * FL + 1], np.stack([np.zeros(J, np.int64), np.ones(J, np.int64)])[None]


def test_identical_windows_the_lower_origin_then_the_earlier_entry_wins(engine):
    """Equal scores inside a block of origins and across two, inside a block of hypotheses and across two."""
    J, n = 3, CHUNK + 60
    corr, nlag, warp = _flat(J)
    hop = np.zeros((3, n + J - 1), np.uint8)
    hop[0, :] = np.arange(n + J - 1) % 2 * 3                                # key 0: origins of one parity share a window, in and across chunks
    hop[1, 5:8] = 3; hop[1, CHUNK + 4:CHUNK + 7] = 3                        # key 1: origins 5 and 260, one per chunk
    hop[2, 100:103] = 3; hop[2, 200:203] = 3                                # key 2: origins 100 and 200 of one chunk
    hyp = [[(0, 17), (1, 17), (0, 18)] + [(1, 40 + e) for e in range(HB)]]  # every entry scores the same: HB + 3 entries, two blocks
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [2], [J], hyp, hop, n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [0, 0, 0]
    assert score[0, 1] == score[0, 2] == (0.9 + 0.9 + 0.9) / 3
    late = [[(0, 17)] * (HB + 2)]                                           # the best entry is in the second block, named there twice
    corr2 = corr.copy(); corr2[3, [18, 18 + FL, 18 + 2 * FL]] = 0.95
    late[0][HB] = late[0][HB + 1] = (1, 17)
    score, origin, rank = _score_equals_twin(engine, corr2, nlag, warp, [2], [J], late, hop, n)
    assert rank[0].tolist() == [HB, HB, HB] and origin[0].tolist() == [1, 5, 100] and score[0, 1] == score[0, 2] == (0.95 + 0.95 + 0.95) / 3


def test_an_entry_named_twice_the_earlier_one_wins(engine, score_rows):
    corr, nlag, warp, nwarp, nslot = score_rows[TILE + 1]
    hop = np.random.default_rng(81).integers(0, 4, (3, 70 + TILE)).astype(np.uint8)
    for H in (3, HB + 3):
        hyp = [[(1, 700)] * H, [(2, 9)] * H]
        _, _, rank = _score_equals_twin(engine, corr, nlag, warp, nwarp, nslot, hyp, hop, 70)
        assert not rank.any()
        hyp[0][0] = (0, 3)
        _, _, rank = _score_equals_twin(engine, corr, nlag, warp, nwarp, nslot, hyp, hop, 70)
        assert set(rank[0].tolist()) <= {0, 1} and not rank[1].any()


def test_all_scores_negative_the_best_does_not_start_at_zero(engine):
    nlag = [(TILE + 1) * FL + 3, 2 * FL + 3]
    corr = _rows(82, nlag, (TILE + 1) * FL + 4, negative=True)
    warp = np.stack([np.stack([np.pad(_ramp(n, e), (0, TILE + 1 - n)) for e in (0, 3, -3)]) for n in (TILE + 1, 2)])
    hop = np.random.default_rng(83).integers(0, 4, (3, 65 + TILE)).astype(np.uint8)
    hyp = np.stack([np.random.default_rng(84).integers(0, 3, (2, HB + 1)), np.random.default_rng(85).integers(0, FL, (2, HB + 1))], axis=2)
    score, origin, _ = _score_equals_twin(engine, corr, nlag, warp, [3, 3], [TILE + 1, 2], hyp, hop, 65)
    assert (score < -0.25).all() and (origin >= 0).all()


def test_a_missing_counter_excludes_exactly_the_windows_that_touch_it(engine):
    J, n = 5, CHUNK + 20
    nlag = [J * FL + 2]
    corr = _rows(86, nlag, J * FL + 2)
    corr[:, :nlag[0]] = -0.5
    warp = np.stack([_ramp(J, 0), _ramp(J, 2)])[None]
    hop = np.random.default_rng(87).integers(0, 4, (3, n + J - 1)).astype(np.uint8)
    for j in range(J):                                                      # key 0: the best window is the one at origin 98, on row 1 ...
        corr[hop[0, 98 + j], 40 + FL * j + warp[0, 1, j]] = 0.9
    hyp = [[(0, 40), (1, 40)]]
    free = _score_equals_twin(engine, corr, nlag, warp, [2], [J], hyp, hop, n)
    assert free[1][0, 0] == 98 and free[2][0, 0] == 1
    hop[0, 100] = 0xFF                                                      # ... which holds column 100: origins 96 .. 100 are out
    hop[1, n + J - 2] = 0xFF                                                # key 1: the last column, touched by the last origin alone
    hop[2, :] = 0xFF                                                        # key 2: nothing to score
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [2], [J], hyp, hop, n)
    assert origin[0, 0] not in range(96, 101) and origin[0, 0] >= 0 and origin[0, 1] != n - 1
    assert np.isneginf(score[0, 2]) and origin[0, 2] == -1 and rank[0, 2] == -1


def test_no_slot_no_origin_and_no_usable_entry_give_nothing(engine):
    nlag = [1214, 2 * FL + 1]
    corr = _rows(88, nlag, 2 * FL + 1)
    warp = np.array([[[0, 0], [0, 1], [0, 2]]] * 2)                         # row 2 leaves the second clip at its last slot
    hop = np.random.default_rng(89).integers(0, 4, (3, 12)).astype(np.uint8)
    hyp = [[(0, 3), (1, 4)], [(0, 5), (1, 6)]]
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [3, 3], [2, 2], hyp, hop, 11)
    assert np.isneginf(score[0]).all() and (origin[0] == -1).all() and (rank[0] == -1).all() and (origin[1] >= 0).all()     # J == 0
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [3, 3], [2, 0], hyp, hop, 11)                          # nslot 0
    assert np.isneginf(score).all() and (origin == -1).all() and (rank == -1).all()
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [3, 3], [2, 2], hyp, hop, 0)                           # an empty span
    assert np.isneginf(score).all() and (origin == -1).all() and (rank == -1).all()
    nothing = [[(0, 3)] * 3, [(2, 5), (3, 6), (-1, 7)]]                     # unusable, past D, negative
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [3, 3], [2, 2], nothing, hop, 11)
    assert np.isneginf(score).all() and (origin == -1).all() and (rank == -1).all()
    by_nwarp = _score_equals_twin(engine, corr, nlag, warp, [3, 1], [2, 2], [[(0, 3)], [(1, 6)]], hop, 11)                   # row 1 >= nwarp
    assert (by_nwarp[1] == -1).all()


def test_an_unusable_entry_between_usable_ones_is_skipped(engine):
    """Row 1 leaves the clip at its last slot, in the second slot tile, and row 3 everywhere: entries on them, entries past the table and
    entries that are no phase sit between usable ones, inside one block of hypotheses and across two."""
    J = TILE + 2
    nlag = [J * FL + 1]
    corr = _rows(90, nlag, J * FL + 3)
    warp = np.stack([_ramp(J, 0), _ramp(J, 0), _ramp(J, 1), np.full(J, 2 ** 31 - 1)])[None]
    warp[0, 1, J - 1] = 2
    hop = np.random.default_rng(91).integers(0, 4, (3, 30 + J - 1)).astype(np.uint8)
    hyp = [[(0, 7), (1, 7), (2, 7), (3, 7), (0, FL), (0, -1), (4, 7), (-1, 7), (2, 1214), (0, 8)]]
    score, origin, rank = _score_equals_twin(engine, corr, nlag, warp, [4], [J], hyp, hop, 30)
    assert np.isfinite(score).all() and set(rank[0].tolist()) <= {0, 2, 8, 9}
    alone = _score_equals_twin(engine, corr, nlag, warp, [4], [J], [[(0, 7), (2, 7), (2, 1214), (0, 8)]], hop, 30)
    assert np.array_equal(_bits(alone[0]), _bits(score)) and np.array_equal(alone[1], origin)


def test_a_table_of_zeros_gives_the_rigid_calls(engine):
    nlag = [(TILE + 1) * FL + 11, 3 * FL, 1000]
    corr = _rows(92, nlag, (TILE + 1) * FL + 11)
    d = _dev(engine, corr)
    zeros, nwarp, nslot = np.zeros((3, 1, TILE + 1), np.int32), [1, 1, 1], [n // FL for n in nlag]
    fold = engine.warp_fold(d, nlag, zeros, nwarp, nslot).cpu().numpy()
    assert np.array_equal(_bits(fold[:, 0]), _bits(engine.phase_fold(d, nlag).cpu().numpy()))
    rng = np.random.default_rng(93)
    phases = rng.integers(0, FL, (3, HB + 3))
    hop = _dev(engine, rng.integers(0, 4, (3, 300 + TILE)).astype(np.uint8))
    want = [t.cpu().numpy() for t in engine.hop_score(d, nlag, phases, hop, 300)]
    hyp = np.stack([np.zeros_like(phases), phases], axis=2)
    got = [t.cpu().numpy() for t in engine.warp_score(d, nlag, zeros, nwarp, nslot, hyp, hop, 300)]
    assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want)) and (got[1][:2] >= 0).all() and (got[1][2] == -1).all()


def test_two_runs_give_the_same_bits(engine, score_rows):
    corr, nlag, warp, nwarp, nslot = score_rows[TILE + 1]
    d, hop = _dev(engine, corr), _dev(engine, np.random.default_rng(94).integers(0, 4, (3, 600 + TILE)).astype(np.uint8))
    hyp = np.stack([np.random.default_rng(95).integers(0, 3, (2, HB + 2)), np.random.default_rng(96).integers(0, FL, (2, HB + 2))], axis=2)
    a = [t.cpu().numpy() for t in engine.warp_score(d, nlag, warp, nwarp, nslot, hyp, hop, 600)]
    b = [t.cpu().numpy() for t in engine.warp_score(d, nlag, warp, nwarp, nslot, hyp, hop, 600)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    f = engine.warp_fold(d, nlag, warp, nwarp, nslot).cpu().numpy()
    assert f.tobytes() == engine.warp_fold(d, nlag, warp, nwarp, nslot).cpu().numpy().tobytes()


def test_both_calls_record_into_a_graph(engine):
    """Neither call allocates, copies or synchronises: with device inputs they record into a stream capture, and a replay gives the
    eager bits."""
    nlag = [3 * FL + 11]
    d = _dev(engine, _rows(97, nlag, 3 * FL + 11))
    i32 = lambda a: _dev(engine, np.array(a, np.int32))                     # noqa: E731
    nl, warp, nwarp, nslot = i32(nlag), i32([[[0, 0, 0], [0, 2, 4], [0, -2, -4]]]), i32([3]), i32([3])
    hyp = i32([[(1, 5), (2, 700), (0, 9)]])
    hop = _dev(engine, np.random.default_rng(98).integers(0, 4, (3, 300 + 2)).astype(np.uint8))
    want = [engine.warp_fold(d, nl, warp, nwarp, nslot), *engine.warp_score(d, nl, warp, nwarp, nslot, hyp, hop, 300)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = [engine.warp_fold(d, nl, warp, nwarp, nslot), *engine.warp_score(d, nl, warp, nwarp, nslot, hyp, hop, 300)]
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


FOLD_ORDER = ("corr", "rows", "stride", "nlag", "B", "warp", "nwarp", "nslot", "D", "Jw", "fold")
SCORE_ORDER = ("corr", "rows", "stride", "nlag", "B", "warp", "nwarp", "nslot", "D", "Jw", "hyp", "H", "hop", "K", "Ccols", "n_origins",
               "score", "origin", "rank", "scratch")


@pytest.fixture(scope="module")
def small(engine):
    """A call that works: two clips of two slots under two rows, three keys, 300 origins (two chunks), two entries."""
    corr = _rows(50, [2 * FL + 1, 2 * FL + 1], 2 * FL + 1)
    d = engine.device
    i32 = lambda a: _dev(engine, np.array(a, np.int32))                     # noqa: E731
    return dict(corr=_dev(engine, corr), rows=8, stride=2 * FL + 1, nlag=i32([2 * FL + 1, 2 * FL + 1]), B=2,
                warp=i32([[[0, 0], [0, 1]]] * 2), nwarp=i32([2, 2]), nslot=i32([2, 2]), D=2, Jw=2, hyp=i32([[(0, 1), (1, 2)], [(1, 3), (0, 4)]]), H=2,
                hop=_dev(engine, np.random.default_rng(51).integers(0, 4, (3, 301)).astype(np.uint8)), K=3, Ccols=301, n_origins=300,
                fold=torch.empty((2, 2, FL), dtype=torch.float64, device=d), score=torch.empty((2, 3), dtype=torch.float64, device=d),
                origin=torch.empty((2, 3), dtype=torch.int64, device=d), rank=torch.empty((2, 3), dtype=torch.int32, device=d),
                scratch=torch.empty(3 * 2 * 3 * 2, dtype=torch.int64, device=d))


FOLD_REFUSALS = [dict(corr=None), dict(nlag=None), dict(warp=None), dict(nwarp=None), dict(nslot=None), dict(fold=None), dict(rows=-1), dict(stride=-1),
                 dict(B=-1), dict(D=-1), dict(Jw=-1), dict(rows=7), dict(stride=1 << 31), dict(B=1 << 28, rows=1 << 30), dict(D=1 << 29)]
SCORE_REFUSALS = [dict(corr=None), dict(nlag=None), dict(warp=None), dict(nwarp=None), dict(nslot=None), dict(hyp=None), dict(hop=None),
                  dict(score=None), dict(origin=None), dict(rank=None), dict(scratch=None), dict(rows=-8), dict(stride=-1), dict(B=-2), dict(D=-1),
                  dict(Jw=-1), dict(H=-1), dict(K=-3), dict(Ccols=-1), dict(n_origins=-1), dict(rows=7), dict(Ccols=300), dict(n_origins=301),
                  dict(Jw=3), dict(H=0), dict(H=1 << 31), dict(D=1 << 31), dict(stride=1 << 31), dict(n_origins=1 << 40, Ccols=(1 << 40) + 1),
                  dict(K=1 << 30, n_origins=1 << 10, Ccols=(1 << 10) + 1)]


@pytest.mark.parametrize("over", FOLD_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_fold_refusals_write_nothing(engine, small, over):
    small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_warp_fold_batch", FOLD_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["fold"] == POISON_F).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_warp_fold_batch")


@pytest.mark.parametrize("over", SCORE_REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_score_refusals_write_nothing(engine, small, over):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I); small["scratch"].fill_(POISON_I)
    assert _raw(engine, "es_warp_score_batch", SCORE_ORDER, small, **over) == nat.ES_EINVAL
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert (small["scratch"] == POISON_I).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_warp_score_batch")


def test_the_accepted_call_and_the_empty_ones(engine, small):
    small["score"].fill_(POISON_F); small["fold"].fill_(POISON_F)
    assert _raw(engine, "es_warp_score_batch", SCORE_ORDER, small, B=0) == 0 and _raw(engine, "es_warp_score_batch", SCORE_ORDER, small, K=0) == 0
    assert _raw(engine, "es_warp_fold_batch", FOLD_ORDER, small, B=0) == 0 and _raw(engine, "es_warp_fold_batch", FOLD_ORDER, small, D=0) == 0
    assert (small["score"] == POISON_F).all() and (small["fold"] == POISON_F).all()
    assert _raw(engine, "es_warp_score_batch", SCORE_ORDER, small) == 0 and _raw(engine, "es_warp_fold_batch", FOLD_ORDER, small) == 0
    corr, hop, warp, hyp = (small[k].cpu().numpy() for k in ("corr", "hop", "warp", "hyp"))
    want = pr.warp_score_model(corr, [2 * FL + 1] * 2, warp, [2, 2], [2, 2], hyp, hop, 300)
    assert np.array_equal(_bits(small["score"].cpu().numpy()), _bits(want[0])) and np.array_equal(small["origin"].cpu().numpy(), want[1])
    assert np.array_equal(small["rank"].cpu().numpy(), want[2])
    assert np.array_equal(_bits(small["fold"].cpu().numpy()), _bits(pr.warp_fold_model(corr, [2 * FL + 1] * 2, warp, [2, 2], [2, 2])))
    with pytest.raises(ValueError):
        engine.warp_fold(small["corr"], [1, 2], small["warp"], [2, 2, 2], [2, 2])      # one nwarp per clip
    with pytest.raises(ValueError):
        engine.warp_score(small["corr"], [1, 2], small["warp"], [2, 2], [2, 2], small["hyp"][:, :, :1], small["hop"], 300)


# ---------------------------------------------------------------------------------------------------------------- end to end
def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases, p.skew, p.drift_ppm, p.hypotheses) == \
               (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases, q.skew, q.drift_ppm, q.hypotheses)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


@pytest.fixture(scope="module")
def drifted():
    """Clip B captured on a clock 100 ppm fast: resampled by 10001/10000."""
    from scipy.signal import resample_poly
    clip = resample_poly(PC.cached("marked", "B").astype(np.float64), 10001, 10000).astype(np.float32)
    clip.setflags(write=False)
    return clip


def test_presence_follows_the_drift_and_is_the_twin(engine, drifted):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    nonce = det.session_nonce
    rigid = det.presence(drifted, 48_000, span=PC.SPAN, phases=8, decoys=32)
    got = det.presence(drifted, 48_000, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300)
    (_, _, _), (ids, corr, nlag) = det._presence_rows
    assert ids == [0] and corr.shape[0] == 4 and int(nlag[0]) == drifted.size - 62 and det.session_nonce is nonce and det._trace is None
    _same(got, pr.presence_model(corr, int(nlag[0]), PC.KEY, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300))
    _same(rigid, pr.presence_model(corr, int(nlag[0]), PC.KEY, span=PC.SPAN, phases=8, decoys=32))
    print(f"B + 100 ppm: rigid {rigid.score:.4f} / {rigid.null.max():.4f}; searched {got.score:.4f} / {got.null.max():.4f} at skew {got.skew}")
    assert not rigid.detected and got.detected and (got.ctr, got.phase) == PC.FOUND and abs(got.skew - 10) <= 1 and len(got.hypotheses) == 8
    by_origin = det.presence(drifted, 48_000, 1, phases=3, decoys=5, drift_ppm=300)                 # the origin known: span (1, 3)
    _same(by_origin, pr.presence_model(corr, int(nlag[0]), PC.KEY, span=(1, 3), phases=3, decoys=5, drift_ppm=300))
    assert by_origin.detected and by_origin.score == got.score and by_origin.skew == got.skew


def test_drift_zero_is_the_call_without_the_argument(engine):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det.presence(PC.cached("marked", "A"), 48_000, span=PC.SPAN)               # the decoy ring is derived once, here
    calls = []
    real = engine._call
    engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        a = det.presence(PC.cached("marked", "A"), 48_000, span=PC.SPAN)
        plain, calls[:] = list(calls), []
        b = det.presence(PC.cached("marked", "A"), 48_000, span=PC.SPAN, drift_ppm=0)
        c = det.presence(PC.cached("marked", "A"), 48_000, span=PC.SPAN, drift_ppm=0.0)
    finally:
        del engine._call
    _same(a, b); _same(a, c)
    assert calls == plain + plain and not any("warp" in n for n in calls) and "es_hop_score_batch" in plain
    assert (a.skew, a.drift_ppm, a.hypotheses) == (0, 0.0, None) and a.detected


def test_presence_batch_with_drift_is_the_single_calls(engine, drifted):
    from scipy.signal import resample_poly
    a = drifted
    clips = [a, a[:40_000], resample_poly(a, 147, 160).astype(np.float32), a[:1000], (a[:30_000] * 32768).astype(np.int16)]
    rates = [48_000, 48_000, 44_100, 48_000, 48_000]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    batch = det.presence_batch(clips, rates, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300)
    assert batch[3] is None and batch[0].detected and batch[0].skew in (9, 10, 11) and batch[1].frames == (40_000 - 62 - 12) // FL
    for clip, fs, got in zip(clips, rates, batch):
        _same(got, det.presence(clip, fs, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300))
    mixed = det.presence_batch(clips[:2], 48_000, [1, None], span=PC.SPAN, phases=8, decoys=32, drift_ppm=300)   # an origin for the first clip alone
    _same(mixed[0], det.presence(clips[0], 48_000, 1, phases=8, decoys=32, drift_ppm=300))
    _same(mixed[1], batch[1])
    assert det.presence_batch([], 48_000, drift_ppm=300) == []
