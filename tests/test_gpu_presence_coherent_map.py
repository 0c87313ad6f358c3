"""GPU: the coherent presence timeline -- es_coherent_score_at_batch bit for bit (uint64 views) against its host twin
(echoseal_amd/presence.py coherent_score_at_model) on the very arrays the kernel reads, with NaN wherever it must not read, against
es_coherent_score_batch where the rows are the implied ones, every refusal with its outputs unwritten, and
WatermarkDetector.presence_coherent_map / WatermarkIdentifier's four coherent calls field for field against the twin on the downloaded
rows and against each other, with the launches counted."""
from unittest import mock

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd import presence_search as ps
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

FL, CT, CHUNK = 1215, nat.ES_COH_TILE, nat.ES_HOP_ORIGINS
POISON_F, POISON_I = -777.25, -77
AT = "es_coherent_score_at_batch"
C_CLIP = (0.2, 5.0, 7, 108)                                                 # clip C of DESIGN 4.23 (tests/test_presence_coherent_map_host.py)
CUT_AT, CUT_LEN = 60_000, 12_650                                            # the 3 s variant of DESIGN 4.28
SMALL = dict(span=(0, 14), decoys=2)


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def rings(engine):
    keys = [PC.KEY] + pr.decoy_keys(2)
    return {K: (engine.keyring(keys[:K]), pr.header_signs(keys[:K])) for K in (1, 3)}


def _hop(rng, K, bases, cols):
    """Hop rows shaped as es_hop_window_batch shapes them: [K, HR, cols], 0xFF where base + column is no counter."""
    hop = rng.integers(0, 4, (K, len(bases), cols)).astype(np.uint8)
    for h, base in enumerate(bases):
        hop[:, h, max(2 ** 32 - base, 0):] = 0xFF
    return hop


def _at_equals_twin(engine, ring_u, tabs, rows4, col, nslot, phases, hop, hop_row, lo, n_origins, dev_tabs=None):
    ring, u = ring_u
    dev_tabs = dev_tabs or [_dev(engine, t) for t in tabs]
    got = [t.cpu().numpy() for t in engine.coherent_score_at(*dev_tabs, np.asarray(rows4, np.int64), np.asarray(col, np.int64), nslot,
                                                             np.asarray(phases, np.int32), ring, _dev(engine, hop), hop_row, lo, n_origins)]
    want = pr.coherent_score_at_model(*tabs, rows4, col, nslot, max(max(nslot), 0), phases, u, hop, hop_row, lo, n_origins)
    assert got[0].dtype == np.float64 and got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    return got


def _tables(seed, rows, stride):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((rows, stride))
    A = rng.standard_normal((rows, stride)) * 8
    D = np.abs(rng.standard_normal((rows, stride))) + 0.5
    return [M, A, D]


@pytest.fixture(scope="module")
def at_tables(engine):
    """Per J: six rows of 190 + 1215 J + 900 columns, made once, left unchanged, uploaded once."""
    out = {}
    for J in (1, CT - 1, CT, CT + 1, 40):
        tabs = _tables(300 + J, 6, 190 + FL * J + 900)
        for t in tabs:
            t.setflags(write=False)
        out[J] = (tabs, [_dev(engine, t) for t in tabs])
    return out


def _records(J, n_origins):
    """Seven records of a table of 190 + 1215 J + 900 columns: columns that are no multiple of 1215; two records that share rows and
    overlap; three whose nslot is clamped: where stride - col - 190 == 1215 J exactly (col 900), a column further (901: J - 1 slots)
    and a column nearer (899: 1215 J + 1, still J); one with a row outside the table; one with a hop row outside [0, HR).  A counter
    base per hop row: one whose windows cross a multiple of 65 536, one of 256 alone, one whose last origin runs past 2^32 - 1 (a 0xFF
    byte), one that crosses 256 across the slots of origin 0."""
    rows4 = [[0, 1, 2, 3], [0, 1, 2, 3], [5, 3, 4, 0], [2, 2, 1, 1], [3, 2, 1, 0], [0, 1, 2, 6], [0, 1, 2, 3]]
    col, nslot = [7, 331, 900, 901, 899, 7, 7], [J, J, J + 3, J, J + 3, J, J]
    bases = [65536 * 3 - 20 - J // 2, 250, 2 ** 32 - n_origins - J + 2, 255]
    hop_row = [0, 1, 2, 3, 1, 0, 4]
    return rows4, col, nslot, bases, hop_row


@pytest.mark.parametrize("J", [1, CT - 1, CT, CT + 1, 40])
@pytest.mark.parametrize("n_origins", [1, 63, 64, 65, 256, 257])
def test_the_kernel_equals_the_twin(engine, rings, at_tables, n_origins, J):
    """Slot counts around the LDS tile of 16 slots and the window's 40; origins around a wave, at one block and past it; K and P alternate."""
    tabs, dev_tabs = at_tables[J]
    K, P = (3 if n_origins % 2 else 1), (1 if J % 2 == 0 else 3)
    rng = np.random.default_rng(1000 * n_origins + J)
    rows4, col, nslot, bases, hop_row = _records(J, n_origins)
    hop = _hop(rng, K, bases, n_origins + (J + 3) - 1)
    phases = rng.integers(0, FL, (7, P))
    if P == 3:
        phases[1, 1], phases[3, 0] = -1, FL                                 # entries that are no phase
    phases[0, 0], phases[2, -1] = 1214, 0
    lo = [bases[h] if h < 4 else 0 for h in hop_row]
    score, origin, rank = _at_equals_twin(engine, rings[K], tabs, rows4, col, nslot, phases, hop, hop_row, lo, n_origins, dev_tabs)
    assert np.isfinite(score[:2]).all() and (origin[:2] >= 0).all() and (origin[:3] < n_origins).all()
    assert (origin[2] <= n_origins - 2).all() and ((origin[2] >= 0) == (n_origins > 1)).all()       # the last origin's last counter would be 2^32
    assert (np.isfinite(score[3]) == (J > 1)).all()                         # a column further: J - 1 slots
    assert np.isfinite(score[4]).all() and (origin[4] >= 0).all()           # a column nearer: still J slots, the last one read to the table's last column but one
    assert np.isneginf(score[5:]).all() and (origin[5:] == -1).all() and (rank[5:] == -1).all()


def test_every_phase_at_two_slots_and_the_jw_clamp(engine, rings):
    tabs = _tables(310, 4, 190 + 2 * FL + 60)
    hop = _hop(np.random.default_rng(311), 3, [65535, 2 ** 32 - 3], 3 + 2 - 1)
    phases = np.tile(np.arange(FL), (3, 1))
    _at_equals_twin(engine, rings[3], tabs, [[0, 1, 2, 3], [3, 2, 1, 0], [0, 0, 0, 0]], [0, 60, 33], [2, 2, 1], phases, hop, [0, 1, 0],
                    [65535, 2 ** 32 - 3, 65535], 3)
    ring, u = rings[3]                                                      # Jw below a record's nslot: the raw call, Jw = 1
    d = engine.device
    out = (torch.empty((3, 3), dtype=torch.float64, device=d), torch.empty((3, 3), dtype=torch.int64, device=d),
           torch.empty((3, 3), dtype=torch.int32, device=d))
    args = dict(m=_dev(engine, tabs[0]), a=_dev(engine, tabs[1]), d=_dev(engine, tabs[2]), rows=4, stride=tabs[0].shape[1],
                row=_dev(engine, np.array([[0, 1, 2, 3], [3, 2, 1, 0], [0, 0, 0, 0]], np.int64)), col=_dev(engine, np.array([0, 60, 33], np.int64)),
                nslot=_dev(engine, np.array([2, 2, 1], np.int32)), B=3, Jw=1, phase=_dev(engine, phases[:, :5].astype(np.int32)), P=5, ring=ring.ring,
                hop=_dev(engine, hop), K=3, HR=2, Ccols=4, hop_row=_dev(engine, np.array([0, 1, 0], np.int32)),
                lo=_dev(engine, np.array([65535, 2 ** 32 - 3, 65535], np.uint32).view(np.int32)), n_origins=3, score=out[0], origin=out[1], rank=out[2],
                scratch=torch.empty(3 * 3 * 3, dtype=torch.int64, device=d))
    assert _raw(engine, args) == 0
    want = pr.coherent_score_at_model(*tabs, [[0, 1, 2, 3], [3, 2, 1, 0], [0, 0, 0, 0]], [0, 60, 33], [2, 2, 1], 1, phases[:, :5], u, hop, [0, 1, 0],
                                      [65535, 2 ** 32 - 3, 65535], 3)
    assert np.array_equal(_bits(out[0].cpu().numpy()), _bits(want[0])) and np.array_equal(out[1].cpu().numpy(), want[1])
    assert np.array_equal(out[2].cpu().numpy(), want[2]) and (want[1][:, 0] >= 0).all()


def test_nothing_outside_a_records_columns_is_read(engine, rings):
    """Every element outside columns [col, col + 1215 J + 190) of the records' own rows, and every unused row, is NaN: the same bits."""
    J, n = CT + 1, 65
    tabs = _tables(320, 7, 190 + FL * J + 900)
    rows4, col, nslot, bases, hop_row = _records(J, n)
    rows4[5] = [0, 1, 2, 7]
    hop = _hop(np.random.default_rng(321), 3, bases, n + J + 2)
    phases = np.random.default_rng(322).integers(0, FL, (7, 3))
    phases[0, 0] = 1214
    lo = [bases[h] if h < 4 else 0 for h in hop_row]
    clean = _at_equals_twin(engine, rings[3], tabs, rows4, col, nslot, phases, hop, hop_row, lo, n)
    keep = np.zeros(tabs[0].shape, bool)
    for r4, c, Jb in zip(rows4[:5], col[:5], (J, J, J, J - 1, J)):          # the five records that have slots, with their clamped J
        keep[r4, c:c + FL * Jb + 190] = True
    assert not keep[6].any() and not keep[:, :7].any() and not keep.all(axis=1).any()
    holed = [np.where(keep, t, np.nan) for t in tabs]
    got = [t.cpu().numpy() for t in engine.coherent_score_at(*[_dev(engine, t) for t in holed], np.array(rows4), np.array(col), nslot,
                                                             phases.astype(np.int32), rings[3][0], _dev(engine, hop), hop_row, lo, n)]
    assert np.array_equal(_bits(got[0]), _bits(clean[0])) and np.array_equal(got[1], clean[1]) and np.array_equal(got[2], clean[2])
    assert np.isfinite(got[0][:5]).all()


def test_records_that_are_not_addressable_or_have_no_slot_read_nothing(engine, rings):
    """Each way of being not addressable (a row below 0 and one at `rows`, a column below 0 and one past `stride`), a column at `stride`
    (addressable, no slot), a hop row below 0 and one at HR, an nslot below 0 and one of 0 -- in tables that are NaN everywhere but in the
    block of the one record that has a slot: every other record is (-inf, -1, -1), and the call is the twin's."""
    stride = 190 + FL + 40
    good = _tables(350, 4, stride)
    keep = np.zeros((4, stride), bool)
    keep[:, 3:3 + FL + 190] = True
    tabs = [np.where(keep, t, np.nan) for t in good]
    hop = _hop(np.random.default_rng(351), 3, [5, 77], 65)
    ok4 = [0, 1, 2, 3]
    rows4 = [ok4, [-1, 1, 2, 3], [0, 1, 2, 4], [0, -1, 2, 3], ok4, ok4, ok4, ok4, ok4, ok4, ok4, [4, 1, 2, 3]]
    col = [3, 3, 3, 3, -1, stride + 1, stride, 3, 3, 3, 3, 3]
    nslot = [1, 1, 1, 1, 1, 1, 1, 1, 1, -1, 0, 1]
    hop_row = [1, 0, 0, 0, 0, 0, 0, -1, 2, 0, 0, 0]
    lo = [77] + [5] * 11
    phases = np.tile(np.array([[9, 1214]]), (12, 1))
    score, origin, rank = _at_equals_twin(engine, rings[3], tabs, rows4, col, nslot, phases, hop, hop_row, lo, 65)
    assert np.isfinite(score[0]).all() and (origin[0] >= 0).all()
    assert np.isneginf(score[1:]).all() and (origin[1:] == -1).all() and (rank[1:] == -1).all()


def test_planted_ties_the_lower_origin_then_the_earlier_entry(engine, rings):
    """m == 0 makes every header sum zero: N = a, and origins whose windows hop alike tie exactly, in a block and across blocks."""
    J, n = 3, CHUNK + 60
    stride = 50 + 190 + FL * J
    M = np.zeros((5, stride))
    A, D = np.full((5, stride), -3.0), np.full((5, stride), 2.0)            # all scores negative: the best does not start at 0
    A[4] = -1.0
    hop = np.zeros((3, 1, n + J - 1), np.uint8)
    hop[0, 0, :] = np.arange(n + J - 1) % 2 * 3                             # key 0: origins of one parity share a window
    hop[1, 0, 5:8] = 3; hop[1, 0, CHUNK + 4:CHUNK + 7] = 3                  # key 1: origins 5 and 260, one per block
    hop[2, 0, 100:103] = 3; hop[2, 0, 200:203] = 3                          # key 2: origins 100 and 200 of one block
    score, origin, rank = _at_equals_twin(engine, rings[3], [M, A, D], [[0, 1, 2, 4]], [50], [J], [[17, 17]], hop, [0], [1000], n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [0, 0, 0] and score[0, 1] == score[0, 2] == -0.5
    A[4, 50 + 17::FL] = -7.0                                                # phase 17 is worse now; 18 named twice: the earlier entry
    _, origin, rank = _at_equals_twin(engine, rings[3], [M, A, D], [[0, 1, 2, 4]], [50], [J], [[17, 18, -1, 18, FL]], hop, [0], [1000], n)
    assert origin[0].tolist() == [1, 5, 100] and rank[0].tolist() == [1, 1, 1]


@pytest.mark.parametrize("J, n_origins", [(2, 65), (CT + 1, 257)])
def test_with_implied_rows_the_outputs_are_those_of_the_clip_call(engine, rings, J, n_origins):
    """row[b][band] = 4 b + band, col = 0, HR = 1, hop_row = 0, lo[b] = lo: es_coherent_score_batch on the same M, A, D, bit for bit."""
    ring, _ = rings[3]
    tabs = [_dev(engine, t) for t in _tables(330 + J, 8, 190 + FL * J + 5)]
    hop = _dev(engine, np.random.default_rng(331).integers(0, 4, (3, n_origins + J - 1)).astype(np.uint8))
    phases = np.random.default_rng(332).integers(0, FL, (2, 3)).astype(np.int32)
    lo = 65536 * 5 - 9
    clip = engine.coherent_score(*tabs, [J, J - 1], phases, ring, hop, lo, n_origins)
    at = engine.coherent_score_at(*tabs, np.arange(8).reshape(2, 4), [0, 0], [J, J - 1], phases, ring, hop, [0, 0], [lo, lo], n_origins)
    for a, b in zip(clip, at):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert bool((clip[1] >= 0).all()) and np.array_equal(_bits(clip[0].cpu().numpy()), _bits(at[0].cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------- refusals
ORDER = ("m", "a", "d", "rows", "stride", "row", "col", "nslot", "B", "Jw", "phase", "P", "ring", "hop", "K", "HR", "Ccols", "hop_row", "lo", "n_origins",
         "score", "origin", "rank", "scratch")


def _raw(engine, args, **over):
    a = dict(args)
    a.update(over)
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                 # noqa: E731
    rc = getattr(engine._lib, AT)(engine._ctx, *[p(a[k]) for k in ORDER], engine._stream())
    torch.cuda.synchronize()
    return rc


@pytest.fixture(scope="module")
def small(engine, rings):
    """A call that works: two records of two slots on eight rows, three keys, two hop rows, 300 origins (two chunks), two list entries."""
    stride = 190 + 2 * FL + 140
    d = engine.device
    full = lambda shape, dt: torch.empty(shape, dtype=dt, device=d)         # noqa: E731
    tabs = _tables(340, 8, stride)
    hop = _hop(np.random.default_rng(341), 3, [9, 70000], 301)
    return dict(m=_dev(engine, tabs[0]), a=_dev(engine, tabs[1]), d=_dev(engine, tabs[2]), rows=8, stride=stride,
                row=_dev(engine, np.array([[0, 1, 2, 3], [7, 6, 5, 4]], np.int64)), col=_dev(engine, np.array([100, 0], np.int64)),
                nslot=_dev(engine, np.array([2, 2], np.int32)), B=2, Jw=2, phase=_dev(engine, np.array([[1, 2], [3, 4]], np.int32)), P=2,
                ring=rings[3][0].ring, hop=_dev(engine, hop), K=3, HR=2, Ccols=301, hop_row=_dev(engine, np.array([1, 0], np.int32)),
                lo=_dev(engine, np.array([70000, 9], np.int32)), n_origins=300, score=full((2, 3), torch.float64), origin=full((2, 3), torch.int64),
                rank=full((2, 3), torch.int32), scratch=full(3 * 2 * 3 * 2, torch.int64), host=(tabs, hop))


REFUSALS = [dict(m=None), dict(a=None), dict(d=None), dict(row=None), dict(col=None), dict(nslot=None), dict(phase=None), dict(ring=None), dict(hop=None),
            dict(hop_row=None), dict(lo=None), dict(score=None), dict(origin=None), dict(rank=None), dict(scratch=None), dict(rows=-8), dict(stride=-1),
            dict(B=-2), dict(Jw=-1), dict(K=-3), dict(Ccols=-1), dict(n_origins=-1), dict(HR=0), dict(HR=-1), dict(HR=1 << 31), dict(rows=1 << 31),
            dict(stride=1 << 31), dict(Ccols=300), dict(n_origins=301), dict(Jw=3), dict(P=0), dict(P=1216), dict(P=-1),
            dict(n_origins=1 << 40, Ccols=(1 << 40) + 1), dict(K=1 << 30, n_origins=1 << 10, Ccols=(1 << 10) + 1)]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refusals_write_nothing(engine, small, over):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I); small["scratch"].fill_(POISON_I)
    assert _raw(engine, small, **over) == nat.ES_EINVAL
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert (small["scratch"] == POISON_I).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith(AT)


def test_the_accepted_call_and_the_empty_ones(engine, small, rings):
    small["score"].fill_(POISON_F); small["origin"].fill_(POISON_I); small["rank"].fill_(POISON_I)
    assert _raw(engine, small, B=0) == 0 and _raw(engine, small, K=0) == 0 and _raw(engine, small, B=0, K=0, score=None, m=None, row=None) == 0
    assert (small["score"] == POISON_F).all() and (small["origin"] == POISON_I).all() and (small["rank"] == POISON_I).all()
    assert _raw(engine, small) == 0
    tabs, hop = small["host"]
    want = pr.coherent_score_at_model(*tabs, [[0, 1, 2, 3], [7, 6, 5, 4]], [100, 0], [2, 2], 2, [[1, 2], [3, 4]], rings[3][1], hop, [1, 0], [70000, 9], 300)
    assert np.array_equal(_bits(small["score"].cpu().numpy()), _bits(want[0])) and np.array_equal(small["origin"].cpu().numpy(), want[1])
    assert np.array_equal(small["rank"].cpu().numpy(), want[2]) and (want[1] >= 0).all()
    assert _raw(engine, small, n_origins=0, Ccols=1, scratch=None, hop=None, m=None) == 0          # no origin: nothing is read, every pair is -inf
    assert np.isneginf(small["score"].cpu().numpy()).all() and (small["origin"] == -1).all() and (small["rank"] == -1).all()


def test_two_runs_give_the_same_bits_and_the_call_records_into_a_graph(engine, small, rings):
    ring = rings[3][0]
    tabs = [small[k] for k in "mad"]
    ph = _dev(engine, np.array([[5, 700], [1214, 0]], np.int32))

    def run():
        return engine.coherent_score_at(*tabs, small["row"], small["col"], small["nslot"], ph, ring, small["hop"], small["hop_row"], [70000, 9], 300)
    a = [t.clone() for t in run()]
    b = run()
    assert all(torch.equal(x, z) for x, z in zip(a, b)) and bool((a[1] >= 0).all())
    torch.cuda.synchronize()
    lo = _dev(engine, np.array([70000, 9], np.int32))                       # every argument on the device already: a capture may not upload
    out = dict(score=torch.empty_like(a[0]), origin=torch.empty_like(a[1]), rank=torch.empty_like(a[2]))
    args = dict(small, phase=ph, lo=lo, **out)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = getattr(engine._lib, AT)(engine._ctx, *[(args[k].data_ptr() if torch.is_tensor(args[k]) else args[k]) for k in ORDER], engine._stream())
    assert rc == 0
    torch.cuda.synchronize()
    for t in out.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], x) for k, x in zip(("score", "origin", "rank"), a))


# ---------------------------------------------------------------------------------------------------------------- end to end
def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases) == (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


def _same_map(m, w):
    assert (m is None) == (w is None)
    if m is not None:
        assert m.starts == w.starts and m.stretches == w.stretches and m.splices == w.splices and m.marked == w.marked
        assert len(m.windows) == len(w.windows)
        for p, q in zip(m.windows, w.windows):
            _same(p, q)


@pytest.fixture(scope="module")
def clip3():
    """The 3 s variant of DESIGN 4.28: sigma 0.2, seed 7, samples [60000, 60000 + 12650) removed."""
    with mock.patch.dict(PC.CLIPS, {"C": C_CLIP}):
        w = PC.marked("C", seconds=3.0)
    x = np.ascontiguousarray(np.concatenate([w[:CUT_AT], w[CUT_AT + CUT_LEN:]]), np.float32)
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def map3(engine, clip3):
    """presence_coherent_map of the clip, made once, and the band-passed rows that call downloaded."""
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    nonce = det.session_nonce
    got = det.presence_coherent_map(clip3, 48_000, **SMALL)
    (ids, y, sizes), = det._presence_rows
    assert ids == [0] and y.shape[0] == 4 and int(sizes[0]) == clip3.size and det.session_nonce is nonce and det._trace is None
    return got, y, int(sizes[0])


def test_the_map_of_the_spliced_loud_clip_is_the_twins(map3):
    got, y, n = map3
    for s, p in zip(got.starts, got.windows):
        print(f"window at slot {s}: own {p.score:.4f}, decoy max {p.null.max():.4f}, ctr {p.ctr}, phase {p.phase}, detected {p.detected}")
    _same_map(got, pr.coherent_map_model(y, n, PC.KEY, **SMALL))
    assert got.starts == [0, 20, 40, 60, 67] and all(p.detected and p.frames == 40 and len(p.phases) == FL for p in got.windows)
    assert [p.ctr for p in got.windows][2:] == [52, 72, 79]
    assert [(s.first, s.last, s.confirmed, s.t) for s in got.stretches] == [(0, 1, True, -PC.CUT), (2, 4, True, -PC.CUT - CUT_LEN)]
    assert len(got.splices) == 1 and got.splices[0].removed == CUT_LEN and got.marked == FL * 107


def test_the_batch_is_the_single_calls(engine, clip3, map3):
    from scipy.signal import resample_poly
    a = PC.cached("marked", "A")
    clips = [clip3, (resample_poly(a[:30_000], 147, 160) * 32768 * 20).astype(np.int16), a[:320 + FL - 1]]
    rates = [48_000, 44_100, 48_000]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    batch = det.presence_coherent_map_batch(clips, rates, **SMALL)
    assert batch[2] is None and len(batch[0].windows) == 5 and len(batch[1].windows) == 1 and batch[1].starts == [0]
    _same_map(batch[0], map3[0])
    _same_map(batch[1], det.presence_coherent_map(clips[1], 44_100, **SMALL))
    _same(batch[1].windows[0], det.presence_coherent(clips[1], 44_100, **SMALL))       # J <= window: presence_coherent on the clip, field for field
    assert batch[1].windows[0].frames <= 40 and det.presence_coherent_map(clips[2], 48_000, **SMALL) is None
    assert det.presence_coherent_map_batch([], 48_000) == []


def test_one_rows_call_per_launch_one_hop_window_and_one_score_per_group_and_width(engine, clip3, map3, monkeypatch):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)

    def count(limit, **kw):
        monkeypatch.setattr(ps, "MAP_HOP_BYTES", limit)
        calls, real = [], engine._call
        engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            m = det.presence_coherent_map(clip3, 48_000, **kw)
        finally:
            del engine._call
        assert calls.count("es_mf_rows_batch") == 1 and not any(n in ("es_coherent_score_batch", "es_warp_score_at_batch", "es_xcorr_batch") for n in calls)
        return m, [n for n in calls if n in ("es_hop_window_batch", AT)]

    assert ps.MAP_HOP_BYTES == 256 << 20
    m, back = count(256 << 20, **SMALL)
    _same_map(m, map3[0])
    assert back == ["es_hop_window_batch", AT]                              # five windows, five hop rows, one width: one group
    K, ccols = 3, 14 + 40 - 1
    m, back = count(K * 2 * ccols, **SMALL)                                 # two hop rows fit: groups of 2, 2 and 1 windows
    _same_map(m, map3[0])
    assert back == ["es_hop_window_batch", AT] * 3
    m, back = count(1, **SMALL)                                             # a group holds at least one window
    _same_map(m, map3[0])
    assert back == ["es_hop_window_batch", AT] * 5
    # a span at the top of the counters: the windows' spans are lowered at 2^32 to widths 20, 11 and 0 -- one score call per width
    top = (2 ** 32 - 70, 2 ** 32 - 50)
    assert sorted({hi - lo for lo, hi in (pr.window_span(top, s, 40) for s in m.starts)}) == [0, 11, 20]
    m, back = count(256 << 20, span=top, decoys=2)
    assert back == ["es_hop_window_batch", AT, AT, AT]
    assert [p.ctr >= 0 for p in m.windows] == [True, True, False, False, False] and not any(p.detected for p in m.windows[2:])


def test_identifier_entry_k_is_the_detector_of_key_k(engine, clip3, map3):
    keys = [PC.OTHER_KEY, PC.KEY]
    clips = [clip3, clip3[:30_000], clip3[:1000]]
    ident = WatermarkIdentifier(keys, list_size=8, engine=engine)
    maps = ident.presence_coherent_map_batch(clips, 48_000, **SMALL)
    ones = ident.presence_coherent_batch(clips[1:], 48_000, **SMALL)
    assert maps[2] is None and ones[1] is None and all(len(g) == 2 for g in maps[:2]) and len(ones[0]) == 2
    _same_map(maps[0][1], map3[0])
    _same_map(ident.presence_coherent_map(clips[1], 48_000, **SMALL)[0], maps[1][0])
    _same(ident.presence_coherent(clips[1], 48_000, **SMALL)[1], ones[0][1])
    for k, key in enumerate(keys):
        det = WatermarkDetector(key, list_size=8, engine=engine)
        want = det.presence_coherent_map_batch(clips, 48_000, **SMALL)
        for c in range(2):
            _same_map(maps[c][k], want[c])
        _same(ones[0][k], det.presence_coherent(clips[1], 48_000, **SMALL))
    assert maps[0][1].marked == FL * 107 and not any(s.confirmed for s in maps[0][0].stretches)    # the other key marks nothing here
