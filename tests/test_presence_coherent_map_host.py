"""CPU: the host side of the coherent presence timeline -- the sixth companion header's place in the binding, the twin of
es_coherent_score_at_batch (echoseal_amd/presence.py coherent_score_at_model) against loops written out here, coherent_windows at its
edges, every argument check of the new public calls without an engine, and coherent_map_model on the spliced loud clip C of DESIGN 4.28
rebuilt with the CPU oracle.  Own score and decoy maximum of every window are printed."""
import math
from unittest import mock

import numpy as np
import pytest

import echoseal_amd._native as nat
import presence_cases as PC
import presence_map_cases as MC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier
from echoseal_amd.tables import pack_tables

FL = 1215
AT = "es_coherent_score_at_batch"


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_the_sixth_companion_header_is_bound_beside_the_abi():
    assert len(nat.DECLARATIONS) == len(nat.SIGNATURES) == 56 and nat.ES_ABI_VERSION == 2
    assert list(nat.COHERENT_AT_DECLARATIONS) == list(nat.COHERENT_AT_SIGNATURES) == [AT] and nat.COHERENT_AT_CONSTANTS == {}
    # the five other companions' tables are as they were
    assert list(nat.PRESENCE_DECLARATIONS) == ["es_phase_fold_batch", "es_hop_score_batch"]
    assert list(nat.WARP_DECLARATIONS) == ["es_warp_fold_batch", "es_warp_score_batch"]
    assert list(nat.LIVE_PRESENCE_DECLARATIONS) == ["es_warp_fold_at_batch", "es_warp_score_at_batch"]
    assert list(nat.PICK_DECLARATIONS) == ["es_fold_pick_batch"] and nat.PICK_CONSTANTS == {"ES_PICK_MAX_H": 64}
    assert list(nat.COHERENT_DECLARATIONS) == ["es_mf_rows_batch", "es_coherent_score_batch"]
    assert nat.COHERENT_CONSTANTS == {"ES_MF_TILE": 256, "ES_COH_TILE": 16, "ES_COH_HDR_PN": 272}
    others = (nat.SIGNATURES, nat.PRESENCE_SIGNATURES, nat.WARP_SIGNATURES, nat.LIVE_PRESENCE_SIGNATURES, nat.PICK_SIGNATURES, nat.COHERENT_SIGNATURES)
    assert not any(set(nat.COHERENT_AT_SIGNATURES) & set(t) for t in others)
    params = nat.COHERENT_AT_DECLARATIONS[AT]
    assert params == [("es_ctx*", "ctx"), ("const double*", "m_dev"), ("const double*", "a_dev"), ("const double*", "d_dev"), ("int64_t", "rows"),
                      ("int64_t", "stride"), ("const int64_t*", "row_dev"), ("const int64_t*", "col_dev"), ("const int32_t*", "nslot_dev"),
                      ("int64_t", "B"), ("int64_t", "Jw"), ("const int32_t*", "phase_dev"), ("int", "P"), ("const uint8_t*", "ring_dev"),
                      ("const uint8_t*", "hop_dev"), ("int64_t", "K"), ("int64_t", "HR"), ("int64_t", "Ccols"), ("const int32_t*", "hop_row_dev"),
                      ("const uint32_t*", "lo_dev"), ("int64_t", "n_origins"), ("double*", "score_dev"), ("int64_t*", "origin_dev"),
                      ("int32_t*", "rank_dev"), ("void*", "scratch_dev"), ("void*", "stream")]
    res, args = nat.COHERENT_AT_SIGNATURES[AT]
    assert res is nat.c_int and len(args) == len(params)
    for (ctype, _), arg in zip(params, args):
        assert (arg is nat.c_int64) == (ctype == "int64_t") and (arg is nat.c_int) == (ctype == "int")
    for path in (nat.HEADER_PATH, nat.COHERENT_HEADER_PATH, nat.LIVE_PRESENCE_HEADER_PATH):
        assert AT not in open(path).read()                                  # the other headers are as they were


# ---------------------------------------------------------------------------------------------------------------- the score over records
def _at_loop(M, A, D, rows4, col, nslot, Jw, phases, u, hop, hop_row, lo, n_origins):
    """include/echoseal_coherent_at.h, one term at a time."""
    rows, stride = M.shape
    B, K, HR = len(nslot), hop.shape[0], hop.shape[1]
    score, origin, rank = np.full((B, K), -math.inf), np.full((B, K), -1, np.int64), np.full((B, K), -1, np.int32)
    for b in range(B):
        ok = 0 <= col[b] <= stride and all(0 <= r < rows for r in rows4[b]) and 0 <= hop_row[b] < HR
        J = min(max(int(nslot[b]), 0), Jw, max(0, stride - col[b] - 190) // FL) if ok else 0
        for k in range(K):
            best = None
            for o in range(n_origins if J else 0):
                if any(hop[k, hop_row[b], o + j] > 3 for j in range(J)):
                    continue
                for p, phi in enumerate(phases[b]):
                    if not 0 <= phi < FL:
                        continue
                    acc = 0.0
                    for j in range(J):
                        c = (lo[b] + o + j) & 0xFFFFFFFF
                        row, s = rows4[b][int(hop[k, hop_row[b], o + j])], col[b] + phi + FL * j
                        v = c & 0xFFFF
                        Z = []
                        for i in range(16):
                            z = 0.0
                            for m in range(8):
                                z = z + float(u[k, 8 * i + m]) * float(M[row, s + 63 + 8 * i + m])
                            Z.append(z)
                        H = Lo = 0.0
                        for i in range(8):
                            H = H + (2.0 * ((v >> (15 - i)) & 1) - 1.0) * Z[i]
                        for i in range(8, 16):
                            Lo = Lo + (2.0 * ((v >> (15 - i)) & 1) - 1.0) * Z[i]
                        N = (float(A[row, s]) + H) + Lo
                        acc = acc + (0.0 if D[row, s] == 0 else N / float(D[row, s]))
                    sc = acc / J
                    if best is None or sc > best[0] or (sc == best[0] and o < best[1]):  # entries ascend within an origin: ties keep the first
                        best = (sc, o, p)
            if best is not None:
                score[b, k], origin[b, k], rank[b, k] = best
    return score, origin, rank


def _tables(seed, rows, stride, K=2):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((rows, stride))
    A = rng.standard_normal((rows, stride)) * 8
    D = np.abs(rng.standard_normal((rows, stride))) + 0.5
    u = 2.0 * rng.integers(0, 2, (K, 128)) - 1.0
    return rng, M, A, D, u


def _hop(rng, K, bases, cols):
    """Hop rows as es_hop_window_batch would shape them: [K, HR, cols], 0xFF where base + column is no counter."""
    hop = rng.integers(0, 4, (K, len(bases), cols)).astype(np.uint8)
    for h, base in enumerate(bases):
        hop[:, h, max(2 ** 32 - base, 0):] = 0xFF
    return hop


def _agree(got, want):
    assert _same_bits(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    assert got[1].dtype == np.int64 and got[2].dtype == np.int32


def test_at_model_is_the_written_out_loop_records_that_share_rows_and_overlap():
    """Columns that are no multiple of 1215, two records on the same rows that overlap, a record whose bands lie in rows of its own
    order; a counter base per record: windows that cross a multiple of 256 within the origins (250) and across the slots of one
    origin (254), a multiple of 65 536 (65 533), and the last counters with 0xFF bytes behind them."""
    stride = 190 + 3 * FL + 700
    rng, M, A, D, u = _tables(200, 6, stride)
    bases = [250, 65536 - 3, 2 ** 32 - 10, 254]
    hop = _hop(rng, 2, bases, 9 + 3 - 1)
    rows4 = [[0, 1, 2, 3], [0, 1, 2, 3], [5, 3, 4, 0], [2, 2, 1, 1]]
    col, nslot, hop_row = [7, 331, 699, 1], [3, 3, 2, 3], [0, 1, 2, 3]
    phases = [[5, 1214, 0], [1214, 7, 7], [3, -1, 600], [0, 1, FL]]
    args = (M, A, D, rows4, col, nslot, 3, phases, u, hop, hop_row, [bases[h] for h in hop_row], 9)
    got = pr.coherent_score_at_model(*args)
    _agree(got, _at_loop(*args))
    assert np.isfinite(got[0]).all() and (got[1] >= 0).all() and (got[1][2] <= 10 - 2).all()       # base 2^32 - 10, J = 2: origins 0 .. 8 exist
    moved = pr.coherent_score_at_model(M, A, D, rows4, col, nslot, 3, phases, u, hop, hop_row, [b + 1 for b in bases[:2]] + bases[2:], 9)
    assert not np.array_equal(moved[0][:2], got[0][:2]) and _same_bits(moved[0][2:], got[0][2:])    # lo is the record's own
    M2 = M.copy(); M2[4:, :] = np.nan; M2[:, 190 + 3 * FL + 331:] = np.nan                          # what records 0, 1 and 3 never read
    again = pr.coherent_score_at_model(M2, A, D, rows4, col, nslot, 3, phases, u, hop, hop_row, [bases[h] for h in hop_row], 9)
    assert _same_bits(again[0][[0, 1, 3]], got[0][[0, 1, 3]])


def test_at_model_the_slot_clamps_at_their_edges():
    """stride - col - 190 == 2 * 1215 exactly, one below and one above; the Jw clamp; nslot below zero."""
    stride = 190 + 2 * FL + 50
    rng, M, A, D, u = _tables(201, 4, stride)
    hop = _hop(rng, 2, [1000], 6 + 3 - 1)
    rows4 = [[0, 1, 2, 3]] * 5
    col, nslot, phases = [50, 51, 49, 50, 0], [3, 3, 3, -2, 9], [[0, 1214]] * 5
    for Jw, want_J in ((3, [2, 1, 2, 0, 2]), (1, [1, 1, 1, 0, 1]), (0, [0] * 5)):
        args = (M, A, D, rows4, col, nslot, Jw, phases, u, hop, [0] * 5, [1000] * 5, 6)
        got = pr.coherent_score_at_model(*args)
        _agree(got, _at_loop(*args))
        assert ((got[1][:, 0] >= 0) == (np.array(want_J) > 0)).all()
        for b, J in enumerate(want_J):                                      # the J the clamp gives is the J that is summed
            one = pr.coherent_score_at_model(M, A, D, rows4[b:b + 1], col[b:b + 1], [J], 3, phases[:1], u, hop, [0], [1000], 6)
            assert _same_bits(one[0], got[0][b:b + 1])
    with pytest.raises(ValueError):
        pr.coherent_score_at_model(M, A, D, rows4, col, nslot, 4, phases, u, hop, [0] * 5, [1000] * 5, 6)      # Ccols < n_origins + Jw - 1
    with pytest.raises(ValueError):
        pr.coherent_score_at_model(M, A, D, rows4, col, nslot, -1, phases, u, hop, [0] * 5, [1000] * 5, 6)


def test_at_model_records_that_are_not_addressable_and_hop_rows_that_do_not_exist():
    stride = 190 + FL + 40
    rng, M, A, D, u = _tables(202, 4, stride)
    hop = _hop(rng, 2, [5, 77], 4)
    rows4 = [[0, 1, 2, 3], [-1, 1, 2, 3], [0, 1, 2, 4], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3]]
    col = [3, 3, 3, -1, stride + 1, stride, 3, 3]                           # col == stride is addressable and has no slot
    hop_row = [1, 0, 0, 0, 0, 0, -1, 2]
    args = (M, A, D, rows4, col, [1] * 8, 1, [[9, 10]] * 8, u, hop, hop_row, [77, 5, 5, 5, 5, 5, 5, 5], 4)
    got = pr.coherent_score_at_model(*args)
    _agree(got, _at_loop(*args))
    assert (got[1][0] >= 0).all() and np.isneginf(got[0][1:]).all() and (got[1][1:] == -1).all() and (got[2][1:] == -1).all()


def test_at_model_planted_ties_lowest_origin_then_earliest_entry():
    """m == 0 makes every header sum zero: N = a, and origins whose windows hop alike tie exactly, whatever their counters."""
    J, n = 2, 6
    stride = 40 + 190 + FL * J
    M = np.zeros((5, stride))
    A, D = np.full((5, stride), -3.0), np.full((5, stride), 2.0)
    A[4] = -1.0
    u = np.ones((1, 128))
    hop = np.array([[[0, 3, 3, 0, 3, 3, 1]]], np.uint8)                     # origins 1 and 4 hop 3, 3
    args = (M, A, D, [[0, 1, 2, 4]], [40], [J], J, [[9, 9, 9]], u, hop, [0], [300], n)
    got = pr.coherent_score_at_model(*args)
    assert got[0][0, 0] == -0.5 and got[1][0, 0] == 1 and got[2][0, 0] == 0
    _agree(got, _at_loop(*args))
    A[4, 49] = A[4, 49 + FL] = -7.0                                         # phase 9 is worse now; 10 and 11 tie: the earlier entry
    got = pr.coherent_score_at_model(M, A, D, [[0, 1, 2, 4]], [40], [J], J, [[9, 11, 10, 11]], u, hop, [0], [300], n)
    assert got[0][0, 0] == -0.5 and got[1][0, 0] == 1 and got[2][0, 0] == 1


def test_at_model_with_implied_rows_is_the_clip_model():
    """row[b][band] = 4 b + band, col = 0, HR = 1, hop_row = 0, lo[b] = lo, Jw >= every J: the bits of coherent_score_model."""
    stride = 190 + 3 * FL + 3
    rng, M, A, D, u = _tables(203, 8, stride, K=3)
    hop = rng.integers(0, 4, (3, 9 + 3 - 1)).astype(np.uint8)
    nslot, phases = [3, 2], [[5, 1214, 0], [1214, 7, 7]]
    want = pr.coherent_score_model(M, A, D, nslot, phases, u, hop, 65533, 9)
    for h in (hop, hop[:, None, :]):
        got = pr.coherent_score_at_model(M, A, D, [[0, 1, 2, 3], [4, 5, 6, 7]], [0, 0], nslot, 3, phases, u, h, [0, 0], [65533, 65533], 9)
        _agree(got, want)
    assert (want[1] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- the windows
@pytest.mark.parametrize("W, S", [(40, 20), (5, 2), (3, 3)])
def test_coherent_windows_at_their_edges(W, S):
    g, _ = pr.mf_tables(48_000)
    n_of = lambda J: 189 + 131 + FL * J                                     # noqa: E731  the shortest clip of J slots
    assert pr.coherent_windows(n_of(1) - 1, g, W, S) == [] and pr.coherent_windows(0, g, W, S) == []
    assert pr.coherent_windows(n_of(1), g, W, S) == [(0, 0, 1)]
    assert pr.coherent_windows(n_of(W), g, W, S) == [(0, 0, W)] and pr.coherent_windows(n_of(W + 1) - 1, g, W, S) == [(0, 0, W)]
    for J in (W + 1, W + S, W + S + 1):
        starts = [s for s in range(J) if s % S == 0 and s + W <= J]
        if starts[-1] != J - W:
            starts.append(J - W)
        assert pr.coherent_windows(n_of(J), g, W, S) == [(s, FL * s, W) for s in starts]
        assert all(FL * s + FL * W + 189 + 131 <= n_of(J) for s in starts)  # every window's samples lie in the clip
    assert len(pr.coherent_windows(n_of(W + 1), g, W, S)) == 2 and len(pr.coherent_windows(n_of(W + S), g, W, S)) == 2
    assert len(pr.coherent_windows(n_of(W + S + 1), g, W, S)) == (2 if S == 1 else 3)
    for bad in ((0, 1), (3, 4), (3, 0), (2.0, 1)):
        with pytest.raises(ValueError):
            pr.coherent_windows(n_of(3), g, *bad)


# ---------------------------------------------------------------------------------------------------------------- refusals
MAP_BAD = [dict(window=2.5), dict(window=True), dict(step=0), dict(window=10, step=11), dict(window=0), dict(confirm=0), dict(confirm=1.0)]
BOTH_BAD = [dict(span=(-1, 5)), dict(span=(5, 2 ** 32 + 1)), dict(span=(9, 3)), dict(span=7), dict(span=(0.0, 4)), dict(decoys=-1), dict(decoys=1.5),
            dict(ctr0=-3), dict(ctr0=2 ** 32), dict(ctr0=[1, 2])]
ONE_BAD = [dict(phases=0), dict(phases=1216), dict(phases=2.0), dict(span=(2 ** 32 - 10, 2 ** 32 - 1))]


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("kw", MAP_BAD + BOTH_BAD, ids=_ids)
def test_the_map_calls_refuse_before_any_engine(kw, monkeypatch):
    det, ident = WatermarkDetector(PC.KEY), WatermarkIdentifier([PC.KEY, PC.OTHER_KEY])
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    clip = np.zeros(320 + 3 * FL, np.float32)
    for who in (det, ident):
        kw1 = dict(kw)
        ctr0 = kw1.pop("ctr0", None)
        with pytest.raises(ValueError):
            who.presence_coherent_map(clip, 48_000, ctr0, **kw1)
        with pytest.raises(ValueError):
            who.presence_coherent_map_batch([clip], 48_000, None if ctr0 is None else [ctr0], **kw1)
    with pytest.raises(TypeError):
        det.presence_coherent_map(clip, 48_000, phases=8)                   # every phase is always searched: there is no such argument
    with pytest.raises(TypeError):
        det.presence_coherent_map(clip, 48_000, drift_ppm=10.0)


@pytest.mark.parametrize("kw", ONE_BAD + BOTH_BAD, ids=_ids)
def test_the_identifiers_coherent_calls_refuse_before_any_engine(kw, monkeypatch):
    ident = WatermarkIdentifier([PC.KEY, PC.OTHER_KEY])
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    clip = np.zeros(320 + 3 * FL, np.float32)                               # J = 3: span (2^32 - 10, 2^32 - 1) reaches counter 2^32
    kw = dict(kw)
    ctr0 = kw.pop("ctr0", None)
    with pytest.raises(ValueError):
        ident.presence_coherent(clip, 48_000, ctr0, **kw)
    with pytest.raises(ValueError):
        ident.presence_coherent_batch([clip], 48_000, None if ctr0 is None else [ctr0], **kw)


def test_clips_without_a_slot_and_no_keys_need_no_engine(monkeypatch):
    det, ident, nobody = WatermarkDetector(PC.KEY), WatermarkIdentifier([PC.KEY, PC.OTHER_KEY]), WatermarkIdentifier([])
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    short = [np.zeros(320 + FL - 1, np.float32), np.zeros(10, np.float32)]
    for who in (det, ident):
        assert who.presence_coherent_map_batch(short, 48_000) == [None, None] and who.presence_coherent_map_batch([], 48_000) == []
        assert who.presence_coherent_map(short[0], 48_000, span=(2 ** 32 - 10, 2 ** 32)) is None      # a window lowers its span: no reach to refuse
    assert ident.presence_coherent_batch(short, 48_000) == [None, None]
    assert nobody.presence_coherent_batch([np.zeros(9000, np.float32)], 48_000) == [None]
    assert nobody.presence_coherent_map_batch([np.zeros(9000, np.float32)], 48_000) == [None]
    assert pr.coherent_map_model(np.zeros((4, 320 + FL - 1)), 320 + FL - 1, PC.KEY, span=(0, 4)) is None


# ---------------------------------------------------------------------------------------------------------------- the verdicts
# Clip C of DESIGN 4.23: white host of sigma 0.2, 5 s, seed 7, spliced as the clips of tests/presence_map_cases.py are; its unmarked host is
# that of seed 108.
C_CLIP = (0.2, 5.0, 7, 108)
SMALL = dict(span=(0, 16), decoys=8)


@pytest.fixture(scope="module")
def y_rows(oracle):
    ba = pack_tables()[0]

    def rows(clip):
        x = np.ascontiguousarray(clip, np.float32)
        y = np.stack([oracle.lfilter(ba[b, :9], ba[b, 9:], x) for b in range(4)])
        y.setflags(write=False)
        return y, x.size
    with mock.patch.dict(PC.CLIPS, {"C": C_CLIP}):                          # the shared table of clips is left as it was
        spliced, host = MC.clip("spliced", "C"), MC.clip("unmarked", "C")
    return {"C": rows(spliced), "U": rows(host), "C_clip": spliced}


def _show(what, m):
    for s, p in zip(m.starts, m.windows):
        print(f"{what}, window at slot {s}: own {p.score:.4f}, decoy max {p.null.max():.4f}, ctr {p.ctr}, phase {p.phase}, detected {p.detected}")


def test_the_twin_maps_the_spliced_loud_clip(y_rows):
    y, n = y_rows["C"]
    m = pr.coherent_map_model(y, n, PC.KEY, **SMALL)
    _show("spliced C, coherent", m)
    J = (n - 189 - 131) // FL
    assert m.starts == [0, 20, 40, 60, 80, 100, 120, 140, J - 40] and J == 186
    assert all(p.detected and p.frames == 40 for p in m.windows)
    assert [(s.first, s.last, s.confirmed, s.t) for s in m.stretches] == [(0, 3, True, MC.T0), (4, 8, True, MC.T0 - MC.CUT_LEN)]
    assert [p.ctr for p in m.windows] == [1, 21, 41, 61, 92, 112, 132, 152, 158] and [p.phase for p in m.windows] == [438] * 4 + [1153] * 5
    assert len(m.splices) == 1 and m.splices[0].removed == MC.CUT_LEN and m.splices[0].lo == 60 * FL and m.splices[0].hi == 120 * FL
    assert m.marked == FL * J and m.stretches[0].ctr0 == 1 and m.stretches[1].start == 80 * FL and m.stretches[1].end == FL * J
    assert all(p.ctr0 == pr.origin_of(p.ctr, p.phase, FL * s) for s, p in zip(m.starts, m.windows))


def test_the_preamble_map_confirms_nothing_on_the_same_clip(oracle, y_rows):
    corr, nlag = PC.oracle_rows(oracle, y_rows["C_clip"])
    m = pr.map_model(corr, nlag, PC.KEY, span=MC.SPAN)
    _show("spliced C, preamble map", m)
    assert not any(p.detected for p in m.windows) and m.stretches == [] and m.splices == [] and m.marked == 0


def test_the_twin_confirms_nothing_on_the_unmarked_host(y_rows):
    y, n = y_rows["U"]
    m = pr.coherent_map_model(y, n, PC.KEY, **SMALL)
    _show("unmarked host (seed 108), coherent", m)
    assert len(m.windows) == 9 and not any(s.confirmed for s in m.stretches) and m.splices == [] and m.marked == 0


def test_a_clip_of_at_most_one_window_is_the_coherent_model_field_for_field(y_rows):
    y, _ = y_rows["C"]
    n = 30_000
    m = pr.coherent_map_model(y[:, :n], n, PC.KEY, **SMALL)
    p, q = m.windows[0], pr.coherent_model(y[:, :n], n, PC.KEY, **SMALL)
    assert m.starts == [0] and len(m.windows) == 1 and q.frames == (n - 320) // FL == 24
    assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases) == (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases)
    assert _same_bits([p.score], [q.score]) and _same_bits(p.null, q.null)
    assert [(s.first, s.last, s.confirmed) for s in m.stretches] == ([(0, 0, False)] if q.detected else []) and m.marked == 0
    one = pr.coherent_map_model(y[:, :n], n, PC.KEY, confirm=1, **SMALL)
    assert one.marked == (FL * 24 if q.detected else 0)
