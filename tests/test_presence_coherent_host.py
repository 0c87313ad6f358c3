"""CPU: the host side of the coherent presence test -- the twin (echoseal_amd/presence.py mf_rows_model,
coherent_score_model, coherent_model) against loops written out here, the slot formula at its edges, every argument check, the companion
header's place in the binding, and the twin's verdicts on clips D and A of DESIGN 4.23 rebuilt with the CPU oracle."""
import math
from unittest import mock

import numpy as np
import pytest

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.tables import pack_tables
from echoseal_amd.utils import mseq_63

FL = 1215


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def tabs():
    return pr.mf_tables(48_000)


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_the_companion_header_is_bound_beside_the_abi():
    assert len(nat.DECLARATIONS) == len(nat.SIGNATURES) == 56 and nat.ES_ABI_VERSION == 2
    assert list(nat.COHERENT_DECLARATIONS) == list(nat.COHERENT_SIGNATURES) == ["es_mf_rows_batch", "es_coherent_score_batch"]
    assert nat.COHERENT_CONSTANTS == {"ES_MF_TILE": 256, "ES_COH_TILE": 16, "ES_COH_HDR_PN": 272} and nat.ES_MF_TILE == 256
    others = (nat.SIGNATURES, nat.PRESENCE_SIGNATURES, nat.WARP_SIGNATURES, nat.LIVE_PRESENCE_SIGNATURES, nat.PICK_SIGNATURES)
    assert not any(set(nat.COHERENT_SIGNATURES) & set(t) for t in others)
    consts = (nat.CONSTANTS, nat.PRESENCE_CONSTANTS, nat.WARP_CONSTANTS, nat.LIVE_PRESENCE_CONSTANTS, nat.PICK_CONSTANTS)
    assert not any(set(nat.COHERENT_CONSTANTS) & set(t) for t in consts)
    assert [n for _, n in nat.COHERENT_DECLARATIONS["es_mf_rows_batch"]] == ["ctx", "y_dev", "rows", "T", "len_dev", "band_dev", "m_dev", "a_dev",
                                                                           "d_dev", "stream"]
    score = nat.COHERENT_DECLARATIONS["es_coherent_score_batch"]
    assert [n for _, n in score] == ["ctx", "m_dev", "a_dev", "d_dev", "rows", "T", "nslot_dev", "B", "phase_dev", "P", "ring_dev", "hop_dev", "K",
                                     "Ccols", "lo", "n_origins", "score_dev", "origin_dev", "rank_dev", "scratch_dev", "stream"]
    assert dict((n, t) for t, n in score)["lo"] == "uint32_t"
    for name, params in nat.COHERENT_DECLARATIONS.items():
        res, args = nat.COHERENT_SIGNATURES[name]
        assert res is nat.c_int and len(args) == len(params) and params[0] == ("es_ctx*", "ctx") and params[-1] == ("void*", "stream")
        for (ctype, _), arg in zip(params, args):
            assert (arg is nat.c_int64) == (ctype == "int64_t") and (arg is nat.c_uint32) == (ctype == "uint32_t") and (arg is nat.c_int) == (ctype == "int")
    src = open(nat.HEADER_PATH).read()
    assert "es_mf_rows_batch" not in src and "es_coherent_score_batch" not in src            # include/echoseal_hip.h is as it was


# ---------------------------------------------------------------------------------------------------------------- the rows
def _rows_loop(y, n, g, c):
    """M, A, D of one record, one term at a time."""
    pre = [2.0 * int(b) - 1.0 for b in mseq_63()]
    L, W = len(g), 190 + len(g)
    M, A, D = {}, {}, {}
    for t in range(n - L + 1):
        s = 0.0
        for i in range(L):
            s = s + float(y[t + i]) * float(g[i])
        M[t] = s
    for t in range(n - W + 1):
        a = q = 0.0
        for k in range(63):
            a = a + pre[k] * M[t + k]
        for k in range(W):
            q = q + float(y[t + k]) * float(y[t + k])
        A[t], D[t] = a, math.sqrt(q) * float(c)
    return M, A, D


def test_the_tables_are_the_engines(tabs):
    g, c = tabs
    _, _, taps, ntaps, _ = pack_tables()
    assert [len(t) for t in g] == list(ntaps) == [131, 116, 123, 93]
    for b in range(4):
        assert g[b].dtype == np.float64 and np.array_equal(g[b][::-1].astype(np.float32), taps[b, :ntaps[b]])
        s = 0.0
        for v in g[b]:
            s = s + float(v) * float(v)
        assert c[b] == math.sqrt(191.0 * s)
    assert max(len(t) for t in pr.mf_tables(44_100)[0]) == 550


@pytest.mark.parametrize("band", range(4))
def test_rows_model_is_the_written_out_loop_around_the_window(tabs, band):
    """n = W - 1 (m alone), W (one start), W + 1 (two), in one call with NaN past every length."""
    g, c = tabs
    W = 190 + len(g[band])
    lens = [W - 1, W, W + 1, len(g[band]) - 1]
    y = np.random.default_rng(60 + band).standard_normal((4, W + 5))
    for r, n in enumerate(lens):
        y[r, n:] = np.nan                                                   # what must never be read
    M, A, D = pr.mf_rows_model(y, lens, [band] * 4, g, c)
    for r, n in enumerate(lens):
        m, a, d = _rows_loop(y[r], n, g[band], c[band])
        assert len(a) == len(d) == max(n - W + 1, 0) and len(m) == max(n - len(g[band]) + 1, 0)
        assert _same_bits(M[r, :len(m)], [m[t] for t in range(len(m))]) and np.isnan(M[r, len(m):]).all()
        assert _same_bits(A[r, :len(a)], [a[t] for t in range(len(a))]) and np.isnan(A[r, len(a):]).all()
        assert _same_bits(D[r, :len(d)], [d[t] for t in range(len(d))]) and np.isnan(D[r, len(d):]).all()
        assert np.isfinite(M[r, :len(m)]).all() and (D[r, :len(d)] > 0).all()
    assert np.isnan(M[3]).all()                                             # shorter than the filter: nothing is defined


def test_rows_model_clamps_lengths_and_refuses_bad_rows(tabs):
    g, c = tabs
    y = np.random.default_rng(64).standard_normal((2, 400))
    M, A, D = pr.mf_rows_model(y, [10 ** 9, -3], [3, 3], g, c)
    assert np.isfinite(M[0, :400 - 93 + 1]).all() and np.isfinite(A[0, :400 - 283 + 1]).all() and np.isnan(M[1]).all()
    zero = pr.mf_rows_model(np.zeros((1, 400)), [400], [3], g, c)
    assert not zero[0][0, :308].any() and not zero[2][0, :118].any()       # a silent record: D == 0
    for bad in (dict(lens=[400], bands=[0, 1]), dict(lens=[400, 400], bands=[0, 4]), dict(lens=[400, 400], bands=[-1, 0])):
        with pytest.raises(ValueError):
            pr.mf_rows_model(y, bad["lens"], bad["bands"], g, c)


def test_the_slot_formula_at_its_edges(tabs):
    g, _ = tabs
    Lmax = 131
    for J in (1, 2):
        n = 189 + Lmax + FL * J
        assert pr.coherent_slots(n - 1, g) == J - 1 and pr.coherent_slots(n, g) == J
        # at n every start phi + 1215 j, phi <= 1214, j < J is defined in the band of the longest filter, and the next one is not
        assert 1214 + FL * (J - 1) + 190 + Lmax <= n < 1214 + FL * (J - 1) + 1 + 190 + Lmax
    assert pr.coherent_slots(0, g) == 0 and pr.coherent_slots(-7, g) == 0
    assert pr.check_coherent_reach((2 ** 32 - 10, 2 ** 32 - 2), 320 + 3 * FL, g) == (2 ** 32 - 10, 2 ** 32 - 2)          # hi + J - 1 == 2^32
    with pytest.raises(ValueError):
        pr.check_coherent_reach((2 ** 32 - 10, 2 ** 32 - 1), 320 + 3 * FL, g)
    assert pr.check_coherent_reach((2 ** 32 - 10, 2 ** 32 - 1), 320 + 3 * FL - 1, g)[1] == 2 ** 32 - 1                   # one sample fewer: J = 2


# ---------------------------------------------------------------------------------------------------------------- the score
def _score_loop(M, A, D, nslot, phases, u, hop, lo, n_origins):
    B, K, T = len(nslot), hop.shape[0], M.shape[1]
    score, origin, rank = np.full((B, K), -math.inf), np.full((B, K), -1, np.int64), np.full((B, K), -1, np.int32)
    for b in range(B):
        J = min(max(int(nslot[b]), 0), max(0, T - 190) // FL)
        for k in range(K):
            best = None
            for o in range(n_origins if J else 0):
                if any(hop[k, o + j] > 3 for j in range(J)):
                    continue
                for p, phi in enumerate(phases[b]):
                    if not 0 <= phi < FL:
                        continue
                    acc = 0.0
                    for j in range(J):
                        c, band, s = lo + o + j, 4 * b + int(hop[k, o + j]), phi + FL * j
                        v = c & 0xFFFF
                        Z = []
                        for i in range(16):
                            z = 0.0
                            for m in range(8):
                                z = z + float(u[k, 8 * i + m]) * float(M[band, s + 63 + 8 * i + m])
                            Z.append(z)
                        H = Lo = 0.0
                        for i in range(8):
                            H = H + (2.0 * ((v >> (15 - i)) & 1) - 1.0) * Z[i]
                        for i in range(8, 16):
                            Lo = Lo + (2.0 * ((v >> (15 - i)) & 1) - 1.0) * Z[i]
                        N = (float(A[band, s]) + H) + Lo
                        acc = acc + (0.0 if D[band, s] == 0 else N / float(D[band, s]))
                    sc = acc / J
                    if best is None or sc > best[0] or (sc == best[0] and o < best[1]):  # entries ascend within an origin: ties keep the first
                        best = (sc, o, p)
            if best is not None:
                score[b, k], origin[b, k], rank[b, k] = best
    return score, origin, rank


def _case(seed, B, J, K, n_origins, negative=False):
    rng = np.random.default_rng(seed)
    T = 190 + FL * J + 3
    M = rng.standard_normal((4 * B, T))
    A = -np.abs(rng.standard_normal((4 * B, T))) * 40 - 50 if negative else rng.standard_normal((4 * B, T)) * 8
    D = np.abs(rng.standard_normal((4 * B, T))) + 0.5
    u = 2.0 * rng.integers(0, 2, (K, 128)) - 1.0
    hop = rng.integers(0, 4, (K, n_origins + J - 1)).astype(np.uint8)
    return M, A, D, u, hop


def _agree(got, want):
    assert _same_bits(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1:], want[1:])
    assert got[1].dtype == np.int64 and got[2].dtype == np.int32


@pytest.mark.parametrize("lo", [0, 250, 65536 - 3, 2 ** 32 - 12])
def test_score_model_is_the_written_out_loop_across_byte_boundaries(lo):
    """Windows whose counters cross a multiple of 256 (lo = 250), of 65 536 (lo = 65 533) and reach the last counter."""
    M, A, D, u, hop = _case(70, 2, 3, 2, 9)
    nslot, phases = [3, 2], [[5, 1214, 0], [1214, 7, 7]]
    got = pr.coherent_score_model(M, A, D, nslot, phases, u, hop, lo, 9)
    _agree(got, _score_loop(M, A, D, nslot, phases, u, hop, lo, 9))
    assert np.isfinite(got[0]).all() and (got[1] >= 0).all()
    if lo == 65536 - 3:                                                    # the header bits do enter: another lo, other scores
        assert not np.array_equal(got[0], pr.coherent_score_model(M, A, D, nslot, phases, u, hop, lo + 1, 9)[0])


def test_score_model_a_silent_window_adds_zero_and_missing_counters_are_not_scored():
    M, A, D, u, hop = _case(71, 1, 2, 3, 6)
    D[:, 40] = 0.0                                                          # slot 0 of phase 40, every band
    hop[1, 3] = 0xFF                                                        # key 1: origins 2 and 3 hold column 3
    hop[2, :] = 0xFF                                                        # key 2: nothing to score
    phases = [[40, 41]]
    got = pr.coherent_score_model(M, A, D, [2], phases, u, hop, 7, 6)
    _agree(got, _score_loop(M, A, D, [2], phases, u, hop, 7, 6))
    assert got[1][0, 1] not in (2, 3) and np.isneginf(got[0][0, 2]) and got[1][0, 2] == -1 and got[2][0, 2] == -1
    only = pr.coherent_score_model(M, A, D, [2], [[40]], u[:1], hop[:1], 7, 6)
    want = _score_loop(M, A, D, [2], [[40]], u[:1], hop[:1], 7, 6)
    _agree(only, want)


def test_score_model_no_slot_no_origin_no_phase():
    M, A, D, u, hop = _case(72, 2, 2, 2, 5)
    none = (np.full((2, 2), -np.inf), np.full((2, 2), -1), np.full((2, 2), -1))
    for nslot, phases, n in (([0, 0], [[1, 2], [3, 4]], 5), ([2, 2], [[1, 2], [3, 4]], 0), ([2, 2], [[-1, FL], [FL + 7, -5]], 5)):
        got = pr.coherent_score_model(M, A, D, nslot, phases, u, hop, 0, n)
        assert np.array_equal(got[0], none[0]) and np.array_equal(got[1], none[1]) and np.array_equal(got[2], none[2])
    got = pr.coherent_score_model(M, A, D, [9, -1], [[1, 2], [3, 4]], u, hop, 0, 5)       # clamped to (T - 190) // 1215 = 2 and to 0
    _agree(got, _score_loop(M, A, D, [2, 0], [[1, 2], [3, 4]], u, hop, 0, 5))
    assert (got[1][0] >= 0).all() and (got[1][1] == -1).all()
    with pytest.raises(ValueError):
        pr.coherent_score_model(M, A, D, [2, 2], [[1], [2]], u, hop[:, :5], 0, 5)          # fewer than n_origins + J - 1 columns
    with pytest.raises(ValueError):
        pr.coherent_score_model(M, A, D, [2, 2, 2], [[1], [2], [3]], u, hop, 0, 5)         # three clips need twelve rows


def test_score_model_planted_ties_lowest_origin_then_earliest_entry():
    """m == 0 makes every header sum zero: N = a, and origins whose windows hop alike tie exactly, whatever their counters."""
    J, n = 2, 6
    T = 190 + FL * J
    M = np.zeros((4, T))
    A, D = np.full((4, T), -3.0), np.full((4, T), 2.0)                      # all scores negative: the best does not start at 0
    A[3] = -1.0
    u = np.ones((1, 128))
    hop = np.array([[0, 3, 3, 0, 3, 3, 1]], np.uint8)                       # origins 1 and 4 hop 3, 3
    score, origin, rank = pr.coherent_score_model(M, A, D, [J], [[9, 9, 9]], u, hop, 300, n)
    assert score[0, 0] == -0.5 and origin[0, 0] == 1 and rank[0, 0] == 0
    _agree((score, origin, rank), _score_loop(M, A, D, [J], [[9, 9, 9]], u, hop, 300, n))
    A[3, 9] = A[3, 9 + FL] = -7.0                                           # phase 9 is worse now; 10 and 11 tie: the earlier entry
    score, origin, rank = pr.coherent_score_model(M, A, D, [J], [[9, 11, 10, 11]], u, hop, 300, n)
    assert score[0, 0] == -0.5 and origin[0, 0] == 1 and rank[0, 0] == 1


def test_score_model_all_scores_negative():
    M, A, D, u, hop = _case(73, 1, 3, 2, 7, negative=True)
    got = pr.coherent_score_model(M, A, D, [3], [[0, 600, 1214]], u, hop, 1000, 7)
    _agree(got, _score_loop(M, A, D, [3], [[0, 600, 1214]], u, hop, 1000, 7))
    assert (got[0] < 0).all() and (got[1] >= 0).all()


def test_header_signs_are_the_ring_bytes():
    keys = [PC.KEY] + pr.decoy_keys(2)
    u = pr.header_signs(keys)
    det = WatermarkDetector(PC.KEY)
    assert u.shape == (3, 128) and set(np.unique(u)) == {-1.0, 1.0} and np.array_equal(u[0], det._hdr_pn_sy.astype(np.float64))
    assert np.array_equal(pr.ring_signs(np.packbits((u > 0).astype(np.uint8), axis=1)), u)


# ---------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw, word", [
    (dict(span=(-1, 5)), "outside"), (dict(span=(5, 2 ** 32 + 1)), "outside"), (dict(span=(9, 3)), "reversed"), (dict(span=7), "pair"),
    (dict(span=(0.0, 4)), "integers"), (dict(span=(2 ** 32 - 10, 2 ** 32)), "wrap"), (dict(span=(2 ** 32 - 10, 2 ** 32 - 1)), "wrap"),
    (dict(phases=0), "phases"), (dict(phases=1216), "phases"), (dict(phases=2.0), "phases"), (dict(phases=True), "phases"),
    (dict(decoys=-1), "decoys"), (dict(decoys=1.5), "decoys"), (dict(ctr0=-3), "ctr0"), (dict(ctr0=2 ** 32), "ctr0"), (dict(ctr0=[1, 2]), "ctr0"),
    (dict(ctr0=2 ** 32 - 1), "outside"),
])
def test_every_refusal_comes_before_any_engine(kw, word, monkeypatch):
    det = WatermarkDetector(PC.KEY)
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    clip = np.zeros(320 + 3 * FL, np.float32)                               # J = 3: span (2^32 - 10, 2^32 - 1) reaches counter 2^32
    kw = dict(kw)
    with pytest.raises(ValueError) as e:
        det.presence_coherent(clip, 48_000, kw.pop("ctr0", None), **kw)
    assert word in str(e.value), str(e.value)


def test_clips_without_a_slot_need_no_engine(monkeypatch):
    det = WatermarkDetector(PC.KEY)
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    assert det.presence_coherent_batch([np.zeros(320 + FL - 1, np.float32), np.zeros(10, np.float32)], 48_000) == [None, None]
    assert det.presence_coherent_batch([], 48_000) == []
    assert pr.coherent_model(np.zeros((4, 320 + FL - 1)), 320 + FL - 1, PC.KEY, span=(0, 4)) is None


# ---------------------------------------------------------------------------------------------------------------- the verdicts
# Clip D of DESIGN 4.23: white host of sigma 0.2, 2 s, seed 7.  Its unmarked host is that of seed 108: with span (0, 16), 8 decoys and all
# phases it scores 0.0827 against a decoy maximum of 0.1043 (seed 107: 0.0866 against 0.0918, undetected too; with 32 decoys at span
# (0, 64) seed 107 is the 1-in-33 false alarm the rule allows, so it is not the one used here).
D_CLIP = (0.2, 2.0, 7, 108)
SMALL = dict(span=(0, 16), decoys=8)


@pytest.fixture(scope="module")
def y_rows(oracle):
    ba = pack_tables()[0]

    def rows(clip):
        x = np.ascontiguousarray(clip, np.float32)
        return np.stack([oracle.lfilter(ba[b, :9], ba[b, 9:], x) for b in range(4)]), x.size
    with mock.patch.dict(PC.CLIPS, {"D": D_CLIP}):                          # the shared table of clips is left as it was
        d = PC.marked("D")
        return {"D": rows(d), "A": rows(PC.cached("marked", "A")), "U": rows(PC.unmarked("D")), "D_clip": d}


def test_the_twin_finds_clip_D_where_the_preamble_test_does_not(oracle, y_rows):
    corr, nlag = PC.oracle_rows(oracle, y_rows["D_clip"])
    old = pr.presence_model(corr, nlag, PC.KEY, span=(0, 64), phases=8, decoys=32)
    print(f"clip D, preamble test: own {old.score:.4f}, decoy max {old.null.max():.4f}")
    assert not old.detected
    y, n = y_rows["D"]
    p = pr.coherent_model(y, n, PC.KEY, **SMALL)
    print(f"clip D, coherent: own {p.score:.4f}, decoy max {p.null.max():.4f}, median {np.median(p.null):.4f}")
    assert p.detected and (p.ctr, p.phase) == PC.FOUND and p.ctr0 == 1 and p.frames == (n - 189 - 131) // FL == 78
    assert p.phases == list(range(FL)) and p.null.shape == (8,)
    assert pr.coherent_model(y, n, PC.KEY, span=(0, 16), decoys=0).detected is False       # no decoy, no verdict


def test_the_twin_finds_clip_A_and_refuses_the_unmarked_host(y_rows):
    y, n = y_rows["A"]
    p = pr.coherent_model(y, n, PC.KEY, **SMALL)
    print(f"clip A, coherent: own {p.score:.4f}, decoy max {p.null.max():.4f}, median {np.median(p.null):.4f}")
    assert p.detected and (p.ctr, p.phase) == PC.FOUND
    y, n = y_rows["U"]
    q = pr.coherent_model(y, n, PC.KEY, **SMALL)
    print(f"unmarked host (seed 108), coherent: own {q.score:.4f}, decoy max {q.null.max():.4f}")
    assert not q.detected and q.ctr >= 0
