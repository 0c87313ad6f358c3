"""CPU: the host side of the presence test under sample-clock drift -- presence.skew_table at its edges and every ValueError,
the warp twins against loops written out here and, on a table of zeros, bit for bit against the rigid twins, the hypothesis pick with
planted ties, unusable rows, the new companion header's place in the binding, and the twin's verdicts on clip B resampled by 10001/10000
and rebuilt with the CPU oracle."""
import math
from fractions import Fraction

import numpy as np
import pytest

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector

FL = 1215


def _rows(seed, nlags, stride):
    corr = np.random.default_rng(seed).uniform(-1.0, 1.0, (4 * len(nlags), stride))
    for b, n in enumerate(nlags):
        corr[4 * b:4 * b + 4, n:] = np.nan                                  # what must never be read
    return corr


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- the skew table
@pytest.mark.parametrize("E", [0, 1, 29, 1214])
def test_skew_table_order_rounding_and_columns(E):
    nlag = {0: 3 * FL + 7, 1: 4000, 29: 97_000, 1214: 1_214_000}[E]
    ppm = {0: 0.0, 1: 250.0, 29: 298.5, 1214: 1000.0}[E]
    assert math.ceil(Fraction(ppm) * nlag / 10 ** 6) == E
    skews, J, warp = pr.skew_table(nlag, ppm)
    assert J == (nlag - E) // FL and J >= 3
    assert skews == [0] + [s * e for e in range(1, E + 1) for s in (-1, 1)] and len(skews) == 2 * E + 1
    assert warp.shape == (2 * E + 1, J) and warp.dtype == np.int32
    assert not warp[0].any() and not warp[:, 0].any()                       # row 0 is the rigid grid; every grid starts where it does
    for d, e in enumerate(skews):
        step = np.diff(warp[d].astype(np.int64))
        assert (step >= 0).all() if e >= 0 else (step <= 0).all()           # monotone
        assert warp[d, J - 1] == math.floor(Fraction(2 * (J - 1) * e + J, 2 * J))
        assert abs(Fraction(int(warp[d, J - 1])) - Fraction((J - 1) * e, J)) <= Fraction(1, 2)
    j = np.arange(J, dtype=np.int64)
    first = FL * j + warp.astype(np.int64)
    assert first.min() >= 0 and first.max() + 1214 < nlag                   # every column phi + 1215 j + warp, phi <= 1214, inside [0, nlag)
    mid = warp[:, J // 2].astype(np.int64)                                   # round half up of j e / J, for negative e too
    assert mid.tolist() == [math.floor(Fraction(J // 2 * e, J) + Fraction(1, 2)) for e in skews]


def test_skew_table_is_exact_where_floats_are_not():
    assert pr.skew_table(10 ** 6, 29.0)[0][-1] == 29                        # 29.0 * 10^6 / 10^6 is exactly 29: no 30th skew
    assert pr.skew_table(10 ** 6, np.nextafter(29.0, 30.0))[0][-1] == 30    # one ulp more is
    assert pr.skew_table(3 * FL, 0)[1:2] == (3,) and pr.skew_table(100, 300.0)[1] == 0 and pr.skew_table(-5, 300.0)[1] == 0
    assert pr.skew_table(2 * FL, 1.0)[1] == 1                               # one sample of skew costs the slot that no longer fits


@pytest.mark.parametrize("bad", [-1.0, -0.0001, math.inf, -math.inf, math.nan, "300", None, True, [300.0], 3 + 0j])
def test_check_drift_refuses(bad):
    with pytest.raises(ValueError) as e:
        pr.check_drift(bad)
    assert "drift_ppm" in str(e.value)
    with pytest.raises(ValueError):
        pr.skew_table(5 * FL, bad)


def test_skew_table_refuses_a_whole_frame_and_an_emptied_clip():
    assert pr.check_drift(0) == 0.0 and pr.check_drift(np.float32(2.5)) == 2.5 and pr.check_drift(np.int64(7)) == 7.0
    assert pr.skew_table(1_214_000, 1000.0)[0][-1] == 1214
    with pytest.raises(ValueError) as e:
        pr.skew_table(1_214_001, 1000.0)                                    # E = 1215
    assert "frame" in str(e.value)
    with pytest.raises(ValueError) as e:
        pr.skew_table(FL, 1.0)                                              # E = 1 takes the only slot
    assert "slot" in str(e.value)
    assert pr.skew_table(FL - 1, 1.0)[1] == 0                               # no slot to begin with: no error, J == 0


@pytest.mark.parametrize("kw, word", [(dict(drift_ppm=-1.0), "drift_ppm"), (dict(drift_ppm=math.nan), "drift_ppm"), (dict(drift_ppm="3"), "drift_ppm"),
                                      (dict(drift_ppm=400_000.0), "frame"), (dict(drift_ppm=300.0, n=FL + 62), "slot")])
def test_every_refusal_comes_before_any_engine(kw, word, monkeypatch):
    det = WatermarkDetector(PC.KEY)
    monkeypatch.setattr(WatermarkDetector, "engine", property(lambda self: pytest.fail("an engine was asked for")))
    clip = np.zeros(kw.pop("n", 3 * FL + 62), np.float32)
    with pytest.raises(ValueError) as e:
        det.presence(clip, 48_000, span=PC.SPAN, **kw)
    assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        pr.presence_model(np.zeros((4, clip.size - 62)), clip.size - 62, PC.KEY, span=PC.SPAN, **kw)


# ---------------------------------------------------------------------------------------------------------------- the twins
def _usable_loop(warp, b, d, nwarp, J, n):
    return d < nwarp[b] and all(0 <= FL * j + int(warp[b][d][j]) and FL * j + int(warp[b][d][j]) + 1214 < n for j in range(J))


def _slots_loop(nslot, warp, nlag):
    return [min(max(int(s), 0), np.shape(warp)[2], n // FL) for s, n in zip(nslot, nlag)]


def _fold_loop(corr, nlag, warp, nwarp, nslot):
    B, D = len(nlag), np.shape(warp)[1]
    out = np.full((B, D, FL), -math.inf)
    for b, J in enumerate(_slots_loop(nslot, warp, nlag)):
        for d in range(D):
            if not _usable_loop(warp, b, d, nwarp, J, nlag[b]):
                continue
            for phi in range(FL):
                s = 0.0
                for j in range(J):
                    s = s + max(float(corr[4 * b + band, phi + FL * j + int(warp[b][d][j])]) for band in range(4))
                out[b, d, phi] = s
    return out


def _score_loop(corr, nlag, warp, nwarp, nslot, hyp, hop, n_origins):
    B, K, D = len(nlag), hop.shape[0], np.shape(warp)[1]
    score, origin, rank = np.full((B, K), -math.inf), np.full((B, K), -1, np.int64), np.full((B, K), -1, np.int32)
    for b, J in enumerate(_slots_loop(nslot, warp, nlag)):
        for k in range(K):
            best = None
            for c in range(n_origins if J else 0):
                if any(hop[k, c + j] > 3 for j in range(J)):
                    continue
                for h, (d, phi) in enumerate(hyp[b]):
                    if not (0 <= d < D and 0 <= phi < FL and _usable_loop(warp, b, d, nwarp, J, nlag[b])):
                        continue
                    s = 0.0
                    for j in range(J):
                        s = s + float(corr[4 * b + hop[k, c + j], phi + FL * j + int(warp[b][d][j])])
                    s = s / J
                    if best is None or s > best[0]:                         # origins ascend, entries ascend: ties keep the first
                        best = (s, c, h)
            if best is not None:
                score[b, k], origin[b, k], rank[b, k] = best
    return score, origin, rank


@pytest.fixture(scope="module")
def planted():
    """Three clips (3 slots and a skew of +-2, one slot, no slot) under one table [3][5][3]; clip 0's row 3 leaves the clip at its last
    slot, clip 1 has two rows, and row 1 of clip 1 starts before lag 0."""
    nlag = [3 * FL + 2, FL + 1, 700]
    corr = _rows(11, nlag, 3 * FL + 6)
    warp = np.zeros((3, 5, 3), np.int64)
    warp[0] = [[0, 0, 0], [0, -1, -2], [0, 1, 2], [0, 1, 3], [0, -1, -1]]    # row 3: 2 * 1215 + 3 + 1214 = nlag: one past the last lag
    warp[1, 1, 0] = -1
    warp[1, 2:] = 10 ** 6                                                    # rows past nwarp: never looked at
    return corr, nlag, warp, [5, 2, 5], [3, 1, 4]


def test_warp_fold_model_is_the_written_out_loop(planted):
    corr, nlag, warp, nwarp, nslot = planted
    got = pr.warp_fold_model(corr, nlag, warp, nwarp, nslot)
    assert got.shape == (3, 5, FL) and _same_bits(got, _fold_loop(corr, nlag, warp, nwarp, nslot))
    assert np.isfinite(got[0, [0, 1, 2, 4]]).all() and np.isneginf(got[0, 3]).all()                 # unusable at the last slot
    assert np.isfinite(got[1, 0]).all() and np.isneginf(got[1, 1:]).all()                           # unusable at the first slot, and by nwarp
    assert not got[2].any()                                                                          # J == 0: zeros in every usable row
    assert not _same_bits(got[0, 1], got[0, 0]) and not _same_bits(got[0, 2], got[0, 4])
    fewer = pr.warp_fold_model(corr, nlag, warp, nwarp, [2, 1, 0])                                  # two slots: row 3 fits
    assert np.isfinite(fewer[0]).all() and _same_bits(fewer, _fold_loop(corr, nlag, warp, nwarp, [2, 1, 0]))


def test_warp_score_model_is_the_written_out_loop(planted):
    corr, nlag, warp, nwarp, nslot = planted
    hop = np.random.default_rng(12).integers(0, 4, (3, 20 + 3 - 1)).astype(np.uint8)
    hop[1, 9] = 0xFF
    hyp = [[(0, 5), (3, 5), (2, 1212), (1, 7), (5, 7), (4, FL)], [(1, 0), (0, 1214), (2, 3), (0, 1214), (-1, 3), (0, -1)], [(0, 0)] * 6]
    got = pr.warp_score_model(corr, nlag, warp, nwarp, nslot, hyp, hop, 20)
    want = _score_loop(corr, nlag, warp, nwarp, nslot, hyp, hop, 20)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[1].dtype == np.int64 and got[2].dtype == np.int32
    assert set(got[2][0].tolist()) <= {0, 2, 3} and (got[2][1] == 1).all()                          # unusable and unnamed entries are never the best
    assert np.isneginf(got[0][2]).all() and (got[1][2] == -1).all() and (got[2][2] == -1).all()      # J == 0
    only = pr.warp_score_model(corr, nlag, warp, nwarp, nslot, [[(3, 5)] * 2, [(1, 0)] * 2, [(0, 0)] * 2], hop, 20)
    assert np.isneginf(only[0]).all() and (only[1] == -1).all() and (only[2] == -1).all()            # nothing but unusable rows: nothing scored


def test_a_table_of_zeros_is_the_rigid_twin():
    nlag = [3 * FL + 100, FL, 700]
    corr = _rows(13, nlag, 3 * FL + 100)
    zeros, nwarp, nslot = np.zeros((3, 1, 3), np.int32), [1, 1, 1], [n // FL for n in nlag]
    assert _same_bits(pr.warp_fold_model(corr, nlag, zeros, nwarp, nslot)[:, 0], pr.fold_model(corr, nlag))
    hop = np.random.default_rng(14).integers(0, 4, (3, 40 + 3 - 1)).astype(np.uint8)
    hop[2, 30] = 0xFF
    phases = [[5, 1214, 0, 5], [1214, 7, 7, 3], [1, 2, 3, 4]]
    got = pr.warp_score_model(corr, nlag, zeros, nwarp, nslot, [[(0, p) for p in row] for row in phases], hop, 40)
    want = pr.score_model(corr, nlag, phases, hop, 40)
    assert _same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    wide = np.zeros((3, 1, 9), np.int32)                                     # a wider table and a larger nslot clamp to nlag // 1215
    assert _same_bits(pr.warp_fold_model(corr, nlag, wide, nwarp, [9, 9, 9])[:, 0], pr.fold_model(corr, nlag))


def test_pick_hypotheses_planted_ties():
    f = np.tile(np.linspace(0.0, 1.0, FL), (3, 1))
    f[1, 7] = f[0, 300] = f[2, 7] = f[0, 1214] = 5.0
    f[2, 3] = f[1, 900] = 4.0
    assert pr.pick_hypotheses(f, 8) == [(0, 300), (0, 1214), (1, 7), (2, 7), (1, 900), (2, 3), (1, 1214), (2, 1214)]
    assert pr.pick_hypotheses(np.zeros((2, FL)), 3) == [(0, 0), (0, 1), (0, 2)]                     # lower row, then lower phase
    f[1] = -np.inf                                                                                   # an unusable row is never picked
    assert pr.pick_hypotheses(f, 6) == [(0, 300), (0, 1214), (2, 7), (2, 3), (2, 1214), (0, 1213)]
    assert pr.pick_hypotheses(f[1:2], 5) == [] and len(pr.pick_hypotheses(f, 1215)) == 1215
    assert pr.pick_hypotheses(f[:1], 1215) == [(0, p) for p in pr.pick_phases(f[0], 1215)]
    with pytest.raises(ValueError):
        pr.pick_hypotheses(f[:, :100], 3)
    with pytest.raises(ValueError):
        pr.pick_hypotheses(f, 0)


def test_presence_keeps_its_positional_fields():
    p = pr.Presence(True, 0.5, np.zeros(2), 1, 438, 1, 78, [438])
    assert (p.skew, p.drift_ppm, p.hypotheses) == (0, 0.0, None)
    q = pr.drift_verdict(np.array([0.5, 0.25]), np.array([3, 1]), np.array([1, 0]), 10, [(0, 7), (2, 438)], [0, -1, 1], 78)
    assert q.detected and (q.ctr, q.phase, q.skew, q.frames, q.phases) == (13, 438, 1, 78, [7, 438]) and q.hypotheses == [(0, 7), (1, 438)]
    assert q.drift_ppm == 1e6 * 1 / (FL * 78)
    none = pr.drift_verdict(np.array([-np.inf, -np.inf]), np.array([-1, -1]), np.array([-1, -1]), 10, [(0, 7)], [0], 78)
    assert not none.detected and (none.ctr, none.phase, none.ctr0, none.skew, none.drift_ppm) == (-1, -1, -1, 0, 0.0)


def test_the_warp_header_is_bound_beside_the_others():
    assert len(nat.DECLARATIONS) == len(nat.SIGNATURES) == 56 and nat.ES_ABI_VERSION == 2
    assert set(nat.PRESENCE_DECLARATIONS) == set(nat.PRESENCE_SIGNATURES) == {"es_phase_fold_batch", "es_hop_score_batch"}
    assert nat.PRESENCE_CONSTANTS == {"ES_HOP_TILE": 64, "ES_HOP_ORIGINS": 256}
    assert set(nat.WARP_DECLARATIONS) == set(nat.WARP_SIGNATURES) == {"es_warp_fold_batch", "es_warp_score_batch"}
    assert not set(nat.WARP_DECLARATIONS) & (set(nat.DECLARATIONS) | set(nat.PRESENCE_DECLARATIONS))
    assert not set(nat.WARP_CONSTANTS) & (set(nat.CONSTANTS) | set(nat.PRESENCE_CONSTANTS))
    assert nat.WARP_CONSTANTS == {"ES_WARP_HB": nat.ES_WARP_HB} and 2 <= nat.ES_WARP_HB <= 16
    from test_abi_binding import POINTERS, SCALARS
    for name, params in nat.WARP_DECLARATIONS.items():
        assert {t for t, _ in params} <= SCALARS | POINTERS, name
        assert params[0] == ("es_ctx*", "ctx") and params[-1] == ("void*", "stream") and name.endswith("_batch"), name
        assert not any(p == "stream" for _, p in params[:-1]) and len(nat.WARP_SIGNATURES[name][1]) == len(params)
        for (ctype, _), arg in zip(params, nat.WARP_SIGNATURES[name][1]):
            assert (arg is nat.c_int64) == (ctype == "int64_t") and (arg is nat.c_int) == (ctype == "int"), (name, ctype)
    for path in (nat.HEADER_PATH, nat.PRESENCE_HEADER_PATH):
        assert "es_warp" not in open(path).read() and "ES_WARP" not in open(path).read()        # the other two headers are as they were


# ---------------------------------------------------------------------------------------------------------------- verdicts on oracle rows
@pytest.fixture(scope="module")
def drifted(oracle):
    """Clip B played 100 ppm slow (resampled by 10001/10000) and B's unmarked host, as oracle rows."""
    from scipy.signal import resample_poly
    clip = resample_poly(PC.cached("marked", "B").astype(np.float64), 10001, 10000).astype(np.float32)
    return PC.oracle_rows(oracle, clip), PC.oracle_rows(oracle, PC.cached("unmarked", "B"))


def test_the_rigid_grid_loses_the_drifted_clip_and_the_search_finds_it(drifted):
    (corr, nlag), _ = drifted
    rigid = pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, phases=8, decoys=32)
    assert not rigid.detected and (rigid.skew, rigid.drift_ppm, rigid.hypotheses) == (0, 0.0, None)
    p = pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300)
    print(f"B + 100 ppm: rigid {rigid.score:.4f} / {rigid.null.max():.4f}; searched {p.score:.4f} / {p.null.max():.4f} at skew {p.skew}")
    assert p.detected and p.ctr == 1 and p.phase == 438 and abs(p.skew - 10) <= 1 and p.ctr0 == 1
    E = math.ceil(Fraction(300) * nlag / 10 ** 6)
    assert p.frames == (nlag - E) // FL and len(p.hypotheses) == 8 and p.phases == [phi for _, phi in p.hypotheses]
    assert (p.skew, 438) in p.hypotheses and p.drift_ppm == 1e6 * p.skew / (FL * p.frames) and 80 < p.drift_ppm < 125
    assert p.null.shape == (32,) and pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, decoys=0, drift_ppm=300).detected is False
    assert not pr.presence_model(corr, nlag, PC.OTHER_KEY, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300).detected


def test_the_search_does_not_flag_the_unmarked_host(drifted):
    _, (corr, nlag) = drifted
    p = pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, phases=8, decoys=32, drift_ppm=300)
    print(f"B's unmarked host: {p.score:.4f} / {p.null.max():.4f}")
    assert not p.detected


def test_a_clip_without_a_whole_slot_has_no_result():
    assert pr.presence_model(np.zeros((4, 1214)), 1214, PC.KEY, span=PC.SPAN, drift_ppm=300) is None
