"""Every row of tests/sync_screen_cases.py has the property it was built for -- asserted from the CPU oracle alone, so that
tests/test_gpu_sync_screen.py cannot quietly test nothing.  No GPU.

Counts "within reach" are counts of exact values within 2 DELTA (order statistics, top-five band) or DELTA (rivals) of the value
that decides; the picker's capacities are 192 exact values per band and 64 rivals per candidate."""
import numpy as np
import pytest

import sync_screen_cases as S
from sync_screen_cases import DELTA, near_count

TS = (1215, 2048, 3000)
CAP, RIVALS = 192, 64


@pytest.fixture(scope="module", params=TS)
def C(request):
    return S.cases(request.param)


def _rows(C, family, **match):
    idx = C.rows(family, **match)
    assert idx, (family, match)
    return [(i, C.info[i], C.ref[i]) for i in idx]


def _peak_near(ref, lag, reach=31):
    """A threshold crosser that survived the suppression within `reach` of `lag` (the fallback's five largest are no crossers)."""
    return not ref["fallback"] and any(abs(int(p) - lag) <= reach for p in ref["peaks"])


def test_row_set(C):
    assert 100 <= len(C.info) <= 150
    assert C.y.shape == (len(C.info), C.T) and np.isfinite(C.y).all()
    assert len({d["name"] + str(d["band"]) for d in C.info}) == len(C.info)
    for fam in ("crossers", "fallback", "madlock", "medlock", "repeats", "satedge", "crosser", "swap", "ordinary"):
        assert C.rows(fam), fam
    for fam in ("medlock", "repeats", "satedge", "crosser", "swap", "ordinary"):
        assert {C.info[i]["band"] for i in C.rows(fam)} == {0, 1, 2, 3}, fam
    unsafe = [d["name"] for d in C.info if not d["f32_safe"]]
    assert len(unsafe) == 13 and all("1e20" in n or "1e+20" in n or "1e+30" in n for n in unsafe), unsafe


def test_near_tied_crossers(C):
    at = S.zone_start(C.T)
    rivals = {}
    for i, d, r in _rows(C, "crossers"):
        corr, Z = r["corr"], d["Z"]
        top, flat = corr.max(), corr[at + Z - 1]
        assert not r["fallback"] and r["thr"] < 0.95 and flat >= r["thr"] + 0.05, d
        # the plateau holds the row's maximum (Z = 20: the windows that straddle the zone's start, graded near-ties, hold it)
        assert top - flat <= (1e-9 if Z >= 50 else 2e-3), d
        assert abs(flat - S.c0(d["r"], 0)) < 1e-9, d                            # ... at the value the zone was built for
        tied = np.abs(corr - flat) <= DELTA                                     # a plateau candidate and its rivals
        # (r = 0.6, Z = 100: the first window's samples end at 1e-8, where the reference's "+ 1e-12" costs more than DELTA)
        assert (corr[tied] >= r["thr"]).all() and tied.sum() >= min(Z, 99), d
        assert near_count(corr, flat, 1e-9) >= min(Z, 66), d                    # ... decided in the last digits
        assert r["total"] == np.count_nonzero(corr == top) >= 1, d              # all within one suppression window: exact ties are all kept
        rivals[d["name"]] = int(tied.sum()) - 1
        if d["r"] == 0.6 and 63 <= Z <= 67:
            assert tied.sum() == Z, d
    names = lambda zs: [f"crossers r0.6 Z{z}" for z in zs]                      # noqa: E731
    assert all(rivals[n] <= RIVALS for n in names((20, 50, 63, 64, 65))), rivals
    assert all(rivals[n] > RIVALS for n in names((66, 67, 100))), rivals
    assert rivals["crossers r0.6 Z65"] == RIVALS and rivals["crossers r0.6 Z66"] == RIVALS + 1
    (big,) = C.rows("crossers", Z=100, r=0.5)
    assert C.ref[big]["total"] > 32 and rivals[C.info[big]["name"]] > RIVALS    # more peaks than a row of the peak table holds
    (mid,) = C.rows("crossers", Z=50, r=0.5)
    assert C.ref[mid]["total"] == 50 and rivals[C.info[mid]["name"]] < RIVALS   # 2**-k: fifty exactly equal peaks


def test_near_tied_fallback(C):
    band5 = {}
    for i, d, r in _rows(C, "fallback"):
        corr = r["corr"]
        assert r["fallback"] and r["total"] == 5 and r["thr"] < 0.95 and not (corr >= r["thr"]).any(), d
        band5[d["name"]] = b = near_count(corr, np.sort(corr)[-5])
        if d["Z"] == 100:
            assert 100 <= b <= 160, (d, b)
        if d["Z"] == 250:
            assert b > CAP, (d, b)
    sweep = [band5[f"fallback Z{z} amp1e20"] for z in S.SWEEP]
    assert min(sweep) <= CAP < max(sweep), sweep
    assert band5["fallback Z192 amp1e12"] <= CAP < band5["fallback Z193 amp1e12"], band5


def test_mad_lock(C):
    band = {}
    for i, d, r in _rows(C, "madlock"):
        corr = r["corr"]
        dev = np.abs(corr - r["med"])
        band[d["name"]] = b = near_count(dev, r["mad"] - 1e-12)
        assert r["thr"] < 0.95 and b >= d["Z"] and near_count(corr, r["med"]) <= 8, (d, b)
        if d["Z"] == 150:
            assert b <= 160, (d, b)
        if d["Z"] == 250:
            assert b > CAP, (d, b)
    sweep = [band[f"madlock Z{z}"] for z in S.SWEEP]
    assert min(sweep) <= CAP - 2 and CAP + 2 <= max(sweep), sweep


def test_median_lock(C):
    for i, d, r in _rows(C, "medlock"):
        b = near_count(r["corr"], r["med"])
        assert r["med"] == 0.0 and r["thr"] < 0.95 and b >= d["Z"], (d, b)
        if d["Z"] == 150:
            assert b <= 170, (d, b)
        if d["Z"] == 250:
            assert b > CAP, (d, b)
    sweep = [near_count(r["corr"], r["med"]) for i, d, r in _rows(C, "medlock", sweep=True)]
    assert len(sweep) == len(S.SWEEP) and min(sweep) <= CAP - 2 and CAP + 2 <= max(sweep), sweep


def test_exact_repeats(C):
    for i, d, r in _rows(C, "repeats"):
        corr, p = r["corr"], d["period"]
        assert r["fallback"] and r["total"] == 5, d
        pk = [int(x) for x in r["peaks"]]
        if p == 38:                                                              # a multiple of the 19-lag energy chunk: exact repeats
            assert np.unique(corr).size == 38, d
            assert pk[0] >= corr.size - 38 and pk == [pk[0] - 38 * k for k in range(5)], pk    # equal values: higher index first
        else:                                                                    # repeats that differ in the last bits
            spread = max(np.ptp(corr[j::p]) for j in range(p))
            assert np.unique(corr).size > p and 0.0 < spread < 1e-12, (d, spread)
            assert len({x % p for x in pk}) == 1, pk


def test_saturation_edge(C):
    for band in range(4):
        below = above = 0
        for i, d, r in _rows(C, "satedge", band=band):
            u = r["med"] + 4.5 * 1.4826 * r["mad"]
            assert abs(u - d["target"]) < 1e-3 and 0.93 - 1e-3 <= u <= 0.97 + 1e-3, (d, u)
            assert (r["thr"] == 0.95) == (d["target"] > 0.95) and (r["thr"] < 0.95) == (u < 0.95), (d, u)
            below += u < 0.95; above += u > 0.95
        assert min(below, above) >= (4 if band == 0 else 1), (band, below, above)
    u0 = [d["target"] for i, d, r in _rows(C, "satedge", band=0)]
    assert min(u0) <= 0.9301 and max(u0) >= 0.9699


def test_crosser_at_threshold(C):
    for kind in ("white", "bandpassed"):
        rows = _rows(C, "crosser", kind=kind)
        for i, d, r in rows:
            p = d["lag"]
            assert d["halvings"] >= 45, d
            assert abs(r["corr"][p - 31:p + 32].max() - r["thr"]) < 1e-9, d
            assert (r["thr"] == 0.95) == (kind == "bandpassed"), d
            assert _peak_near(r, p) == (d["side"] == "at"), (d, r["peaks"])      # opposite outcomes an ulp of amplitude apart
        assert {d["band"] for _, d, _ in rows} == ({0} if kind == "white" else {0, 1, 2, 3})
        for i, d, r in _rows(C, "swap", kind=kind):
            p, q = d["lag"], d["lag2"]
            c = r["corr"]
            assert d["halvings"] >= 45 and q - p == 300 < S.NMS, d
            assert abs(c[q - 31:q + 32].max() - c[p - 31:p + 32].max()) < 1e-9 and c[p - 31:p + 32].max() > r["thr"] + 0.01, d
            assert _peak_near(r, q) == (d["side"] == "second"), (d, r["peaks"])
            assert _peak_near(r, p) or d["side"] == "second", (d, r["peaks"])


def test_ordinary_rows_are_far_from_every_capacity(C):
    for i, d, r in _rows(C, "ordinary"):
        corr = r["corr"]
        assert r["thr"] == 0.95 and r["med"] + 4.5 * 1.4826 * r["mad"] > 1.1, d
        assert near_count(corr, r["med"]) <= 8 and near_count(np.abs(corr - r["med"]), r["mad"]) <= 8, d
        assert near_count(corr, np.sort(corr)[-5]) <= 8 and np.count_nonzero(corr >= 0.95 - 2 * DELTA) <= 2, d
        if "planted" in d["name"]:
            assert not r["fallback"] and r["total"] == 1 and int(r["peaks"][0]) == d["lag"] and corr[d["lag"]] > 0.96, d


def test_screens_stay_inside_the_contract(C):
    moved = 0
    for i in (C.rows("crossers")[0], C.rows("satedge")[0], C.rows("ordinary")[-1]):
        r = C.ref[i]
        scr = S.screens(r["corr"], r["thr"], r["med"], r["peaks"], seed=i)       # asserts |screen - corr| <= DELTA itself
        assert tuple(scr) == S.PATTERNS
        for name, s in scr.items():
            e = s.astype(np.float64) - r["corr"]
            assert s.dtype == np.float32 and np.abs(e).max() <= DELTA
            assert (np.abs(e).max() >= 2.8e-5) == (name != "zero"), name        # the patterns use the bound they are given
        bins = lambda v: np.floor((v.astype(np.float64) + 1.0) * 128.0)          # noqa: E731
        moved += np.count_nonzero(bins(scr["bin edge"]) != bins(scr["zero"]))
        assert np.array_equal(scr["top five down"] < scr["zero"], np.isin(np.arange(r["corr"].size), np.argsort(r["corr"], kind="stable")[-5:]))
    assert moved >= 3                                                            # some values do change histogram bin


def test_saturation_margin_has_no_witness_row():
    """Why no row of the case set pins MARG (the slack of the picker's histogram proof that thr saturates at 0.95).

    The proof reads, from the 1/128-wide histogram of the screen, the bin bl of the lower middle order statistic and the largest j
    for which at least half the values lie j bins or more outside the median's bins, and declares thr = 0.95 when
    P = lo(bl) - MARG + 6.6717 (j/128 - MARG) >= 0.95 + 1e-6.  For a screen within a of the exact row the exact median is at least
    lo(bl) - a and the exact MAD at least j/128 - 2a, so the exact threshold is at least T = lo(bl) - a + 6.6717 (j/128 - 2a); a
    record can only be decided wrongly when P passes and T < 0.95.  P and T live on the lattice (bl + 6.6717 j)/128, and between
    the two conditions no lattice point falls -- not for MARG = DELTA (the shortened margin of the sensitivity check), not even
    for MARG = 0: the nearest point (bl 243, j 1) leaves T 1.3e-4 above 0.95.  So the margin's sufficiency rests on the argument
    in es_sync32.hip, and no screen within DELTA can show a shorter one wrong."""
    lo = lambda b: -1.0 + b / 128.0                                              # noqa: E731
    for a in (S.A, DELTA):
        for marg in (2.5 * DELTA, DELTA, 0.0):
            least = min(lo(bl) - a + 6.6717 * (j / 128.0 - 2 * a)
                        for bl in range(1, 255) for j in range(64)
                        if lo(bl) - marg + 6.6717 * (j / 128.0 - marg) >= 0.95 + 1e-6)
            assert least >= 0.95 + 1e-4, (a, marg, least)
