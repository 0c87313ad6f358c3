"""The sync picker against the CPU oracle on screens and records built to be its worst case (tests/sync_screen_cases.py).

sync_pick_row (es_sync32.hip) promises the float64 threshold and peak list for ANY float32 screen within DELTA = 3e-5 of the exact
correlation row.  es_pick_exact_batch takes the screen as an argument, so the promise is tested directly: every row of the case
set under every error pattern of |e| <= 2.9e-5, then under the project's own screens (two-kernel and fused), then at a batch large
enough for the fused grid to stride.  No tolerance anywhere: thr bit for bit, npeaks and the whole peak row exactly, all against
the oracle.  tests/test_sync_screen_cases.py shows (without a GPU) that the rows have the near-ties they are named after.

Flag codes (why a record went to sync_exact_row): 1 non-finite screen, 2 median band > 192, 3 MAD band > 192, 4 more than 64 rivals
of a candidate, 5 top-five band > 192.  The families reach: median lock 2, MAD lock 3, near-tied crossers 4, near-tied fallback 5,
and every row 1 once a NaN, an Inf and 1e31 are planted in its screen."""
import types

import numpy as np
import pytest
import torch

import sync_screen_cases as S

pytestmark = pytest.mark.gpu

TS = (1215, 2048, 3000)          # frame specialisation, two-wave window specialisation, generic multi-segment kernel


@pytest.fixture(scope="module", params=TS)
def G(request, engine, oracle):
    C = S.cases(request.param)
    dev = engine.device
    g = types.SimpleNamespace(C=C, T=C.T, R=len(C.info), engine=engine)
    g.y = torch.from_numpy(C.y.copy()).to(dev)
    g.y32 = g.y.float()
    g.band = torch.from_numpy(C.band).to(dev)
    per_row = [S.screens(r["corr"], r["thr"], r["med"], r["peaks"], seed=i) for i, r in enumerate(C.ref)]
    g.screens = {p: np.stack([s[p] for s in per_row]) for p in S.PATTERNS}
    g.safe = np.array([d["f32_safe"] for d in C.info])
    g.runs = {}                                                                  # name of a run -> (thr, peaks, npeaks, flags as numpy)
    return g


def _np(t):
    return t.cpu().numpy()


def _mismatches(C, thr, peaks, npeaks, rows=None):
    """Rows whose (thr bits, npeaks, whole peak row incl. the -1 tail) differ from the oracle's."""
    thr, peaks, npeaks = _np(thr), _np(peaks), _np(npeaks)
    bits = thr.view(np.uint64)
    rows = np.arange(len(C.info)) if rows is None else np.asarray(rows)
    want = C.thr.view(np.uint64)
    bad = []
    for j, i in enumerate(rows):
        if bits[j] != want[i] or npeaks[j] != C.npeaks[i] or not np.array_equal(peaks[j], C.peaks[i]):
            bad.append((C.info[i]["name"], C.info[i]["band"], float(thr[j]), float(C.thr[i]), int(npeaks[j]), int(C.npeaks[i]),
                        peaks[j][:6].tolist(), C.peaks[i][:6].tolist()))
    return bad


def _non_finite(G):
    scr = G.screens["zero"].copy()
    n = scr.shape[1]
    scr[:, n // 7] = np.nan; scr[:, n // 2] = np.inf; scr[:, n - 3] = 1e31
    return scr


def _run(G, name):
    """One launch per name, kept: a screen pattern or "non-finite" through es_pick_exact_batch, "two-kernel" (es_xcorr32_batch +
    es_pick_exact_batch) and "fused" (es_sync_fused_batch) on y32 = float32(y)."""
    if name not in G.runs:
        e = G.engine
        if name == "fused":
            out = e.sync_fused(G.y, G.y32, G.band)
        elif name == "two-kernel":
            G.corr32 = e.xcorr32(G.y32, G.band)
            out = e.pick_exact(G.corr32, G.y, G.band)
        else:
            scr = _non_finite(G) if name == "non-finite" else G.screens[name]
            out = e.pick_exact(torch.from_numpy(np.ascontiguousarray(scr)).to(e.device), G.y, G.band)
        torch.cuda.synchronize()
        G.runs[name] = (out[0], out[1], out[2], _np(out[3]))
    return G.runs[name]


# ---------------------------------------------------------------------------------------------------------------- a
def test_float64_path(G):
    """engine.xcorr is bit-equal to oracle.ncc, engine.pick to the oracle's threshold and peaks: the near-tie rows through
    es_xcorr_kernel / es_pick_kernel too."""
    corr = G.engine.xcorr(G.y, G.band)
    want = np.stack([r["corr"] for r in G.C.ref])
    assert np.array_equal(_np(corr).view(np.uint64), want.view(np.uint64))
    thr, peaks, npeaks = G.engine.pick(corr)
    assert not _mismatches(G.C, thr, peaks, npeaks)


# ---------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("pattern", S.PATTERNS)
def test_worst_case_screens(G, pattern):
    scr = G.screens[pattern]
    want = np.stack([r["corr"] for r in G.C.ref])
    assert np.abs(scr.astype(np.float64) - want).max() <= S.DELTA               # the contract, a condition of the test
    thr, peaks, npeaks, flags = _run(G, pattern)
    assert not _mismatches(G.C, thr, peaks, npeaks), pattern
    assert set(np.unique(flags)) <= {0, 2, 3, 4, 5}                              # a finite screen is never "non-finite"


def test_non_finite_screens(G):
    """A NaN, an Inf and 1e31 planted in every row's screen: code 1, and the answer from float64 re-evaluations alone."""
    thr, peaks, npeaks, flags = _run(G, "non-finite")
    assert (flags == 1).all()
    assert not _mismatches(G.C, thr, peaks, npeaks)


# ---------------------------------------------------------------------------------------------------------------- c
def test_own_screens(G):
    """The project's own screens: xcorr32 + pick_exact and the fused kernel on y32 = float32(y)."""
    safe = np.flatnonzero(G.safe)
    t2, tf = _run(G, "two-kernel"), _run(G, "fused")
    want = np.stack([r["corr"] for r in G.C.ref])
    err = np.abs(_np(G.corr32).astype(np.float64) - want)[safe]
    assert err.max() <= S.DELTA, err.max()                                       # the screen's own bound on float32-safe records
    # every row goes through both: samples of 1e20 and 1e30 overflow the float32 energies, which must flag the record (expected
    # code 1), never hand a wrong screen to the picker -- the assertion is the result
    assert not _mismatches(G.C, t2[0], t2[1], t2[2]), "two-kernel"
    assert not _mismatches(G.C, tf[0], tf[1], tf[2]), "fused"
    f2, ff = t2[3], tf[3]
    assert np.array_equal(f2[safe], ff[safe]), [(G.C.info[i]["name"], f2[i], ff[i]) for i in safe if f2[i] != ff[i]]


# ---------------------------------------------------------------------------------------------------------------- d
def _flags_of(G, name):
    return _run(G, name)[3]


def test_every_branch_ran(G):
    C = G.C
    zero = _flags_of(G, "zero")
    seen = set(np.unique(zero)) | set(np.unique(_flags_of(G, "non-finite")))
    assert seen >= {0, 1, 2, 3, 4, 5}, seen
    name = lambda i: (C.info[i]["name"], C.info[i]["band"], int(zero[i]))        # noqa: E731
    expect = []                                                                  # (rows, code) under e = 0
    expect.append((C.rows("medlock", Z=250), 2)); expect.append((C.rows("medlock", Z=150), 0))
    expect.append((C.rows("madlock", Z=250), 3)); expect.append((C.rows("madlock", Z=150), 0))
    expect.append((C.rows("fallback", Z=250), 5)); expect.append((C.rows("fallback", Z=100), 0))
    # near-tied crossers: a plateau candidate has (values within DELTA of it) - 1 rivals, and at most 64 fit: Z <= 65 settles from
    # the screen, Z >= 66 cannot (tests/test_sync_screen_cases.py: the count is Z for 63 .. 67, 50 - 59 below, >= 99 at Z = 100)
    expect.append(([i for i in C.rows("crossers") if C.info[i]["Z"] >= 66], 4))
    expect.append(([i for i in C.rows("crossers") if C.info[i]["Z"] <= 65], 0))
    for rows, code in expect:
        assert rows and all(zero[i] == code for i in rows), (code, [name(i) for i in rows])
    # both sides of each capacity, under at least one screen pattern
    sweeps = {"medlock": (C.rows("medlock", sweep=True), 2),
              "madlock": ([i for i in C.rows("madlock") if C.info[i]["Z"] in S.SWEEP and "frac" not in C.info[i]["name"]], 3),
              "fallback": ([i for i in C.rows("fallback") if C.info[i]["Z"] in S.SWEEP], 5),
              "crossers": ([i for i in C.rows("crossers") if 63 <= C.info[i]["Z"] <= 67], 4)}
    for fam, (rows, code) in sweeps.items():
        got = set()
        for p in S.PATTERNS:
            got |= set(_flags_of(G, p)[rows].tolist())
        assert got == {0, code}, (fam, got)
    # saturation edge: both outcomes of the threshold
    sat = C.rows("satedge")
    thr = _np(_run(G, "zero")[0])[sat]
    assert (thr == 0.95).any() and (thr < 0.95).any()
    # ordinary rows: nothing in them is within reach of a capacity (test_ordinary_rows_are_far_from_every_capacity), so no rule
    # of the picker can flag them, whatever the screen
    for p in S.PATTERNS + ("two-kernel", "fused"):
        assert not _flags_of(G, p)[C.rows("ordinary")].any(), p


# ---------------------------------------------------------------------------------------------------------------- e
def test_capacity_of_a_launch(G):
    """The row set repeated to about 4 x num_cu x 32 records, so that the fused grid strides: same answers as the single pass.
    sync_exact_row is slow by design, so the rows the single pass flagged keep their place only in the first and the last two
    repetitions (a few hundred flagged rows per launch); in between an unflagged row stands in for them."""
    e, C = G.engine, G.C
    single = _run(G, "fused")
    assert not _mismatches(C, single[0], single[1], single[2])
    flagged = single[3] != 0
    reps = -(-4 * torch.cuda.get_device_properties(e.device).multi_processor_count * 32 // G.R)
    idx = np.tile(np.arange(G.R), reps).reshape(reps, G.R)
    idx[2:-2, flagged] = C.rows("ordinary")[0]
    idx = idx.reshape(-1)
    assert np.count_nonzero(flagged[idx]) <= 400
    sel = torch.from_numpy(idx).to(e.device)
    y = G.y.index_select(0, sel); y32 = G.y32.index_select(0, sel); band = G.band.index_select(0, sel)
    thr, peaks, npeaks, flags = e.sync_fused(y, y32, band)
    torch.cuda.synchronize()
    for got, one in ((thr, single[0]), (peaks, single[1]), (npeaks, single[2])):
        assert torch.equal(got, one.index_select(0, sel))
    assert np.array_equal(_np(flags), single[3][idx])
