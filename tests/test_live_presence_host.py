"""CPU: the host side of the presence test on live windows -- the third companion header's place in the binding and the
library's exports, presence.window_rows and presence.live_span against loops written out here, the reach clipping at the top of the
counter range, presence.live_model on CPU-oracle rows against presence_model, and every ValueError of LiveMonitor.presence,
LiveIdentifier.presence and WatermarkIdentifier.presence_batch, raised before an engine exists."""
import ctypes

import numpy as np
import pytest

import echoseal_amd._native as nat
import presence_cases as PC
from echoseal_amd import presence as pr
from echoseal_amd.acquire import origin_of
from echoseal_amd.detector import LiveMonitor, WatermarkDetector
from echoseal_amd.identify import LiveIdentifier, WatermarkIdentifier
from echoseal_amd.monitor import host_table

FL, CTR_END = 1215, 1 << 32
NAMES = {"es_warp_fold_at_batch", "es_warp_score_at_batch"}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    """Two Presence results, field for field; floats by their bits."""
    assert (a is None) == (b is None)
    if a is None:
        return
    assert (a.detected, a.ctr, a.phase, a.ctr0, a.frames, a.phases, a.skew, a.hypotheses) == \
           (b.detected, b.ctr, b.phase, b.ctr0, b.frames, b.phases, b.skew, b.hypotheses)
    assert np.array_equal(_bits([a.score, a.drift_ppm]), _bits([b.score, b.drift_ppm])) and np.array_equal(_bits(a.null), _bits(b.null))


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_the_live_presence_header_is_bound_beside_the_others():
    assert len(nat.DECLARATIONS) == len(nat.SIGNATURES) == 56 and nat.ES_ABI_VERSION == 2
    assert set(nat.PRESENCE_DECLARATIONS) == {"es_phase_fold_batch", "es_hop_score_batch"}
    assert set(nat.WARP_DECLARATIONS) == {"es_warp_fold_batch", "es_warp_score_batch"}
    assert set(nat.LIVE_PRESENCE_DECLARATIONS) == set(nat.LIVE_PRESENCE_SIGNATURES) == NAMES
    others = set(nat.DECLARATIONS) | set(nat.PRESENCE_DECLARATIONS) | set(nat.WARP_DECLARATIONS)
    assert not NAMES & others
    assert not set(nat.LIVE_PRESENCE_CONSTANTS) & (set(nat.CONSTANTS) | set(nat.PRESENCE_CONSTANTS) | set(nat.WARP_CONSTANTS))
    from test_abi_binding import POINTERS, SCALARS
    for name, params in nat.LIVE_PRESENCE_DECLARATIONS.items():
        assert {t for t, _ in params} <= SCALARS | POINTERS, name
        assert params[0] == ("es_ctx*", "ctx") and params[-1] == ("void*", "stream") and name.endswith("_batch"), name
        assert not any(p == "stream" for _, p in params[:-1]) and len(nat.LIVE_PRESENCE_SIGNATURES[name][1]) == len(params)
        for (ctype, _), arg in zip(params, nat.LIVE_PRESENCE_SIGNATURES[name][1]):
            assert (arg is nat.c_int64) == (ctype == "int64_t") and (arg is nat.c_int) == (ctype == "int"), (name, ctype)
        assert ("const int64_t*", "row_dev") in params and ("const int64_t*", "col_dev") in params and ("const int32_t*", "nlag_dev") in params
    score = dict((p, t) for t, p in nat.LIVE_PRESENCE_DECLARATIONS["es_warp_score_at_batch"])
    assert score["HR"] == "int64_t" and score["hop_row_dev"] == "const int32_t*"
    for path in (nat.HEADER_PATH, nat.PRESENCE_HEADER_PATH, nat.WARP_HEADER_PATH):          # the other three headers are as they were
        assert "es_warp_fold_at" not in open(path).read() and "es_warp_score_at" not in open(path).read()


def test_both_symbols_are_exported_by_the_built_library():
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name


# ---------------------------------------------------------------------------------------------------------------- window_rows
def test_window_rows_against_a_loop():
    rows, stride = 11, 40
    corr = np.random.default_rng(1).uniform(-1, 1, (rows, stride))
    for rows4, col, nlag in [((7, 2, 9, 0), 0, 40), ((7, 2, 9, 0), 5, 12), ((3, 3, 3, 3), 39, 9), ((0, 1, 2, 3), 40, 5), ((10, 9, 8, 7), 1, -4),
                             ((10, 9, 8, 7), 17, 100)]:
        got = pr.window_rows(corr, rows4, col, nlag)
        n = min(max(nlag, 0), stride - col)
        want = np.zeros((4, n))
        for band in range(4):
            for i in range(n):
                want[band, i] = corr[rows4[band], col + i]
        assert got.shape == (4, n) and np.array_equal(_bits(got), _bits(want)), (rows4, col, nlag)
    for rows4, col in [((0, 1, 2, -1), 0), ((0, 1, 2, rows), 0), ((0, 1, 2, 3), -1), ((0, 1, 2, 3), stride + 1)]:       # not addressable: no lags
        assert pr.window_rows(corr, rows4, col, 10).shape == (4, 0)
    with pytest.raises(ValueError):
        pr.window_rows(corr, (0, 1, 2), 0, 10)
    assert pr.table_rows([2, 0, 3, 1], 5) == [21, 23, 20, 22]               # entry `band` = 4 s + j with bands[j] == band
    with pytest.raises(ValueError):
        pr.table_rows([0, 1, 2, 2], 0)


# ---------------------------------------------------------------------------------------------------------------- live_span
@pytest.mark.parametrize("origin", [0, 7, 4_000_000_000])
def test_the_counter_of_slot_0_lies_in_the_live_span(origin):
    """A window that starts at absolute sample w0 (a multiple of 1216) of a stream whose frame k carries counter origin + k: the frame
    that starts at w0 + phi carries origin + round((w0 + phi) / 1215), the rounding of plan_at and origin_of."""
    for w0 in [1216 * k for k in (0, 1, 2, 3, 17, 607, 608, 1214, 1215, 1216, 100_000)]:
        lo, hi = pr.live_span(origin, w0, 3)
        assert hi == lo + 2
        for phi in range(FL):
            a = w0 + phi
            ctr = origin + a // FL + (1 if 2 * (a % FL) > FL else 0)        # round(a / 1215), written out: 1215 is odd, no ties
            assert lo <= ctr < hi, (w0, phi)
            assert origin_of(ctr, phi, w0) == origin


def test_live_span_is_clipped_at_the_top_of_the_counter_range():
    top = CTR_END - 1
    assert pr.live_span(top, 0, 1) == (top, CTR_END)                        # the one window of the last counter
    assert pr.live_span(top, 0, 2) == (top, top)                            # two slots from it would pass 2^32: nothing to search
    assert pr.live_span(top - 5, 0, 5) == (top - 5, top - 3)                # hi + J - 1 = 2^32 - 4 + 4: just fits
    assert pr.live_span(top - 5, 0, 6) == (top - 5, top - 4)                # lowered by one
    assert pr.live_span(top - 5, 0, 7) == (top - 5, top - 5)
    assert pr.live_span(top, 1216 * 10, 4) == (CTR_END, CTR_END)            # past the end: empty, never reversed
    for origin, w0, J in [(top - 5, 0, 6), (top - 40, 1216 * 30, 8), (0, 0, 1)]:
        lo, hi = pr.live_span(origin, w0, J)
        assert 0 <= lo <= hi <= CTR_END and (hi == lo or hi + J - 1 <= CTR_END)
        pr.check_reach((lo, hi), J * FL + 62)                               # what presence_model asks of a span
    with pytest.raises(ValueError, match="2\\^32"):
        pr.check_reach((top - 5, top - 2), 6 * FL + 62)                     # the unclipped span is what check_reach refuses


# ---------------------------------------------------------------------------------------------------------------- live_model
@pytest.fixture(scope="module")
def clip_a(oracle):
    return PC.oracle_rows(oracle, PC.cached("marked", "A"))


def test_live_model_on_a_window_from_sample_0_is_presence_model(clip_a):
    corr, nlag = clip_a
    bands = [2, 0, 3, 1]
    hist = np.full((8, nlag + 100), np.nan)                                 # stream 1 of two; what is not its window must never be read
    for band in range(4):
        hist[4 + bands.index(band), :nlag] = corr[band]
    n = nlag + 62
    want = pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, phases=8, decoys=32)
    assert want.detected and (want.ctr, want.phase) == PC.FOUND
    _same(pr.live_model(hist, 1, bands, 0, 0, n, PC.KEY, span=PC.SPAN, phases=8, decoys=32), want)
    _same(pr.live_model(hist, 1, bands, 0, 0, n, PC.KEY, origin=-1, span=PC.SPAN), want)
    drift = pr.live_model(hist, 1, bands, 0, 0, n, PC.KEY, span=PC.SPAN, drift_ppm=300)
    _same(drift, pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN, drift_ppm=300))
    assert drift.hypotheses is not None
    # with the stream's origin the span is live_span's: the clip was marked from counter 0 and cut at 777, so frame 1 leads
    got = pr.live_model(hist, 1, bands, 0, 0, n, PC.KEY, origin=0, phases=8, decoys=32)
    _same(got, pr.presence_model(corr, nlag, PC.KEY, span=(0, 2), phases=8, decoys=32))
    assert got.detected and (got.ctr, got.phase, got.ctr0) == (1, 438, 1)
    assert pr.live_model(hist, 1, bands, 0, 0, 62 + FL - 1, PC.KEY) is None                 # no whole slot


def test_live_model_reads_the_window_where_it_lies(clip_a):
    """The same rows as a window that starts at absolute sample w0 = 2 * 1216 of a table whose column 0 is absolute lag 1216."""
    corr, nlag = clip_a
    bands, base, w0 = [0, 1, 2, 3], 1216, 2 * 1216
    hist = np.full((4, nlag + 1216 + 7), np.nan)
    hist[:, w0 - base:w0 - base + nlag] = corr
    got = pr.live_model(hist, 0, bands, base, w0, w0 + nlag + 62, PC.KEY, span=PC.SPAN)
    want = pr.presence_model(corr, nlag, PC.KEY, span=PC.SPAN)
    assert got.ctr0 == origin_of(want.ctr, want.phase, w0) == max(0, 1 - (2 * (w0 + 438) + FL) // (2 * FL))
    got.ctr0 = want.ctr0
    _same(got, want)


# ---------------------------------------------------------------------------------------------------------------- refusals, no engine
BAD = [(dict(span=(5, 4)), "reversed"), (dict(span=(0, CTR_END + 1)), "outside"), (dict(span=(0.0, 4)), "integers"), (dict(span=7), "pair"),
       (dict(phases=0), "phases"), (dict(phases=1216), "phases"), (dict(phases=2.0), "phases"), (dict(decoys=-1), "decoys"),
       (dict(decoys=True), "decoys"), (dict(drift_ppm=-1.0), "drift_ppm"), (dict(drift_ppm=float("nan")), "drift_ppm"),
       (dict(drift_ppm="3"), "drift_ppm")]


@pytest.mark.parametrize("bad, match", BAD)
def test_bad_arguments_are_refused_without_an_engine(bad, match):
    det, ident = WatermarkDetector(PC.KEY, list_size=8), WatermarkIdentifier([PC.KEY, PC.OTHER_KEY], list_size=8)
    mon = LiveMonitor(det, host_table(2, 3648, 1300, fs_target=48_000))
    live = LiveIdentifier(ident, host_table(2, 3648, 1300, fs_target=48_000), memo_slots=0)
    clip = np.zeros(5000, np.float32)
    for call in (lambda: mon.presence(**bad), lambda: live.presence(**bad), lambda: ident.presence(clip, 48_000, **bad),
                 lambda: ident.presence_batch([clip, clip[:3000]], 48_000, **bad)):
        with pytest.raises(ValueError, match=match):
            call()
    assert det._engine is None and ident._det._engine is None


def test_streams_and_reach_are_checked_without_an_engine():
    det, ident = WatermarkDetector(PC.KEY, list_size=8), WatermarkIdentifier([PC.KEY, PC.OTHER_KEY], list_size=8)
    tab = host_table(4, 3648, 1300, fs_target=48_000, ctr0=[None, 5, None, None])
    tab.live[2] = False
    tab.n_host[:2] = 62 + 2 * FL + 3                                        # two whole slots in the windows of streams 0 and 1
    for obj in (LiveMonitor(det, tab), LiveIdentifier(ident, tab, memo_slots=0)):
        with pytest.raises(ValueError, match="closed"):
            obj.presence([2])
        with pytest.raises(ValueError, match="twice"):
            obj.presence([0, 0])
        with pytest.raises(ValueError, match="outside"):
            obj.presence([4])
        with pytest.raises(ValueError, match="outside"):
            obj.presence([-1])
        with pytest.raises(ValueError, match="2\\^32"):
            obj.presence([0], span=(CTR_END - 4, CTR_END))                  # stream 0 has no origin: two frames from the last origin pass 2^32
        with pytest.raises(ValueError, match="drift_ppm"):
            obj.presence([0], drift_ppm=500_000.0)                          # more than a frame of skew across the window
        assert obj.presence([3]) == [None] and obj.presence([]) == []       # no whole slot, nobody named: no GPU work either
    assert tab.n_host.tolist()[:2] == [62 + 2 * FL + 3] * 2 and tab.origin_host.tolist() == [-1, 5, -1, -1]
    clip = np.zeros(62 + 2 * FL, np.float32)
    with pytest.raises(ValueError, match="2\\^32"):
        ident.presence(clip, 48_000, span=(CTR_END - 4, CTR_END))
    with pytest.raises(ValueError, match="ctr0"):
        ident.presence_batch([clip, clip], 48_000, [1], span=PC.SPAN)
    with pytest.raises(ValueError, match="ctr0"):
        ident.presence(clip, 48_000, -1)
    with pytest.raises(ValueError, match="drift_ppm"):
        ident.presence(clip, 48_000, drift_ppm=500_000.0)
    assert det._engine is None and ident._det._engine is None
