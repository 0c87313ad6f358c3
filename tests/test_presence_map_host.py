"""CPU: the host side of the presence timeline -- the pick header's place in the binding, pick_model against a loop written
out here and against pick_hypotheses, map_windows against a loop, every argument check without an engine, stretches on hand-made window
lists, and map_model on the spliced clips of tests/presence_map_cases.py rebuilt with the CPU oracle.  Scores are printed, not asserted."""
import math
import os

import numpy as np
import pytest

import echoseal_amd._native as nat
import presence_cases as PC
import presence_map_cases as MC
from echoseal_amd import presence as pr
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

FL = 1215


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_the_pick_header_has_tables_of_its_own():
    assert len(nat.DECLARATIONS) == 56
    assert list(nat.PICK_DECLARATIONS) == ["es_fold_pick_batch"] and nat.PICK_CONSTANTS == {"ES_PICK_MAX_H": 64} and nat.ES_PICK_MAX_H == 64
    assert [n for _, n in nat.PICK_DECLARATIONS["es_fold_pick_batch"]] == ["ctx", "fold_dev", "B", "D", "nwarp_dev", "H", "hyp_dev", "val_dev", "stream"]
    res, args = nat.PICK_SIGNATURES["es_fold_pick_batch"]
    from ctypes import c_int, c_int64, c_void_p
    assert res is c_int and args == [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
    others = [nat.SIGNATURES, nat.PRESENCE_SIGNATURES, nat.WARP_SIGNATURES, nat.LIVE_PRESENCE_SIGNATURES]
    assert not any(set(nat.PICK_SIGNATURES) & set(t) for t in others) and "ES_PICK_MAX_H" not in nat.CONSTANTS
    assert pr.PICK_MAX_H == nat.ES_PICK_MAX_H
    with open(os.path.join(os.path.dirname(nat.HEADER_PATH), "..", "echoseal_amd", "csrc", "Makefile")) as f:
        rule = next(line for line in f if line.startswith("%.o:"))
    assert "../../include/echoseal_pick.h" in rule.split()


# ---------------------------------------------------------------------------------------------------------------- the pick
def _pick_loop(fold, nwarp, H):
    """The definition of include/echoseal_pick.h, one comparison at a time."""
    B, D, _ = fold.shape
    hyp, val = np.full((B, H, 2), -1, np.int32), np.full((B, H), -math.inf)
    for b in range(B):
        nw = D if nwarp is None else min(max(int(nwarp[b]), 0), D)
        taken = set()
        for h in range(H):
            best = None
            for d in range(nw):
                for phi in range(FL):
                    v = float(fold[b, d, phi])
                    if (d, phi) in taken or v != v or v == -math.inf:
                        continue
                    if best is None or v > best[0]:                         # rows ascend, phases ascend: of equal values the first stays
                        best = (v, d, phi)
            if best is None:
                break
            taken.add(best[1:])
            hyp[b, h] = best[1:]
            val[b, h] = fold[b, best[1], best[2]]
    return hyp, val


@pytest.mark.parametrize("name", list(MC.edge_folds()))
def test_pick_model_is_the_written_out_loop(name):
    fold, nwarp = MC.edge_folds()[name]
    for H in (1, 9):
        hyp, val = pr.pick_model(fold, nwarp, H)
        want_hyp, want_val = _pick_loop(fold, nwarp, H)
        assert hyp.dtype == np.int32 and val.dtype == np.float64 and hyp.shape == (3, H, 2) and val.shape == (3, H)
        assert np.array_equal(hyp, want_hyp) and np.array_equal(_bits(val), _bits(want_val)), name
    assert not np.isnan(pr.pick_model(fold, nwarp, 64)[1]).any()


def test_pick_model_is_pick_hypotheses_on_the_folds_of_the_public_calls():
    rng = np.random.default_rng(27)
    fold = rng.standard_normal((4, 5, FL)).round(1)                         # rounded: many equal values
    fold[0, 2] = fold[1, 0] = fold[1, 4] = -np.inf; fold[2] = -np.inf
    nwarp = [5, 5, 3, 2]
    for H in (1, 8, 64):
        hyp, _ = pr.pick_model(fold, nwarp, H)
        for b in range(4):
            want = pr.pick_hypotheses(fold[b, :nwarp[b]], H)
            assert [tuple(e) for e in hyp[b].tolist() if e[0] >= 0] == want and (hyp[b, len(want):] == -1).all()
    assert (pr.pick_model(fold, nwarp, 8)[0][2] == -1).all()
    for bad in (0, 65, 2.0, True):
        with pytest.raises(ValueError):
            pr.pick_model(fold, nwarp, bad)
    with pytest.raises(ValueError):
        pr.pick_model(fold, [5, 5], 8)


# ---------------------------------------------------------------------------------------------------------------- the windows
@pytest.mark.parametrize("W,S", [(40, 20), (5, 5), (7, 3), (4, 1)])
def test_map_windows_is_the_written_out_loop(W, S):
    for J in (0, 1, W, W + 1, W + S, W + S + 1):
        for extra in (0, 1214):
            nlag = FL * J + extra
            got = pr.map_windows(nlag, W, S)
            if J == 0:
                want = []
            elif J <= W:
                want = [(0, 0, nlag)]
            else:
                starts, s = [], 0
                while s <= J - W:
                    starts.append(s)
                    s += S
                if starts[-1] != J - W:
                    starts.append(J - W)
                want = [(s, FL * s, FL * W) for s in starts]
            assert got == want, (J, extra)
            assert all(col + n <= nlag for _, col, n in got) and (not got or got[-1][1] + FL * (got[-1][2] // FL) == FL * J)
    assert pr.map_windows(-5, W, S) == []


def test_window_span_follows_the_window_and_is_lowered_at_2_32():
    E = 1 << 32
    assert pr.window_span((0, 4096), 0, 40) == (0, 4096) and pr.window_span((0, 4096), 20, 40) == (20, 4116)
    assert pr.window_span((7, 9), 100, 40) == (107, 109)
    assert pr.window_span((E - 100, E), 0, 40) == (E - 100, E - 39) and pr.window_span((E - 100, E), 80, 40) == (E - 20, E - 20)
    assert pr.window_span((E - 100, E), 200, 40) == (E, E) and pr.window_span((E - 50, E), 0, 1) == (E - 50, E)
    for lo, hi in [pr.window_span((E - 100, E), s, 40) for s in range(0, 200, 7)]:
        assert lo <= hi and (hi == lo or hi + 40 - 1 <= E)
    with pytest.raises(ValueError):
        pr.window_span((5, 3), 0, 1)


@pytest.mark.parametrize("kw", [dict(window=40.0), dict(step=2.5), dict(confirm="2"), dict(window=True), dict(step=0), dict(step=-1),
                                dict(window=10, step=11), dict(window=0), dict(confirm=0), dict(phases=65), dict(phases=0), dict(phases=8.0),
                                dict(decoys=-1), dict(drift_ppm=-1.0), dict(drift_ppm=float("nan")), dict(drift_ppm=30_000), dict(span=(5, 3)),
                                dict(span=(0, (1 << 32) + 1)), dict(ctr0=-1)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_every_bad_argument_is_refused_before_an_engine_exists(kw):
    """No engine is handed in and none can be made here: a ValueError, never the NativeError of a missing GPU."""
    clip = np.zeros(3 * 48_000, np.float32)
    det = WatermarkDetector(PC.KEY)
    ident = WatermarkIdentifier([PC.KEY, PC.OTHER_KEY])
    for who in (det, ident):
        kw1 = dict(kw)
        ctr0 = kw1.pop("ctr0", None)
        with pytest.raises(ValueError):
            who.presence_map(clip, 48_000, ctr0, **kw1)
        with pytest.raises(ValueError):
            who.presence_map_batch([clip, clip[:5000]], 48_000, None if ctr0 is None else [ctr0, None], **kw1)
    grid = {k: kw[k] for k in ("window", "step", "confirm", "phases") if k in kw}
    if grid:
        with pytest.raises(ValueError):
            pr.check_map(*[grid.get(k, d) for k, d in (("window", 40), ("step", 20), ("confirm", 2), ("phases", 8))])
        if "confirm" not in grid:
            with pytest.raises(ValueError):
                pr.map_model(np.zeros((4, 3 * FL)), 3 * FL, PC.KEY, **grid)
    assert pr.check_map(40, 20, 2, 8) == (40, 20, 2, 8) and pr.check_map(1, 1, 1, 64) == (1, 1, 1, 64)


# ---------------------------------------------------------------------------------------------------------------- stretches
W, S = 40, 20


def _win(w, t, detected=True, score=0.5, phase=100):
    """A hand-made verdict of window w (column 1215 S w) whose anchor is t: ctr from col + phase - 1215 ctr = t."""
    col = FL * S * w
    if t is None:
        return pr.Presence(False, -math.inf, np.zeros(4), -1, -1, -1, W, [])
    assert (col + phase - t) % FL == 0
    return pr.Presence(detected, score, np.zeros(4), (col + phase - t) // FL, phase, 0, W, [phase])


def _stretches(wins, drift=0.0, confirm=2):
    cols = [FL * S * w for w in range(len(wins))]
    return pr.stretches(wins, cols, [FL * W] * len(wins), drift, confirm)


def _ends(st):
    return [(s.first, s.last, s.confirmed) for s in st]


def test_a_lone_detected_window_confirms_nothing():
    T = 100 - 3 * FL
    st, sp, marked = _stretches([_win(0, T, False), _win(1, T), _win(2, T, False), None])
    assert _ends(st) == [(1, 1, False)] and sp == [] and marked == 0
    assert (st[0].start, st[0].end, st[0].t, st[0].ctr0) == (FL * S, FL * (S + W), T, pr.origin_of(S + 3, 100, FL * S))
    st, _, marked = _stretches([_win(0, T, False), _win(1, T), _win(2, T, False)], confirm=1)
    assert _ends(st) == [(1, 1, True)] and marked == FL * W
    assert _stretches([])[0] == [] and _stretches([None, _win(1, None)]) == ([], [], 0)


def test_a_gap_ends_a_stretch_and_a_splice_joins_confirmed_ones_across_anything():
    T = 100 - FL
    wins = [_win(0, T, score=0.9), _win(1, T, score=0.4), _win(2, T, False), _win(3, T - 7 * FL), _win(4, T, score=0.6), _win(5, T, score=0.7), _win(6, T)]
    st, sp, marked = _stretches(wins)
    assert _ends(st) == [(0, 1, True), (3, 3, False), (4, 6, True)]         # the undetected window, then a lone window on another grid
    assert st[0].score == 0.4 and st[2].score == 0.5 and st[0].end == FL * (S + W) and st[2].start == 4 * FL * S
    assert sp == [pr.Splice(FL * S, FL * (4 * S + W), 0)]                   # same grid on both sides: nothing is missing
    assert marked == (st[0].end - st[0].start) + (st[2].end - st[2].start)
    st, sp, marked = _stretches(wins[:3] + [_win(3, T)] + wins[4:])
    assert _ends(st) == [(0, 1, True), (3, 6, True)] and marked == (FL * (S + W)) + (FL * (6 * S + W) - FL * 3 * S)
    st, _, marked = _stretches([_win(w, T) for w in range(4)])
    assert _ends(st) == [(0, 3, True)] and marked == FL * (3 * S + W)      # overlapping windows are counted once


@pytest.mark.parametrize("drift,tol", [(0.0, 1), (300, 1 + math.ceil(300 * FL * S / 1e6)), (0.5, 2)])
def test_the_tolerance_holds_at_tol_and_breaks_at_tol_plus_one(drift, tol):
    assert tol == 1 + -(-int(drift * 10) * FL * S // 10 ** 7)               # exact: the ceiling of drift_ppm (col_b - col_a) / 10^6
    T = 100 - FL
    for sign in (1, -1):
        ph = 100 + sign * tol
        st, sp, _ = _stretches([_win(0, T), _win(1, T + sign * tol, phase=ph)], drift)
        assert _ends(st) == [(0, 1, True)] and sp == []
        ph = 100 + sign * (tol + 1)
        st, sp, _ = _stretches([_win(0, T), _win(1, T + sign * (tol + 1), phase=ph)], drift)
        assert _ends(st) == [(0, 0, False), (1, 1, False)] and sp == []
    assert pr.consistent(0, 0, tol, FL * S, drift) and not pr.consistent(0, 0, tol + 1, FL * S, drift) and pr.consistent(tol, FL * S, 0, 0, drift)
    walk = [_win(w, T + w * tol, phase=100 + w * tol) for w in range(4)]    # each window against the one before it, not against the first
    assert _ends(_stretches(walk, drift)[0]) == [(0, 3, True)]


def test_an_insertion_is_a_negative_removal():
    T = 100 - FL
    wins = [_win(0, T), _win(1, T), _win(2, T + 5000, phase=240), _win(3, T + 5000, phase=240)]
    st, sp, marked = _stretches(wins)
    assert _ends(st) == [(0, 1, True), (2, 3, True)] and sp == [pr.Splice(FL * S, FL * (2 * S + W), -5000)]
    assert marked == FL * (3 * S + W)
    cut = [_win(0, T), _win(1, T), _win(2, T - 12_650, phase=100 - 12_650 % FL + FL), _win(3, T - 12_650, phase=100 - 12_650 % FL + FL)]
    assert _stretches(cut)[1] == [pr.Splice(FL * S, FL * (2 * S + W), 12_650)]


# ---------------------------------------------------------------------------------------------------------------- the clips
def _show(name, m):
    for w, p in enumerate(m.windows):
        print(f"{name} window {w} (slot {m.starts[w]}): detected {p.detected}, own {p.score:.4f}, decoy max {p.null.max():.4f}, ctr {p.ctr}, phase {p.phase}")


def test_map_model_finds_the_splice_of_clip_a(oracle):
    corr, nlag = MC.rows(oracle, "spliced", "A")
    m = pr.map_model(corr, nlag, PC.KEY, span=MC.SPAN)
    _show("A", m)
    assert m.starts == [0, 20, 40, 60, 80, 100, 120, 140, 146] and all(p.detected and p.frames == 40 for p in m.windows)
    assert [(s.first, s.last, s.confirmed, s.t, s.ctr0) for s in m.stretches] == [(0, 2, True, MC.T0, 1), (3, 8, True, MC.T0 - MC.CUT_LEN, 11)]
    assert [(p.ctr, p.phase) for p in m.windows[:3]] == [(1, 438), (21, 438), (41, 438)] and (m.windows[3].ctr, m.windows[3].phase) == (72, 1153)
    assert m.splices == [pr.Splice(40 * FL, 100 * FL, MC.CUT_LEN)]
    assert m.splices[0].lo <= MC.CUT_AT < m.splices[0].hi and m.marked == 186 * FL
    assert (m.stretches[0].start, m.stretches[0].end, m.stretches[1].start, m.stretches[1].end) == (0, 80 * FL, 60 * FL, 186 * FL)
    assert m.stretches[1].score == min(p.score for p in m.windows[3:]) and m.windows[4].ctr0 == pr.origin_of(92, 1153, 80 * FL) == 11
    other = pr.map_model(corr, nlag, PC.OTHER_KEY, span=MC.SPAN)
    assert not any(s.confirmed for s in other.stretches) and other.marked == 0 and other.splices == []


def test_map_model_on_clip_b_bridges_the_window_that_straddles_the_cut(oracle):
    corr, nlag = MC.rows(oracle, "spliced", "B")
    m = pr.map_model(corr, nlag, PC.KEY, span=MC.SPAN)
    _show("B", m)
    assert [p.detected for p in m.windows] == [True, True, True, False, True, True, True, True, True]
    assert [(s.first, s.last, s.confirmed, s.t) for s in m.stretches] == [(0, 2, True, MC.T0), (4, 8, True, MC.T0 - MC.CUT_LEN)]
    assert m.splices == [pr.Splice(40 * FL, 120 * FL, MC.CUT_LEN)] and m.marked == 186 * FL


def test_an_unmarked_host_has_no_confirmed_stretch(oracle):
    corr, nlag = MC.rows(oracle, "unmarked", "A")
    m = pr.map_model(corr, nlag, PC.KEY, span=MC.SPAN)
    _show("A's host", m)
    assert len(m.windows) == 9 and not any(s.confirmed for s in m.stretches) and m.marked == 0 and m.splices == []
    for w, (s, col, n) in enumerate(pr.map_windows(nlag)):                  # exactly the windows' own verdicts
        p = pr.presence_model(corr[:, col:col + n], n, PC.KEY, span=(MC.SPAN[0] + s, MC.SPAN[1] + s))
        q = m.windows[w]
        assert (p.detected, p.ctr, p.phase, p.phases) == (q.detected, q.ctr, q.phase, q.phases) and _bits([p.score, *p.null]).tolist() == _bits([q.score, *q.null]).tolist()
    assert [(s.first, s.last) for s in m.stretches] == [(w, w) for w, p in enumerate(m.windows) if p.detected]


def test_map_model_follows_the_drifted_clip(oracle):
    corr, nlag = MC.rows(oracle, "drifted", "A")
    m = pr.map_model(corr, nlag, PC.KEY, span=MC.SPAN, drift_ppm=300)
    _show("A drifted", m)
    sure = [s for s in m.stretches if s.confirmed]
    assert len(sure) == 2 and len(m.splices) == 1 and abs(m.splices[0].removed - MC.CUT_LEN) <= 8
    assert sure[0].first == 0 and sure[1].last == len(m.windows) - 1 and m.windows[0].hypotheses is not None
    assert [pr.anchor(p, FL * s) for p, s in zip(m.windows[:3], m.starts)] != [MC.T0] * 3      # the anchors walk: the tolerance is in use


def test_a_clip_of_at_most_one_window_is_the_presence_call(oracle):
    corr, nlag = MC.rows(oracle, "spliced", "A")
    for n in (40 * FL, 12 * FL + 100):
        m = pr.map_model(corr[:, :n], n, PC.KEY, span=PC.SPAN)
        p, q = pr.presence_model(corr[:, :n], n, PC.KEY, span=PC.SPAN), m.windows[0]
        assert m.starts == [0] and len(m.windows) == 1
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases, p.skew, p.drift_ppm, p.hypotheses) == \
               (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases, q.skew, q.drift_ppm, q.hypotheses)
        assert _bits([p.score, *p.null]).tolist() == _bits([q.score, *q.null]).tolist() and q.detected
        assert [(s.first, s.last, s.confirmed) for s in m.stretches] == [(0, 0, False)] and m.marked == 0
        assert pr.map_model(corr[:, :n], n, PC.KEY, span=PC.SPAN, confirm=1).marked == FL * (n // FL)
    assert pr.map_model(corr[:, :1214], 1214, PC.KEY) is None
