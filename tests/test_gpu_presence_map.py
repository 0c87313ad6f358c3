"""GPU: the presence timeline -- es_fold_pick_batch exactly (ints equal, values as uint64 views) against its host twin
presence.pick_model on folds that hold every edge of its definition, without val_dev, every refusal with its outputs unwritten, the empty
calls, two runs, capture and replay; the device pick inside presence_search.search against the host's pick, field for field, with the default
route's call sequence unchanged; and presence_map / presence_map_batch of detector and identifier against presence.map_model on the
downloaded rows, against each other, and launch by launch."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import echoseal_amd._native as nat
import presence_cases as PC
import presence_map_cases as MC
from echoseal_amd import presence as pr
from echoseal_amd import presence_search as ps
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

FL = 1215
POISON_I, POISON_F = -77, -777.25
KEYS3 = [PC.OTHER_KEY, PC.KEY, bytes(range(64, 96))]


def _dev(engine, a):
    return torch.from_numpy(np.array(a, order="C")).to(engine.device)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _equals_model(engine, fold, nwarp, H):
    hyp, val = engine.fold_pick(_dev(engine, fold), nwarp, H)
    want_hyp, want_val = pr.pick_model(fold, nwarp, H)
    hyp, val = hyp.cpu().numpy(), val.cpu().numpy()
    assert hyp.dtype == np.int32 and val.dtype == np.float64 and hyp.shape == want_hyp.shape and val.shape == want_val.shape
    assert np.array_equal(hyp, want_hyp), (hyp, want_hyp)
    assert np.array_equal(_bits(val), _bits(want_val)), (val, want_val)
    return hyp, val


# ---------------------------------------------------------------------------------------------------------------- the pick against its twin
@pytest.mark.parametrize("H", [1, 8, 9, 64])
@pytest.mark.parametrize("name", list(MC.edge_folds()))
def test_fold_pick_equals_the_twin(engine, name, H):
    fold, nwarp = MC.edge_folds()[name]
    hyp, val = _equals_model(engine, fold, nwarp, H)
    if name == "nothing-to-pick":
        assert (hyp[:] == -1).all() and np.isneginf(val).all()              # every row -inf, one row of them, nwarp = 0
    if name == "nan-inside-a-row":
        assert not np.isnan(val).any() and (hyp[2, 1:] == -1).all() and tuple(hyp[2, 0]) == (1, 0)
    if name == "winner-at-the-last-element":
        assert tuple(hyp[0, 0]) == (4, 1214) and tuple(hyp[1, 0]) == (0, 0) and (H == 1 or tuple(hyp[1, 1]) == (4, 1214))
    if name == "zeros-of-both-signs" and H >= 8:
        assert [tuple(e) for e in hyp[0, :3]] == [(0, 9), (1, 2), (1, 5)] and _bits(val[0, :3]).tolist() == _bits([0.0, -0.0, -0.0]).tolist()


def test_fold_pick_takes_a_phase_fold_and_more_than_one_wave_of_rows(engine):
    rng = np.random.default_rng(28)
    flat = rng.standard_normal((5, FL)).round(2)
    hyp, _ = engine.fold_pick(_dev(engine, flat), None, 8)
    assert np.array_equal(hyp.cpu().numpy(), pr.pick_model(flat[:, None, :], None, 8)[0])
    assert [p for _, p in hyp[0].cpu().numpy().tolist()] == pr.pick_phases(flat[0], 8)
    big = rng.standard_normal((2, 59, FL)).round(3)                         # the table of +-300 ppm over a one-second window
    _equals_model(engine, big, [59, 31], 8)


def test_fold_pick_without_values(engine):
    fold, nwarp = MC.edge_folds()["nan-past-nwarp"]
    hyp, val = engine.fold_pick(_dev(engine, fold), nwarp, 9, want_val=False)
    assert val is None and np.array_equal(hyp.cpu().numpy(), pr.pick_model(fold, nwarp, 9)[0])


def _pick_inputs(engine):
    fold = np.random.default_rng(29).standard_normal((3, 2, FL)).round(2)
    return dict(fold=_dev(engine, fold), B=3, D=2, nwarp=_dev(engine, np.array([2, 1, 2], np.int32)), H=8,
                hyp=torch.empty((3, 8, 2), dtype=torch.int32, device=engine.device), val=torch.empty((3, 8), dtype=torch.float64, device=engine.device)), fold


ORDER = ("fold", "B", "D", "nwarp", "H", "hyp", "val")


def _raw(engine, args, **over):
    a = dict(args)
    a.update(over)
    p = lambda v: v.data_ptr() if torch.is_tensor(v) else v                 # noqa: E731
    rc = engine._lib.es_fold_pick_batch(engine._ctx, *[p(a[k]) for k in ORDER], engine._stream())
    torch.cuda.synchronize()
    return rc


REFUSALS = [dict(fold=None), dict(hyp=None), dict(B=-1), dict(D=-1), dict(H=0), dict(H=-1), dict(H=65), dict(H=1 << 40), dict(B=1 << 31),
            dict(D=(((1 << 31) - 1) // FL) + 1), dict(B=-1, D=0), dict(H=0, B=0)]


@pytest.mark.parametrize("over", REFUSALS, ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_refusals_write_nothing(engine, over):
    args, _ = _pick_inputs(engine)
    args["hyp"].fill_(POISON_I); args["val"].fill_(POISON_F)
    assert _raw(engine, args, **over) == nat.ES_EINVAL
    assert (args["hyp"] == POISON_I).all() and (args["val"] == POISON_F).all()
    assert engine._lib.es_last_error(engine._ctx).decode().startswith("es_fold_pick_batch")


def test_the_accepted_call_and_the_empty_ones(engine):
    """B * D == 0 enqueues nothing and writes nothing, D == 0 with records included (the header's decision); the wrapper fills the lists
    of such a call itself.  A null nwarp is D rows for every record, a null val is allowed."""
    args, fold = _pick_inputs(engine)
    args["hyp"].fill_(POISON_I); args["val"].fill_(POISON_F)
    assert _raw(engine, args, B=0) == 0 and _raw(engine, args, D=0) == 0 and _raw(engine, args, B=0, D=0, fold=None, hyp=None) == 0
    assert (args["hyp"] == POISON_I).all() and (args["val"] == POISON_F).all()
    assert _raw(engine, args, val=None) == 0
    want_hyp, want_val = pr.pick_model(fold, [2, 1, 2], 8)
    assert np.array_equal(args["hyp"].cpu().numpy(), want_hyp) and (args["val"] == POISON_F).all()
    assert _raw(engine, args) == 0 and np.array_equal(_bits(args["val"].cpu().numpy()), _bits(want_val))
    assert _raw(engine, args, nwarp=None) == 0 and np.array_equal(args["hyp"].cpu().numpy(), pr.pick_model(fold, None, 8)[0])
    for shape in ((0, 2, FL), (3, 0, FL)):
        hyp, val = engine.fold_pick(torch.empty(shape, dtype=torch.float64, device=engine.device), None, 4)
        assert tuple(hyp.shape) == (shape[0], 4, 2) and bool((hyp == -1).all()) and tuple(val.shape) == (shape[0], 4) and bool(torch.isinf(val).all())
    for bad in (dict(H=0), dict(H=65), dict(nwarp=[1, 2])):
        with pytest.raises(ValueError):
            engine.fold_pick(args["fold"], bad.get("nwarp"), bad.get("H", 8))
    with pytest.raises(ValueError):
        engine.fold_pick(args["fold"][:, :, :1214].contiguous())


def test_two_runs_give_the_same_bits(engine):
    args, _ = _pick_inputs(engine)
    a, b = engine.fold_pick(args["fold"], args["nwarp"], 64), engine.fold_pick(args["fold"], args["nwarp"], 64)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b)) and bool((a[0] >= 0).all())


def test_the_pick_records_into_a_graph(engine):
    args, fold = _pick_inputs(engine)
    want = engine.fold_pick(args["fold"], args["nwarp"], 9)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = engine.fold_pick(args["fold"], args["nwarp"], 9)
    torch.cuda.synchronize()
    for t in got:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and np.array_equal(got[0].cpu().numpy(), pr.pick_model(fold, [2, 1, 2], 9)[0])


# ---------------------------------------------------------------------------------------------------------------- inside the search
def _corr(engine, clip):
    """The four correlation rows of a clip at 48 kHz as the detector's front makes them -> (corr float64 [4, n] on the device, nlag)."""
    x = _dev(engine, np.tile(np.asarray(clip, np.float32), (4, 1)))
    bid = _dev(engine, np.arange(4, dtype=np.uint8))
    return engine.xcorr(engine.bpf(x, bid), bid), clip.size - 62


@pytest.fixture(scope="module")
def records(engine):
    """The spliced clip A's rows and its nine windows as records of the _at calls, each with its own span; under +-300 ppm too."""
    corr, nlag = _corr(engine, MC.clip("spliced"))
    wins = pr.map_windows(nlag)
    at = (np.array([[0, 1, 2, 3]] * len(wins), np.int64), np.array([c for _, c, _ in wins], np.int64))
    spans = [pr.window_span(MC.SPAN, s, n // FL) for s, _, n in wins]
    ring = engine.keyring(KEYS3 + pr.decoy_keys(8))
    return corr, [n for _, _, n in wins], at, spans, ring


def _same(p, q):
    assert (p is None) == (q is None)
    if p is not None:
        assert (p.detected, p.ctr, p.phase, p.ctr0, p.frames, p.phases, p.skew, p.drift_ppm, p.hypotheses) == \
               (q.detected, q.ctr, q.phase, q.ctr0, q.frames, q.phases, q.skew, q.drift_ppm, q.hypotheses)
        assert _bits([p.score]).tolist() == _bits([q.score]).tolist() and np.array_equal(_bits(p.null), _bits(q.null))


def _same_map(m, q):
    assert (m is None) == (q is None)
    if m is not None:
        assert len(m.windows) == len(q.windows) and m.starts == q.starts and m.stretches == q.stretches and m.splices == q.splices and m.marked == q.marked
        for a, b in zip(m.windows, q.windows):
            _same(a, b)


@pytest.mark.parametrize("drift", [0.0, 300.0])
def test_fold_pick_on_real_folds_is_pick_hypotheses(engine, records, drift):
    corr, nlags, at, _, _ = records
    tabs = [pr.skew_table(n, drift) for n in nlags] if drift else None
    D, J = (len(tabs[0][0]), tabs[0][1]) if drift else (1, nlags[0] // FL)
    warp = np.stack([t[2] for t in tabs]) if drift else np.zeros((len(nlags), 1, J), np.int32)
    fold = engine.warp_fold_at(corr, at[0], at[1], nlags, warp, [D] * len(nlags), [J] * len(nlags))
    hyp, val = engine.fold_pick(fold, [D] * len(nlags), 8)
    host = fold.cpu().numpy()
    for b in range(len(nlags)):
        want = pr.pick_hypotheses(host[b], 8)
        assert [tuple(e) for e in hyp[b].cpu().numpy().tolist()] == want
        assert _bits(val[b].cpu().numpy()).tolist() == _bits([host[b][e] for e in want]).tolist()


@pytest.mark.parametrize("drift", [0.0, 300.0])
def test_the_search_with_the_device_pick_is_the_search_without(engine, records, drift):
    corr, nlags, at, spans, ring = records
    calls, real = [], engine._call
    engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        host = ps.search(engine, ring, 3, corr, nlags, spans, drift, 8, at=at, pos0=at[1])
        mark = len(calls)
        device = ps.search(engine, ring, 3, corr, nlags, spans, drift, 8, at=at, pos0=at[1], device_pick=True)
    finally:
        del engine._call
    assert calls[:mark] == ["es_warp_fold_at_batch", "es_hop_window_batch", "es_warp_score_at_batch"]       # the default route: as it was
    assert calls[mark:] == ["es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch"]
    assert len(host) == len(device) == len(nlags)
    for h, d in zip(host, device):
        assert len(h) == len(d) == 3
        for p, q in zip(h, d):
            _same(p, q)
    assert all(r[1].detected for r in device)
    with pytest.raises(ValueError):
        ps.search(engine, ring, 3, corr[:, :nlags[0]].contiguous(), nlags[:1], spans[:1], drift, 8, device_pick=True)      # the at= route only
    with pytest.raises(ValueError):
        ps.search(engine, ring, 3, corr, nlags, spans, drift, 65, at=at, device_pick=True)


# ---------------------------------------------------------------------------------------------------------------- the public calls
def _twin(det, key, kind_rows, **kw):
    """map_model on the rows the detector's last call downloaded for its twin."""
    (ids, corr, nlag), = kind_rows
    return [pr.map_model(corr[4 * k:4 * k + 4], int(nlag[k]), key, **kw) for k in range(len(ids))]


def test_presence_map_of_the_spliced_clip_is_the_twin_on_its_rows(engine):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    m = det.presence_map(MC.clip("spliced"), 48_000, span=MC.SPAN)
    want, = _twin(det, PC.KEY, det._presence_rows, span=MC.SPAN)
    _same_map(m, want)
    for w, p in enumerate(m.windows):
        print(f"window {w}: detected {p.detected}, own {p.score:.4f}, decoy max {p.null.max():.4f}, ctr {p.ctr}, phase {p.phase}")
    assert m.starts == [0, 20, 40, 60, 80, 100, 120, 140, 146] and all(p.detected for p in m.windows)
    assert [(s.first, s.last, s.confirmed, s.t, s.ctr0) for s in m.stretches] == [(0, 2, True, MC.T0, 1), (3, 8, True, MC.T0 - MC.CUT_LEN, 11)]
    assert m.splices == [pr.Splice(40 * FL, 100 * FL, MC.CUT_LEN)] and m.marked == 186 * FL
    det._presence_rows = []
    short = det.presence_map(MC.clip("spliced"), 48_000, ctr0=1)             # span (1, 3) follows no cut: the mark is lost behind it; the window
                                                                            # that straddles the cut still holds 19 slots of the first grid
    _same_map(short, _twin(det, PC.KEY, det._presence_rows, span=(1, 3))[0])
    assert [(s.first, s.last) for s in short.stretches if s.confirmed] == [(0, 3)] and short.splices == []


def test_presence_map_batch_is_the_single_calls(engine):
    from scipy.signal import resample_poly
    b = PC.cached("marked", "B")
    clips = [MC.clip("spliced"), (resample_poly(b.astype(np.float64), 147, 160) * 32768).astype(np.int16), MC.clip("spliced")[:30_000],
             MC.clip("spliced")[:1200]]
    rates = [48_000, 44_100, 48_000, 48_000]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    got = det.presence_map_batch(clips, rates, span=MC.SPAN)
    assert len(got) == 4 and got[3] is None
    for c in range(4):
        _same_map(got[c], det.presence_map(clips[c], rates[c], span=MC.SPAN))
    assert len(got[0].splices) == 1 and got[0].splices[0].removed == MC.CUT_LEN
    assert len(got[1].windows) == 3 and [(s.first, s.last, s.confirmed) for s in got[1].stretches] == [(0, 2, True)] and got[1].splices == []
    assert got[1].marked == FL * ((b.size - 62) // FL) and got[1].stretches[0].t == MC.T0
    assert len(got[2].windows) == 1 and got[2].starts == [0]                # J <= W: the presence call on the clip, field for field
    _same(got[2].windows[0], det.presence(clips[2], 48_000, span=MC.SPAN))
    mixed = det.presence_map_batch(clips[:2], rates[:2], [1, None], span=MC.SPAN, window=30, step=7, confirm=3, phases=4, decoys=7)
    _same_map(mixed[0], det.presence_map(clips[0], 48_000, 1, window=30, step=7, confirm=3, phases=4, decoys=7))
    _same_map(mixed[1], det.presence_map(clips[1], 44_100, span=MC.SPAN, window=30, step=7, confirm=3, phases=4, decoys=7))


def test_one_fold_one_pick_and_one_hop_window_per_group(engine, monkeypatch):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    whole = det.presence_map(MC.clip("spliced"), 48_000, span=MC.SPAN)

    def count(limit):
        if limit is not None:
            monkeypatch.setattr(ps, "MAP_HOP_BYTES", limit)
        calls, real = [], engine._call
        engine._call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            m = det.presence_map(MC.clip("spliced"), 48_000, span=MC.SPAN)
        finally:
            del engine._call
        _same_map(m, whole)
        return [n for n in calls if n in ("es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch")], calls

    assert ps.MAP_HOP_BYTES == 256 << 20
    back, calls = count(None)
    assert back == ["es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch"]        # nine windows, one group
    assert not any("phase_fold" in n or n in ("es_warp_fold_batch", "es_hop_score_batch", "es_warp_score_batch") for n in calls)
    K, ccols = 33, MC.SPAN[1] - MC.SPAN[0] + 40 - 1
    back, _ = count(K * 4 * ccols)                                          # four hop rows fit: groups of 4, 4 and 1 windows
    assert back == ["es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch"] * 3
    back, _ = count(1)                                                      # a group holds at least one window
    assert back == ["es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch"] * 9


def test_identifier_entry_k_is_the_detector_of_key_k(engine):
    clips = [MC.clip("spliced"), MC.clip("spliced")[:30_000], MC.clip("spliced")[:1000]]
    ident = WatermarkIdentifier(KEYS3, list_size=8, engine=engine)
    got = ident.presence_map_batch(clips, 48_000, span=MC.SPAN)
    assert got[2] is None and all(len(g) == 3 for g in got[:2])
    for k, key in enumerate(KEYS3):
        want = WatermarkDetector(key, list_size=8, engine=engine).presence_map_batch(clips, 48_000, span=MC.SPAN)
        for c in range(2):
            _same_map(got[c][k], want[c])
    assert got[0][1].marked == 186 * FL and got[0][0].marked == 0 and got[0][2].marked == 0
    one = ident.presence_map(clips[0], 48_000, span=MC.SPAN)
    for k in range(3):
        _same_map(one[k], got[0][k])


def test_presence_map_follows_drift_like_the_twin(engine):
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    det._presence_rows = []
    m = det.presence_map(MC.clip("drifted"), 48_000, span=MC.SPAN, drift_ppm=300)
    _same_map(m, _twin(det, PC.KEY, det._presence_rows, span=MC.SPAN, drift_ppm=300)[0])
    sure = [s for s in m.stretches if s.confirmed]
    assert len(sure) == 2 and len(m.splices) == 1 and abs(m.splices[0].removed - MC.CUT_LEN) <= 8
    assert m.windows[0].hypotheses is not None and len(m.windows[0].hypotheses) == 8
