"""GPU: the launches and results of every public presence call, pinned to tests/golden/presence_trace.json.  Per call
the ordered C-ABI entry points the engine was asked for -- with each name the dtype and shape of every tensor argument, the value of every
integer scalar and null for None -- and every field of every Presence, PresenceMap, Stretch and Splice that came back, floats as their
64-bit patterns.  The file was recorded before the presence code was split into presence.py (what needs no GPU) and presence_search.py (the
launches), so the split is held to the launches and bits of before.  ECHOSEAL_WRITE_PRESENCE_TRACE=1 writes the file; without it the test
only compares.  The shapes are the smallest that reach every arm: clips of about 12 slots, windows of 5 slots every 3, spans 4 wide."""
import dataclasses
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import presence_cases as PC
import presence_map_cases as MC
from echoseal_amd import presence as pr
from echoseal_amd import presence_search as ps
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

FL, SEG = 1215, 1216
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "presence_trace.json")
WRITE = "ECHOSEAL_WRITE_PRESENCE_TRACE"
SLOTS = 12
N = SLOTS * FL + 100                                                        # a clip of 12 slots: 14680 samples
GRID = dict(window=5, step=3, confirm=2, phases=4, decoys=3)
COH_GRID = dict(window=5, step=3, confirm=2, decoys=3)
SPAN = (0, 4)                                                               # clip A's first whole frame carries counter 1
KEYS2 = [PC.OTHER_KEY, PC.KEY]
WINDOW = 8 * SEG                                                            # the live monitors' window: seven slots


def _f64(v) -> str:
    return "f64:%016x" % int(np.float64(v).view(np.uint64))


def _arg(a):
    """An argument of a C-ABI call as the golden file holds it."""
    if a is None:
        return None
    if type(a) is torch.Tensor:
        return f"{str(a.dtype).replace('torch.', '')}{list(a.shape)}"
    if isinstance(a, (bool, int, np.integer)):
        return int(a)
    if isinstance(a, (float, np.floating)):
        return _f64(a)
    return type(a).__name__


def _value(v):
    """A result as the golden file holds it: dataclasses by field, floats as their 64-bit patterns, a long identity list by its length."""
    if dataclasses.is_dataclass(v):
        return {"type": type(v).__name__, **{f.name: _value(getattr(v, f.name)) for f in dataclasses.fields(v)}}
    if isinstance(v, np.ndarray):
        return [_value(x) for x in v.tolist()]
    if isinstance(v, (list, tuple)):
        if len(v) > 64 and list(v) == list(range(len(v))):
            return {"range": len(v)}
        return [_value(x) for x in v]
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return _f64(v)
    assert v is None, type(v)
    return None


def _traced(engine, call):
    """call() with the engine's one C-ABI door recorded -> {"calls": [[name, arguments]], "result": ...}."""
    calls, real = [], engine._call
    engine._call = lambda name, *a: (calls.append([name, [_arg(x) for x in a]]), real(name, *a))[1]
    try:
        res = call()
    finally:
        del engine._call
    return {"calls": calls, "result": _value(res)}


def _splice12():
    """Twelve slots of clip A with MC.CUT_LEN samples (ten frames and 500 samples) removed from the middle: the first whole frame carries
    counter 1, and the grid anchor moves by CUT_LEN at the cut."""
    a = PC.cached("marked", "A")
    return np.ascontiguousarray(np.concatenate([a[:N // 2], a[N // 2 + MC.CUT_LEN:N + MC.CUT_LEN]]))


def _record(engine, monkeypatch) -> dict:
    from scipy.signal import resample_poly
    a, u, sp = PC.cached("marked", "A"), PC.cached("unmarked", "A"), _splice12()
    low = (resample_poly(a[:12_000].astype(np.float64), 147, 160) * 32768).astype(np.int16)
    ragged, rates = [a[:N], low, a[:1000]], [48_000, 44_100, 48_000]
    top = (2 ** 32 - 10, 2 ** 32 - 6)                                       # windows at slots 0, 3, 6, 7: widths 4, 3 and two empty spans
    assert sorted({hi - lo for lo, hi in (pr.window_span(top, s, 5) for s in (0, 3, 6, 7))}) == [0, 3, 4]
    det = WatermarkDetector(PC.KEY, list_size=8, engine=engine)
    ident = WatermarkIdentifier(KEYS2, list_size=8, engine=engine)
    nobody = WatermarkIdentifier([], list_size=8, engine=engine)
    out = {}

    def run(name, call):
        assert name not in out
        out[name] = _traced(engine, call)

    run("batch-equal", lambda: det.presence_batch([a[:N], u[:N]], 48_000, span=SPAN, phases=4, decoys=3))
    run("batch-ragged-drift", lambda: det.presence_batch(ragged, rates, [1, None, None], span=SPAN, phases=4, decoys=3, drift_ppm=300))
    run("batch-ragged-drift-one-span", lambda: det.presence_batch([a[:N], a[:N - 300], a[:1000]], 48_000, span=SPAN, phases=4, decoys=3, drift_ppm=300))
    run("batch-ragged-rigid", lambda: det.presence_batch(ragged, rates, span=SPAN, phases=4, decoys=3))
    run("map", lambda: det.presence_map(sp, 48_000, span=SPAN, **GRID))
    run("map-drift", lambda: det.presence_map(sp, 48_000, span=SPAN, drift_ppm=300, **GRID))
    run("map-top", lambda: det.presence_map(sp, 48_000, span=top, **GRID))
    run("map-batch-ragged", lambda: det.presence_map_batch(ragged, rates, [1, None, None], span=SPAN, **GRID))
    run("coherent-1215", lambda: det.presence_coherent(a[:N], 48_000, span=SPAN, decoys=3))
    run("coherent-cheap", lambda: det.presence_coherent(a[:N], 48_000, span=SPAN, phases=4, decoys=3))
    run("coherent-batch-ragged", lambda: det.presence_coherent_batch(ragged, rates, [1, None, None], span=SPAN, phases=4, decoys=3))
    run("coherent-map", lambda: det.presence_coherent_map(sp, 48_000, span=SPAN, **COH_GRID))
    run("coherent-map-top", lambda: det.presence_coherent_map(sp, 48_000, span=top, **COH_GRID))
    run("identifier-batch", lambda: ident.presence_batch(ragged, rates, [1, None, None], span=SPAN, phases=4, decoys=3, drift_ppm=300))
    run("identifier-coherent-map-batch", lambda: ident.presence_coherent_map_batch([sp, a[:N - 300], a[:1000]], 48_000, span=SPAN, **COH_GRID))
    run("nobody-batch", lambda: nobody.presence_batch([a[:N], a[:N - 300]], 48_000, span=SPAN, phases=4, decoys=3))
    run("nobody-coherent-map-batch", lambda: nobody.presence_coherent_map_batch([sp], 48_000, span=SPAN, **COH_GRID))

    def live(owner, **kw):
        mon = owner.open_streams(3, window_s=WINDOW / 48_000, chunk_max=4000, ctr0=[1, None, None], **kw)
        for lo, hi in ((0, 4000), (4000, 8000), (8000, 12_000)):            # the third push slides the window: w0 = 2 * 1216
            mon.push([a[lo:hi], a[lo:hi]], [0, 1])
        assert mon.table.n_host[:2].tolist() == [12_000, 12_000] and mon.table.n_host[2] == 0
        return mon

    mon, lid = live(det), live(ident, memo_slots=0)
    run("monitor", lambda: mon.presence(span=(0, 8), phases=4, decoys=3))
    run("monitor-drift", lambda: mon.presence([1, 0], span=(0, 8), phases=4, decoys=3, drift_ppm=300))
    run("live-identifier", lambda: lid.presence(span=(0, 8), phases=4, decoys=3))
    with monkeypatch.context() as m:                                        # a hop table of two hop rows per group: the four windows in two groups
        m.setattr(ps, "MAP_HOP_BYTES", 4 * 2 * (4 + 5 - 1))
        run("map-two-groups", lambda: det.presence_map(sp, 48_000, span=SPAN, **GRID))
        run("coherent-map-two-groups", lambda: det.presence_coherent_map(sp, 48_000, span=SPAN, **COH_GRID))
    return out


def _names(case):
    return [c[0] for c in case["calls"]]


def test_every_public_presence_call_launches_and_returns_what_it_did(engine, monkeypatch):
    got = json.loads(json.dumps(_record(engine, monkeypatch)))
    # what the shapes were chosen to reach, whatever the file says
    assert "es_phase_fold_batch" in _names(got["batch-equal"]) and "es_hop_score_batch" in _names(got["batch-equal"])
    assert "es_bpf_batch" in _names(got["batch-equal"]) and "es_sync_ragged_batch" not in _names(got["batch-equal"])
    assert "es_sync_ragged_batch" in _names(got["batch-ragged-rigid"])       # the two float32 clips; the int16 clip is a launch of its own
    drift = _names(got["batch-ragged-drift"])
    assert drift.count("es_warp_fold_batch") == 2 and drift.count("es_warp_score_batch") == 2           # two span groups
    assert got["batch-ragged-drift"]["result"][2] is None
    one = _names(got["batch-ragged-drift-one-span"])                        # unequal lengths under one span: sync_ragged, then the warp route
    assert one == ["es_sync_ragged_batch", "es_warp_fold_batch", "es_hop_window_batch", "es_warp_score_batch"]
    group = ("es_warp_fold_at_batch", "es_fold_pick_batch", "es_hop_window_batch", "es_warp_score_at_batch")
    assert [n for n in _names(got["map"]) if n in group] == list(group)
    assert [n for n in _names(got["map-two-groups"]) if n in group] == list(group) * 2
    assert [n for n in _names(got["map-top"]) if n in group] == list(group) + ["es_warp_score_at_batch"] * 2      # widths 0, 3 and 4
    assert _names(got["coherent-map-two-groups"]).count("es_hop_window_batch") >= 2
    assert "es_xcorr_batch" in _names(got["coherent-cheap"]) and "es_xcorr_batch" not in _names(got["coherent-1215"])
    assert got["nobody-batch"]["result"] == [None, None] and got["nobody-coherent-map-batch"]["result"] == [None]
    assert got["monitor"]["result"][2] is None and got["monitor"]["result"][0]["type"] == "Presence"
    if os.environ.get(WRITE):
        with open(GOLDEN, "w") as f:
            json.dump(got, f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for name in want:
        assert _names(got[name]) == _names(want[name]), name
        assert got[name]["calls"] == want[name]["calls"], name
        assert got[name]["result"] == want[name]["result"], name
