"""GPU: the engine calls of the detector and the identifier after the sync, in order.

A wrapper around the engine (here only, not in the library) records, for the methods the back end uses, the name of every call, the shapes
of its tensor arguments and what it returned.  What must have been called is worked out from what the planners gave -- the counts
es_plan_batch wrote (seen coming back from `plan`), the plans of WatermarkDetector._scan_plan, the counters of _acquire_plan, the answers
of the memo -- and from the cap on the candidates of one decode, which every case replaces on the instance by a value smaller than the
candidates at hand and not dividing them: every decode then has several chunks and a partial last one.  Per chunk of n candidates there
is one schedule call, two demodulations, one list decode of 4 n rows and one selection, in that order, and nothing else in between."""
from dataclasses import dataclass

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import NB, WatermarkIdentifier
from echoseal_amd.scan import cut_launches

from test_gpu_scan_launches import KEYS, _queue

RECORDED = ("header", "plan", "hop_window", "schedule", "schedule_keyed", "llr", "scl", "select", "aead_check_keyed", "memo_probe", "memo_insert",
            "acquire_mask", "acquire_list")
LIST, CAP = 2, 3
W8, CM8 = 3648, 1300                                                        # the smallest geometry of test_gpu_live_identify.py
FILL = (1300, 1046)                                                         # n = 2 346: one more chunk_max and the window is full, still from 0


@dataclass
class _Call:
    name: str
    shapes: list         # of the tensor and array arguments, positional then keyword
    flags: dict          # bool / int keyword arguments
    out: object


class _Recording:
    """An engine's attributes handed through; the calls of the back end's methods recorded in order."""

    def __init__(self, eng) -> None:
        self._eng, self.calls = eng, []

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if name not in RECORDED:
            return attr

        def recorded(*a, **k):
            out = attr(*a, **k)
            shapes = [tuple(v.shape) for v in list(a) + list(k.values()) if torch.is_tensor(v) or isinstance(v, np.ndarray)]
            self.calls.append(_Call(name, shapes, {n: v for n, v in k.items() if isinstance(v, (bool, int))}, out))
            return out
        return recorded


def _chunk(calls, at: int, n: int, keyed: bool) -> int:
    """calls[at : at + 5] is the decode of one chunk of n candidates -> at + 5."""
    names = [c.name for c in calls[at:at + 5]]
    assert names == ["schedule_keyed" if keyed else "schedule", "llr", "llr", "scl", "select"], (at, names)
    sched, l0, l1, scl, sel = calls[at:at + 5]
    assert sched.shapes == [(n,)] * (2 if keyed else 1) and sched.flags.get("want_pn", True), (at, sched)
    for v, ll in enumerate((l0, l1)):
        assert ll.flags == {"variant": v} and ll.shapes[1:] == [(n,), (n, 152), (n,), (n,)], (at, ll.shapes, ll.flags)
    assert scl.shapes == [(4 * n, 1024)] and scl.flags == {"list_size": LIST, "skip_if_hard_ok": False}, (at, scl.shapes, scl.flags)
    assert sel.shapes == [(4 * n,)] * (2 if keyed else 1), (at, sel.shapes)
    return at + 5


def _chunks(calls, at: int, total: int, keyed: bool, upto: int | None = None, cap: int = CAP) -> int:
    """ceil(total / cap) chunks from calls[at] on, the last one partial (upto: the walk stopped at that candidate)."""
    for k in range(0, total if upto is None else upto, cap):
        at = _chunk(calls, at, min(cap, total - k), keyed)
    return at


def _cap_below(sizes: list) -> int:
    """One less than the longest plan: that plan is decoded in two chunks, a full one and a partial one of one candidate."""
    return max(2, max(sizes) - 1)


def _detector(eng):
    """A detector on the recording engine and the sizes of the plans its _scan_plan gives, in call order.  Its cap is replaced by
    _cap_below those sizes, asked for when the walk begins: a (clip, band) holds only a handful of candidates."""
    det = WatermarkDetector(KEYS[0], list_size=LIST, engine=eng)
    sizes, real = [], det._scan_plan
    det._pair_cap = lambda: _cap_below(sizes) if sizes else CAP

    def scan_plan(scan, bi):
        out = real(scan, bi)
        sizes.append(len(out[0]))
        return out
    det._scan_plan = scan_plan
    return det, sizes


def _detector_batches(m: np.ndarray, groups: list, cap: int) -> list:
    """The candidates of each decode of a walk in which nothing is accepted (WatermarkDetector._verify_scans), from the plan sizes m[clip, band]: when the
    walk reaches a (clip, band) with candidates that is not decoded yet, that one and -- in walk order, the clip's further bands, then the
    later clips of its launch -- as many further ones as fit under the cap go through one decode."""
    group_of = {i: sorted(g) for g in groups for i in g}
    done, out = set(), []
    for i in range(m.shape[0]):
        for bi in range(NB):
            if not m[i, bi] or (i, bi) in done:
                continue
            todo = [(i, r) for r in range(bi, NB)] + [(j, r) for j in group_of[i] if j > i for r in range(NB)]
            batch, n = [], 0
            for jr in todo:
                if jr in done:
                    continue
                if batch and n + m[jr] > cap:
                    break
                batch.append(jr); n += int(m[jr])
            done.update(batch)
            out.append(n)
    return out


def _check_detector(calls, at: int, sizes: list, groups: list) -> None:
    m = np.array(sizes, np.int64).reshape(-1, NB)
    assert m.shape[0] == sum(len(g) for g in groups)
    cap = _cap_below(sizes)
    batches = _detector_batches(m, groups, cap)
    assert sum(batches) == m.sum() and m.max() > cap                        # everything planned is decoded once; the cap does cut
    assert any(n > cap and n % cap for n in batches)                        # ... some decode into several chunks and a partial last one
    for n in batches:
        at = _chunks(calls, at, n, keyed=False, cap=cap)
    assert at == len(calls), [c.name for c in calls[at:at + 8]]


@pytest.mark.parametrize("origin", [None, 5000], ids=["relative", "one-origin"])
def test_verify_batch_decodes_in_capped_chunks(engine, origin):
    clips, rates = _queue()
    eng = _Recording(engine)
    det, sizes = _detector(eng)
    launches = cut_launches(clips, rates, 48_000, NB, det._conditioned)
    ctr0 = None if origin is None else [None, origin, None, None, None]
    assert det.verify_batch(clips, rates, ctr0) == [False] * 5
    assert [c.name for c in eng.calls[:len(launches)]] == ["header"] * len(launches)       # one header decode per launch, all before the walk
    _check_detector(eng.calls, len(launches), sizes, [la.idx for la in launches])


def _orders(engine):
    """[N, 4] band index of each key's rank r: its band of counter 0 first (rtwm/detector.py:46-52)."""
    hop0 = engine.keyring(KEYS).hop0.cpu().numpy().astype(np.int64)
    return np.array([[h] + [b for b in range(NB) if b != h] for h in hop0], np.int64)


def _rank_totals(plan_call, order: np.ndarray, clips: int) -> list:
    """The candidates of each band rank when no key matches, from the counts the plan call returned."""
    count = plan_call.out.count.cpu().numpy().astype(np.int64).reshape(len(KEYS), clips * NB)
    rows = np.arange(clips)[None, :] * NB
    return [int(count[np.arange(len(KEYS))[:, None], rows + order[:, r][:, None]].sum()) for r in range(NB)]


@pytest.mark.parametrize("origin", [None, 5000], ids=["relative", "one-origin"])
def test_identify_batch_decodes_rank_by_rank_in_capped_chunks(engine, origin):
    clips, rates = _queue()
    eng = _Recording(engine)
    ident = WatermarkIdentifier(KEYS, list_size=LIST, engine=eng)
    ident._pair_cap = lambda: CAP
    launches = cut_launches(clips, rates, 48_000, NB, ident._det._conditioned)
    ctr0 = None if origin is None else [None, origin, None, None, None]
    assert ident.identify_batch(clips, rates, ctr0) == [[None, None]] * 5
    order, calls, at, cut = _orders(engine), eng.calls, 0, 0
    for la in launches:                                                     # one group per launch: header, hop table, plan, four ranks
        absolute = origin is not None and 1 in la.idx
        head = calls[at:at + 3]
        assert [c.name for c in head] == ["header", "hop_window" if absolute else "schedule_keyed", "plan"], (la.idx, [c.name for c in head])
        assert absolute or head[1].flags == {"want_pn": False}             # (the hop table of clips without origins: bands only)
        at += 3
        totals = _rank_totals(head[2], order, len(la.idx))
        cut += sum(t > CAP and t % CAP > 0 for t in totals)
        for total in totals:
            at = _chunks(calls, at, total, keyed=True)
    assert at == len(calls), [c.name for c in calls[at:at + 8]]             # nothing else: no match, so no final AEAD check either
    assert cut > 0                                                          # some rank was decoded in several chunks and a partial last one


@pytest.fixture(scope="module")
def marked(engine):
    """6 000 samples of noise with frames embedded under KEYS[0] from counter 70 000, a prefix of it, and the noise alone."""
    host = (0.05 * np.random.default_rng(21).standard_normal((1, 6000))).astype(np.float32)
    x = engine.embed(KEYS[0], host, ctr0=70_000, seed=5).audio[0].cpu().numpy()
    return [x, x[:4900].copy(), host[0]]


@pytest.mark.parametrize("span", [(68_000, 72_096), (2 << 16, 66 << 16)], ids=["around-the-frames", "64-high-halves-elsewhere"])
def test_acquire_batch_enumerates_once_per_launch_and_decodes_in_capped_chunks(engine, marked, span):
    eng = _Recording(engine)
    det, _ = _detector(eng)
    launches = cut_launches(marked, [48_000] * 3, 48_000, NB, det._conditioned)
    tries, real = {}, det._acquire_plan

    def acquire_plan(scans, pos0, span_, max_records):
        out = real(scans, pos0, span_, max_records)
        tries.update({i: sum(len(c) for c in p[3]) for i, p in zip(launches[0].idx, out)})      # (one launch: asserted below)
        return out
    det._acquire_plan = acquire_plan
    assert len(launches) == 1
    got = det.acquire_batch(marked, 48_000, span=span)
    calls, wide = eng.calls, span[0] > 72_096
    assert [c.name for c in calls[:2]] == ["header", "acquire_mask"]        # ONE mask launch over the records of every clip ...
    total = int(calls[1].out[1].cpu().numpy().astype(np.int64).sum())        # (the counts it returned)
    assert total == sum(tries.values()) and (total > 0 or not wide)
    at = 2
    if total:                                                               # ... and ONE list launch
        assert calls[2].name == "acquire_list" and calls[2].out[1].numel() == total
        at = 3
    for i in range(len(marked)):                                            # the walk: clip by clip in input order, up to the accepted candidate
        at = _chunks(calls, at, tries[i], keyed=False, upto=None if got[i] is None else got[i].tried)
    assert at == len(calls), [c.name for c in calls[at:at + 8]]
    if wide:                                                                # the frames' own counters are not in the span: every candidate fails
        assert got == [None] * 3 and any(t > CAP and t % CAP for t in tries.values()), tries


def _noise(streams: int, n: int, seed: int):
    return (0.1 * np.random.default_rng(seed).standard_normal((streams, n))).astype(np.float32)


def test_live_monitor_push_decodes_in_capped_chunks(engine):
    eng = _Recording(engine)
    det, sizes = _detector(eng)
    mon = det.open_streams(4, window_s=W8 / 48_000, chunk_max=CM8)
    xs, at = _noise(4, sum(FILL) + CM8, 43), 0
    for ln in FILL:
        mon.push([x[at:at + ln] for x in xs])
        at += ln
    del sizes[:], eng.calls[:]
    assert mon.push([x[at:at + CM8] for x in xs]) == [False] * 4           # n = 3 646: the longest window that starts at 0
    assert eng.calls[0].name == "header"                                    # one header decode per tick
    _check_detector(eng.calls, 1, sizes, [[0, 1, 2, 3]])


def test_live_identifier_ticks_probe_once_per_rank_and_decode_what_the_memo_does_not_know(engine):
    eng = _Recording(engine)
    ident = WatermarkIdentifier(KEYS, list_size=LIST, engine=eng)
    ident._pair_cap = lambda: CAP
    live = ident.open_streams(2, window_s=W8 / 48_000, chunk_max=CM8)
    assert live.memo_slots > 0
    fill = (1300, 1300, 1046)                                               # n = 3 646; both recorded ticks then look at [2 432, n)
    xs, pos = _noise(2, sum(fill) + CM8 + 64, 44), 0
    for ln in fill:
        live.push([x[pos:pos + ln] for x in xs])
        pos += ln
    live.forget()                                                           # the first recorded tick starts with an empty memo
    order, seen = _orders(engine), []
    for ln in (CM8, 64):
        del eng.calls[:]
        assert live.push([x[pos:pos + ln] for x in xs]) == [[None, None]] * 2
        pos += ln
        calls = eng.calls
        assert [c.name for c in calls[:2]] == ["header", "plan"]            # one of each per tick; the window's hop table was built by the first push
        at, planned, decoded, probes = 2, 0, 0, 0
        for total in _rank_totals(calls[1], order, 2):
            if not total:
                continue
            assert calls[at].name == "memo_probe" and calls[at].shapes == [(total,), (total,)], (at, calls[at].name, calls[at].shapes)
            new = int((calls[at].out.cpu().numpy() == 0).sum())             # what the memo does not know is decoded ...
            at = _chunks(calls, at + 1, new, keyed=True)
            if new:                                                         # ... and remembered by ONE insert per rank
                assert calls[at].name == "memo_insert" and calls[at].shapes == [(new,), (new,)], (at, calls[at].name, calls[at].shapes)
                at += 1
            planned, decoded, probes = planned + total, decoded + new, probes + 1
        assert at == len(calls), [c.name for c in calls[at:at + 8]]
        assert live.stats == {"planned": planned, "decoded": decoded, "skipped": planned - decoded}
        seen.append((planned, decoded, probes))
    (p1, d1, r1), (p2, d2, r2) = seen
    assert d1 == p1 > CAP and r1 > 0                                    # an empty memo: everything planned is decoded, in several chunks
    assert r2 > 0 and d2 < p2                                               # the second tick: one probe per rank, fewer rows decoded than planned
