"""GPU: verify(), verify_batch() and the identifier against traces of the reference's own verify() at every branch of its search
(tests/golden/search_traces.npz, generator oracle/refshim/gen_golden_search.py; tests/test_golden_search.py holds the CPU oracle to
the same fixture and asserts that every case reaches its branch).  List size 1 throughout, as the reference ran.

Result and tries must equal the fixture; of the header records, ok and the low 16 bits exactly, the score within 1e-6 relative (DESIGN
section 2).  Every reference result is False: a True here is a failure to look into."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LIST = 1
SYNC_CALLS = ("sync_fast", "sync", "sync_ragged")                           # the three branches of scan.sync_launch


class _SyncNames:
    """An engine's attributes handed through; the names of its sync calls recorded in order."""

    def __init__(self, eng) -> None:
        self._eng, self.names = eng, []

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if name not in SYNC_CALLS:
            return attr

        def recorded(*a, **k):
            self.names.append(name)
            return attr(*a, **k)
        return recorded


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "search_traces.npz"))


def _cases(g) -> list:
    return [str(c) for c in g["cases"]]


def _keys(g) -> list:
    """The ring of the fixture: the four own keys, then the two strangers."""
    return [k.tobytes() for k in g["keys"]] + [k.tobytes() for k in g["strangers"]]


def _tag(g, name: str, k: int):
    """Under which tag the fixture holds the reference's trace of clip `name` under ring key k (None: it holds none)."""
    return "own" if k == int(g[f"{name}/key"]) else f"s{k - 4}" if k >= 4 else None


def _want(g, name: str, tag: str):
    p = f"{name}/{tag}"
    return ([tuple(int(v) for v in r) for r in g[f"{p}/tries"]],
            [(bool(r[2]), int(r[3]), float(s)) for r, s in zip(g[f"{p}/visited"], g[f"{p}/score"])])


def _check(at, trace, hdr, want) -> None:
    tries, headers = want
    assert [(bool(a), int(b)) for a, b, _ in hdr] == [(a, b) for a, b, _ in headers], (at, "header ok / low 16 bits")
    for j, ((_, _, s), (_, _, ref)) in enumerate(zip(hdr, headers)):
        assert abs(s - ref) <= 1e-6 * max(1.0, abs(ref)), (at, "header score", j, s, ref)
    assert [tuple(t) for t in trace] == tries, (at, "tries", len(trace), len(tries))


@pytest.fixture(scope="module")
def single(engine, gold):
    """verify() of every case under its own key, one call each -> {case: (result, _trace, _hdr_trace, session nonce, sync calls)}."""
    out = {}
    for name in _cases(gold):
        eng = _SyncNames(engine)
        det = WatermarkDetector(_keys(gold)[int(gold[f"{name}/key"])], list_size=LIST, engine=eng)
        det._trace, det._hdr_trace = [], []
        res = det.verify(gold[f"{name}/clip"], int(gold[f"{name}/fs_in"]))
        out[name] = (res, det._trace, det._hdr_trace, det.session_nonce, eng.names)
    return out


@pytest.fixture(scope="module")
def batched(engine, gold):
    """One verify_batch per ring key over every clip the fixture has a trace of under that key -- all of them for a stranger, lengths
    and rates mixed -> {key index: (cases, results, _trace, _hdr_trace, session nonce, sync calls)}."""
    out = {}
    for k, key in enumerate(_keys(gold)):
        names = [n for n in _cases(gold) if _tag(gold, n, k)]
        eng = _SyncNames(engine)
        det = WatermarkDetector(key, list_size=LIST, engine=eng)
        det._trace, det._hdr_trace = [], []
        res = det.verify_batch([gold[f"{n}/clip"] for n in names], [int(gold[f"{n}/fs_in"]) for n in names])
        out[k] = (names, res, det._trace, det._hdr_trace, det.session_nonce, eng.names)
    return out


def test_single_verify_follows_the_reference(gold, single):
    tries = 0
    for name in _cases(gold):
        res, trace, hdr, nonce, _ = single[name]
        assert res is bool(gold[f"{name}/own/result"]) is False and nonce is None, name
        _check(name, trace, hdr, _want(gold, name, "own"))
        tries += len(trace)
    assert tries > 1_000


def test_verify_batch_follows_the_reference(gold, batched):
    for k, (names, res, trace, hdr, nonce, _) in batched.items():
        wants = [_want(gold, n, _tag(gold, n, k)) for n in names]
        assert res == [False] * len(names) and nonce is None, k          # the nonce of sequential verify() calls: nothing was accepted
        _check(("key", k), trace, hdr, ([t for w in wants for t in w[0]], [h for w in wants for h in w[1]]))
    assert len(batched[4][0]) == len(batched[5][0]) == len(_cases(gold))   # a stranger's batch holds every case
    assert len({int(gold[f"{n}/fs_in"]) for n in batched[4][0]}) >= 5 and len({gold[f"{n}/clip"].size for n in batched[4][0]}) >= 10


def test_identifier_follows_the_reference_under_every_key(engine, gold):
    names, keys = _cases(gold), _keys(gold)
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine)
    ident.trace = True
    out, traces = ident.identify_batch([gold[f"{n}/clip"] for n in names], [int(gold[f"{n}/fs_in"]) for n in names])
    assert out == [[None] * len(keys)] * len(names)
    compared = 0
    for n, per_key in zip(names, traces):
        for k in range(len(keys)):
            tag = _tag(gold, n, k)
            if tag:
                _check((n, "key", k), per_key[k][0], per_key[k][1], _want(gold, n, tag))
                compared += 1
    assert compared == 3 * len(names)


def test_cases_go_through_every_sync_branch(gold, single, batched):
    alone = {name: calls for name, (_, _, _, _, calls) in single.items()}
    assert all(len(c) == (gold[f"{n}/clip"].size >= 63) for n, c in alone.items())       # one sync call per verify(), none below the template
    assert {"sync_fast", "sync"} == {c for calls in alone.values() for c in calls}
    assert "sync_ragged" in batched[4][5] and "sync_ragged" in batched[5][5]              # a stranger's batch: every length in one call
