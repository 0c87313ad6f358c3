"""GPU: the launch sequence of verify_batch and identify_batch, counted at the engine.

A queue of five short noise clips is cut by scan.cut_launches; a wrapper around the engine (here only, not in the library) counts the
calls of its methods.  Per launch there is one sync-family call -- sync_fast where the launch's clips are equally long and no longer than
FAST_MAX_LAGS + 62 = 4 158 samples, sync where they are equally long and longer, sync_ragged where they differ --, one resample_ragged
call where the call has a clip at another rate and none otherwise, and one header decode: under the detector's key for verify_batch,
over all keys for identify_batch, which makes no second one and leaves its detector alone."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier
from echoseal_amd.scan import cut_launches, sync_launch

KEYS = [b"\xAA" * 32, bytes(range(32))]
COUNTED = ("sync_fast", "sync", "sync_ragged", "resample_ragged", "header")


class _Counting:
    """An engine's attributes handed through, the calls of its methods counted by name."""

    def __init__(self, eng) -> None:
        self._eng, self.calls = eng, collections.Counter()

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not callable(attr):
            return attr

        def counted(*a, **k):
            self.calls[name] += 1
            return attr(*a, **k)
        return counted


class _Watched(WatermarkDetector):
    """A detector that records the names of the attributes assigned to it."""
    assigned: list = []

    def __setattr__(self, name, value):
        _Watched.assigned.append(name)
        super().__setattr__(name, value)


def _queue():
    rng = np.random.default_rng(41)
    f = lambda n: (0.1 * rng.standard_normal(n)).astype(np.float32)
    pcm = np.clip(np.round(0.1 * rng.standard_normal(3500) * 32768), -32768, 32767).astype(np.int16)
    return [f(3000), f(3000), f(4100), pcm, f(3300)], [48_000, 48_000, 48_000, 48_000, 44_100]


def _expected(engine, clips, rates):
    """The call counts the launch cut asks for; every launch must have a peak that can hold a frame."""
    det = WatermarkDetector(KEYS[0], list_size=2, engine=engine)
    launches = cut_launches(clips, rates, 48_000, 4, det._conditioned)
    want = collections.Counter()
    for la in launches:
        equal = min(la.sizes) == max(la.sizes)
        want["sync_ragged" if not equal else "sync_fast" if max(la.sizes) - 62 <= engine.FAST_MAX_LAGS else "sync"] += 1
        want["resample_ragged"] += la.rates is not None
        assert sync_launch(engine, la, range(4)).rows.size > 0, la.idx      # ... so the header count below is not vacuous
        want["header"] += 1
    return launches, want


def _counts(eng):
    return {name: eng.calls[name] for name in COUNTED}


def test_verify_batch_same_rate_launch_sequence(engine):
    clips, rates = _queue()
    clips, rates = clips[:4], rates[:4]
    launches, want = _expected(engine, clips, rates)
    assert [la.idx for la in launches] == [[0, 1, 2], [3]] and all(la.rates is None for la in launches)
    eng = _Counting(engine)
    res = WatermarkDetector(KEYS[0], list_size=2, engine=eng).verify_batch(clips, rates)
    assert res == [False] * 4
    assert _counts(eng) == {"sync_fast": 1, "sync": 0, "sync_ragged": 1, "resample_ragged": 0, "header": 2} == {n: want[n] for n in COUNTED}


def test_verify_batch_mixed_rate_launch_sequence(engine):
    clips, rates = _queue()
    launches, want = _expected(engine, clips, rates)
    assert [la.idx for la in launches] == [[0, 1, 4, 2], [3]] and all(la.rates is not None for la in launches)
    assert [la.sizes for la in launches] == [[3000, 3000, 3592, 4100], [3500]]
    eng = _Counting(engine)
    res = WatermarkDetector(KEYS[0], list_size=2, engine=eng).verify_batch(clips, rates)
    assert res == [False] * 5
    assert _counts(eng) == {"sync_fast": 1, "sync": 0, "sync_ragged": 1, "resample_ragged": 2, "header": 2} == {n: want[n] for n in COUNTED}


def test_identify_batch_launch_sequence_and_untouched_detector(engine):
    clips, rates = _queue()
    launches, want = _expected(engine, clips, rates)
    assert len(launches) == 2
    eng = _Counting(engine)
    ident = WatermarkIdentifier(KEYS, list_size=2, engine=eng)
    det = ident._det
    det.__class__ = _Watched
    before = dict(vars(det))
    _Watched.assigned.clear()
    res = ident.identify_batch(clips, rates)
    assert _Watched.assigned == []                                          # no attribute of the detector is reassigned ...
    assert det._engine is eng is before["_engine"]                          # ... its engine least of all
    assert vars(det).keys() == before.keys() and all(vars(det)[k] is v for k, v in before.items())
    assert res == [[None, None]] * 5
    # ONE header decode per group (over both keys), not a second one under the detector's own key
    assert _counts(eng) == {"sync_fast": 1, "sync": 0, "sync_ragged": 1, "resample_ragged": 2, "header": 2} == {n: want[n] for n in COUNTED}
