"""CPU-side checks of batching recordings of unequal length: the C ABI surface of the two ragged entry points, the cut of a queue of
clips into launches (detector.ragged_buckets), and the candidate planner's host twin with a sample count of its own per row."""
import ctypes
import os
import re

import numpy as np

from identify_cases import detector_plan, random_scan, reference_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_ENTRY_POINTS = ("es_sync_ragged_batch", "es_plan_ragged_batch")


def test_ragged_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    hdr = open(os.path.join(ROOT, "include", "echoseal_hip.h")).read()
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in RAGGED_ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\)\s*;", hdr)
        assert decl, name
        assert name in nat.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(nat.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.es_abi_version() == nat.ES_ABI_VERSION == int(re.search(r"#define\s+ES_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    # the ragged calls take the arguments of their equal-length twins plus the per-record lengths
    assert len(nat.SIGNATURES["es_sync_ragged_batch"][1]) == len(nat.SIGNATURES["es_sync_batch"][1]) + 1
    assert len(nat.SIGNATURES["es_plan_ragged_batch"][1]) == len(nat.SIGNATURES["es_plan_batch"][1]) + 1


def _check_buckets(lengths, rows, budget):
    from echoseal_amd.detector import ragged_buckets
    buckets = ragged_buckets(lengths, rows, budget)
    flat = [i for b in buckets for i in b]
    assert sorted(flat) == list(range(len(lengths)))                       # every index in exactly one bucket
    for b in buckets:
        assert b, "an empty bucket"
        ls = [lengths[i] for i in b]
        assert ls == sorted(ls)                                            # lengths ascend within a bucket
        assert len(b) == 1 or len(b) * rows * max(ls) <= budget, (b, ls)
    seq = [lengths[i] for i in flat]
    assert seq == sorted(seq)                                              # ... and from bucket to bucket: equal lengths are adjacent
    for a, b in zip(flat, flat[1:]):
        assert lengths[a] != lengths[b] or a < b                           # equal lengths keep their input order
    # greedy: a bucket was closed only because the next clip did not fit
    for b, nxt in zip(buckets, buckets[1:]):
        assert (len(b) + 1) * rows * lengths[nxt[0]] > budget
    assert ragged_buckets(list(lengths), rows, budget) == buckets          # deterministic
    return buckets


def test_ragged_buckets():
    from echoseal_amd.detector import RAGGED_ROW_SAMPLES, ragged_buckets
    assert RAGGED_ROW_SAMPLES == 1 << 26
    assert ragged_buckets([], 4, 100) == []
    assert _check_buckets([5], 4, 1) == [[0]]                              # one oversize clip still goes, alone
    assert _check_buckets([10, 10, 10], 1, 30) == [[0, 1, 2]]
    assert _check_buckets([10, 10, 10], 1, 29) == [[0, 1], [2]]
    assert _check_buckets([30, 10, 20, 10], 2, 120) == [[1, 3, 2], [0]]
    assert _check_buckets([30, 10, 20, 10], 2, 80) == [[1, 3], [2], [0]]
    assert _check_buckets([100, 1, 100, 1], 4, 8) == [[1, 3], [0], [2]]
    rng = np.random.default_rng(5)
    for it in range(200):
        n = int(rng.integers(1, 40))
        lengths = rng.integers(63, 300_000, n).tolist()
        if it % 3 == 0:                                                    # runs of equal lengths
            lengths = [lengths[int(k)] for k in rng.integers(0, max(1, n // 3), n)]
        rows = int(rng.choice([1, 4]))
        budget = int(rng.choice([1, 300_000, 2_000_000, 1 << 26]))
        buckets = _check_buckets(lengths, rows, budget)
        if budget == 1 << 26 and rows * n * max(lengths) <= budget:
            assert len(buckets) == 1
    # a service's queue: 200 uploads of 1 .. 6 s in four bands are a handful of launches, not 200
    lengths = rng.integers(48_000, 288_000, 200).tolist()
    assert len(_check_buckets(lengths, 4, RAGGED_ROW_SAMPLES)) <= 4


def test_launches_group_by_sample_type_and_leave_short_clips_out():
    from echoseal_amd.detector import WatermarkDetector
    f = lambda n: np.zeros(n, np.float32)
    i = lambda n: np.zeros(n, np.int16)
    signals = [f(5000), i(700), f(62), f(63), i(0), f(5000), i(64), f(100)]
    assert WatermarkDetector._launches(signals, 4) == [[3, 7, 0, 5], [6, 1]]
    assert WatermarkDetector._launches([f(10), i(62)], 4) == []


def test_plan_reference_with_a_length_per_row_equals_scan_plan():
    """The ragged planner's twin: rows of one call with a sample count of their own each -- plan_reference with the row's M is
    WatermarkDetector._scan_plan on that row (which sees only the peaks that fit the row's own clip)."""
    rng = np.random.default_rng(77)
    seen_m, unfit, nonempty = set(), 0, 0
    for call in range(40):
        lens = rng.choice([1215, 1216, 1300, 2430, 5000, 12_000, 30_011, 48_000, 240_000], 8)
        assert len(set(lens.tolist())) > 1
        for M in lens:
            s = random_scan(rng, M=int(M))
            want, want_log = detector_plan(s)
            got, looked, _raw = reference_plan(s)
            assert got == want and looked == want_log, (call, int(M), s.kind, got[:4], want[:4])
            n = min(int(s.npeaks) & 0xFFFF, 25)
            unfit += int(((s.peaks[:n] + 1215) > s.M).any())
            nonempty += bool(want)
            seen_m.add(int(M))
    assert len(seen_m) == 9 and unfit >= 20 and nonempty >= 50, (seen_m, unfit, nonempty)
