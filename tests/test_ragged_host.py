"""CPU-side checks of batching recordings of unequal length: the C ABI surface of the two ragged entry points, the cut of a queue of
clips into launches (scan.ragged_buckets and scan.cut_launches; detector re-exports the former), and the candidate planner's host twin with a sample count of its own per row."""
import ctypes
import os

import numpy as np

from identify_cases import detector_plan, random_scan, reference_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_ENTRY_POINTS = ("es_sync_ragged_batch", "es_plan_ragged_batch")


def test_ragged_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in RAGGED_ENTRY_POINTS:
        assert name in nat.DECLARATIONS, name
        assert name in nat.SIGNATURES, name
        assert len(nat.DECLARATIONS[name]) == len(nat.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.es_abi_version() == nat.ES_ABI_VERSION == nat.CONSTANTS["ES_ABI_VERSION"] == 2
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


def _unreached(clip, rate):
    raise AssertionError("a 1-D clip at fs_target, or of a sample type the device conditions, was handed to the host's conditioning")


def test_launches_group_by_sample_type_and_leave_short_clips_out():
    from echoseal_amd.scan import cut_launches
    f = lambda n: np.zeros(n, np.float32)
    i = lambda n: np.zeros(n, np.int16)
    signals = [f(5000), i(700), f(62), f(63), i(0), f(5000), i(64), f(100)]
    cut = lambda sigs: cut_launches(sigs, [48_000] * len(sigs), 48_000, 4, _unreached)
    assert [la.idx for la in cut(signals)] == [[3, 7, 0, 5], [6, 1]]
    assert [la.idx for la in cut([f(10), i(62)])] == []
    assert all(la.rates is None and [c.size for c in la.clips] == la.sizes for la in cut(signals))


# (sample type, samples, rate): lengths at 48 kHz from 60 to 4 354; clips 3, 6, 10 and 15 are shorter than the 63-chip template as they
# come and not after resampling; 4, 5, 13 and 14 stay shorter; 0 / 2 / 7 and 1 / 8 are equally long at 48 kHz across rates and types
MIXED_QUEUE = [("f4", 3000, 48_000), ("i2", 2900, 44_100), ("f8", 1000, 16_000), ("f4", 30, 16_000), ("i2", 62, 48_000), ("f4", 20, 16_000),
               ("f8", 60, 44_100), ("f4", 2756, 44_100), ("i2", 3157, 48_000), ("f8", 4100, 48_000), ("f4", 57, 44_100), ("i2", 500, 16_000),
               ("f4", 4000, 44_100), ("f8", 62, 48_000), ("f4", 56, 44_100), ("i2", 21, 16_000)]


def test_cut_launches_over_a_mixed_rate_queue():
    """The expected idx lists are what the detector's two launch cutters of the commit before scan.py (one for calls with a clip at
    another rate, one for calls without) returned for these queues, run on the CPU; the small budget, 4 rows x 3 clips x 3 000 samples,
    splits every sample type."""
    from echoseal_amd.scan import RAGGED_ROW_SAMPLES, Launch, cut_launches
    from echoseal_amd.utils import resampled_length
    clips = [np.zeros(n, dt) for dt, n, _ in MIXED_QUEUE]
    rates = [fs for _, _, fs in MIXED_QUEUE]
    want = {RAGGED_ROW_SAMPLES: [[10, 3, 0, 7, 12], [6, 2, 9], [15, 11, 1, 8]],                       # float32, float64, int16
            4 * 3 * 3000: [[10, 3, 0], [7, 12], [6, 2], [9], [15, 11], [1, 8]]}
    sizes = [resampled_length(n, fs, 48_000) for _, n, fs in MIXED_QUEUE]
    assert min(sizes) < 63 and sizes[3] >= 63 > MIXED_QUEUE[3][1]
    for budget, idx in want.items():
        kw = {} if budget == RAGGED_ROW_SAMPLES else {"budget": budget}
        launches = cut_launches(clips, rates, 48_000, 4, _unreached, **kw)
        assert [la.idx for la in launches] == idx
        for la in launches:
            assert la.sizes == [sizes[i] for i in la.idx] and la.rates == [rates[i] for i in la.idx] and la.fs_target == 48_000
            assert all(la.clips[k] is clips[i] for k, i in enumerate(la.idx))          # raw, as they came
            assert len({c.dtype for c in la.clips}) == 1
            part = la.part(1, 3)
            assert isinstance(part, Launch) and (part.idx, part.sizes, part.rates) == (la.idx[1:3], la.sizes[1:3], la.rates[1:3])
            assert all(a is b for a, b in zip(part.clips, la.clips[1:3]))
    # the same lengths, all at 48 kHz: the host form, float32 (float64 clips converted) then int16
    host = [np.zeros(n, dt) for (dt, _, _), n in zip(MIXED_QUEUE, sizes)]
    launches = cut_launches(host, [48_000] * len(host), 48_000, 4, _unreached)
    assert [la.idx for la in launches] == [[10, 6, 3, 0, 2, 7, 9, 12], [15, 11, 1, 8]]
    assert [la.clips[0].dtype for la in launches] == [np.float32, np.int16]
    for la in launches:
        assert la.rates is None and la.sizes == [sizes[i] for i in la.idx] == [c.size for c in la.clips]
        assert len({c.dtype for c in la.clips}) == 1


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


def test_cut_launches_conditions_a_clip_outside_the_kernels_limits_on_the_host():
    """A rate pair whose reduced up or down exceeds 2^20 makes the ragged kernel write nothing: such a clip goes down the host-signal
    path -- condition(clip, rate), as 2-D and oddly typed clips do -- while its neighbours stay raw on the device path, so the batch
    call still equals the per-clip calls."""
    from echoseal_amd.scan import cut_launches
    from echoseal_amd.utils import resample_limits
    far = 1_048_583                                                         # coprime to 48 000 and above 2^20
    clips = [np.zeros(3000, np.float32), np.ones(70_000, np.float32), np.zeros(2900, np.int16), np.ones(70_000, np.int16), np.zeros(4000, np.float32)]
    rates = [44_100, far, 44_100, far, 48_000]
    assert resample_limits(70_000, far, 48_000) is not None and resample_limits(3000, 44_100, 48_000) is None
    asked = []

    def condition(clip, rate):
        asked.append((clip.dtype, clip.size, rate))
        return np.full(3205, 0.5, np.float64)                               # what conditioning hands back: some signal at fs_target
    launches = cut_launches(clips, rates, 48_000, 4, condition)
    assert asked == [(np.float32, 70_000, far), (np.int16, 70_000, far)]     # only the two clips out of range, each once
    assert [la.idx for la in launches] == [[1, 3, 0, 4], [2]] and [la.clips[0].dtype for la in launches] == [np.float32, np.int16]
    f32 = launches[0]
    assert f32.rates == [48_000, 48_000, 44_100, 48_000] and f32.sizes == [3205, 3205, 3266, 4000]
    assert f32.clips[2] is clips[0] and f32.clips[3] is clips[4] and launches[1].clips[0] is clips[2]      # raw, as they came
    assert all(c.dtype == np.float32 and c.size == 3205 and (c == 0.5).all() for c in f32.clips[:2])
    # alone in its call it is conditioned on the host as well, and the call is still cut for the device path
    asked.clear()
    (one,) = cut_launches([clips[1]], [far], 48_000, 4, condition)
    assert asked == [(np.float32, 70_000, far)] and one.rates == [48_000] and one.sizes == [3205]
