"""CPU-side checks of counter origins: the planner's host twin against WatermarkDetector._scan_plan at origins and
absolute positions across the counter range, the memo's encoding for streams with an origin, every refusal without an engine, and the
C ABI surface and code objects of es_plan_at_batch / es_hop_window_batch."""
import ctypes
import os

import numpy as np
import pytest

from code_objects import code_objects, disassembly, kernel_metadata
from identify_cases import detector_plan, random_scan, reference_plan

from echoseal_amd.detector import FRAME_LEN, WatermarkDetector, _Scan
from echoseal_amd.identify import LiveIdentifier, WatermarkIdentifier, plan_reference
from echoseal_amd.scan import CTR_END, check_counter_reach, counter_estimate, counter_origins
from echoseal_amd.utils import BAND_PLAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGINS = (0, 1, 199, 200, 201, 65_436, 65_536)                            # the last two: the low-16 gate across the 0xFFFF boundary
POS_BIG = 1216 * 2 ** 30                                                   # 2 * (pos0 + start) passes 2^41: 64-bit arithmetic or nothing
NEW_ENTRY_POINTS = ("es_plan_at_batch", "es_hop_window_batch")
NEW_KERNELS = ("es_plan_at_kernel", "es_hop_window_kernel")


class _HopAt:
    """BandHop stand-in over a hop window: band of counter ctr = BAND_PLAN[hop[ctr - base]], no band outside the window."""

    def __init__(self, hop, base):
        self._hop, self._base = hop, int(base)

    def band(self, ctr):
        col = int(ctr) - self._base
        return BAND_PLAN[int(self._hop[col])] if 0 <= col < len(self._hop) else None


def at_scan(rng, pos0, ctr0, kind=None, M=None):
    """identify_cases.random_scan moved to (pos0, ctr0): the same peaks, lengths and header hits, with a hop window that starts at
    base = max(0, ctr0 + est(pos0) - 200), ceil(M / 1215) + 402 wide, and low-16 words drawn around the absolute estimates."""
    s = random_scan(rng, kind, M)
    base = max(0, counter_estimate(0, pos0, ctr0) - 200)
    C = -(-s.M // FRAME_LEN) + 402
    p = {"mixed": 0.25, "dense": 0.9, "sparse": 0.02, "all": 1.0, "gap": 0.25}[s.kind]
    other = (s.band + 1 + rng.integers(0, 3, C)) % 4
    hop = np.where(rng.random(C) < p, s.band, other).astype(np.uint8)
    est = np.array([counter_estimate(int(st), pos0, ctr0) for st in s.fit], np.int64)
    if s.kind == "gap":
        for e in est:
            lo = max(0, int(e) - 3 - base)
            hop[lo:int(e) + 4 - base] = other[lo:int(e) + 4 - base]
    lo16 = rng.integers(0, 65536, s.fit.size).astype(np.int32)
    for j in np.flatnonzero(rng.random(s.fit.size) < 0.6):
        c = int(est[j]) + int(rng.integers(-200, 201))
        if 0 <= c < CTR_END:
            lo16[j] = c & 0xFFFF
            if rng.random() < 0.7 and 0 <= c - base < C:
                hop[c - base] = s.band
    s.hop, s.hdr_lo16 = hop, lo16
    return s, base


def detector_plan_at(s, base, pos0, ctr0):
    """WatermarkDetector._scan_plan on the scan with the origin carried by the scan -> ([(start, ctr, header-log index)], looked)."""
    det = WatermarkDetector(bytes(32), list_size=1)
    det._hop = _HopAt(s.hop, base)
    nf = s.fit.size
    scan = _Scan(bands=[BAND_PLAN[s.band]], src=None, sel=np.arange(nf), rows=np.zeros(nf, np.int64), starts=s.fit.astype(np.int64),
                 hdr=(s.hdr_ok.astype(bool), s.hdr_lo16.astype(np.int64), np.zeros(nf)), ctr0=ctr0, pos0=pos0)
    plan, hdr_log = det._scan_plan(scan, 0)
    return [(start, ctr, h) for (_j, start, ctr, h) in plan], len(hdr_log)


def reference_plan_at(s, base, pos0, ctr0):
    plan, looked = plan_reference(s.peaks, s.npeaks, s.M, s.band, s.hdr_ok, s.hdr_lo16, s.hop, pos0=pos0, ctr0=ctr0, hop_base=base)
    fit_rank = np.cumsum((s.peaks >= 0) & (s.peaks + FRAME_LEN <= s.M)) - 1
    return [(int(s.peaks[slot]), ctr, int(fit_rank[slot])) for slot, ctr in plan], looked


def _count(seen, s, want, looked):
    seen["empty"] += not want
    seen["cut"] += len(want) == 400 and looked < s.fit.size
    for j in range(looked):
        mine = [c for (_s, c, h) in want if h == j]
        seen["hdr_hit"] += bool(s.hdr_ok[j] and mine)
        seen["hdr_miss"] += bool(s.hdr_ok[j] and not mine)
        seen["wide_fallback"] += bool(not s.hdr_ok[j] and len(mine) > 7)
        seen["tight"] += bool(not s.hdr_ok[j] and 0 < len(mine) <= 7)


@pytest.mark.parametrize("pos0", (0, 1216, 1216 * 37, POS_BIG))
def test_plan_reference_equals_scan_plan_at_origins(pos0):
    rng = np.random.default_rng(418 + pos0 % 1000)
    seen = {"cut": 0, "wide_fallback": 0, "tight": 0, "hdr_hit": 0, "hdr_miss": 0, "empty": 0}
    for it in range(280):
        ctr0 = ORIGINS[it % len(ORIGINS)]
        s, base = at_scan(rng, pos0, ctr0)
        want, want_log = detector_plan_at(s, base, pos0, ctr0)
        got, looked = reference_plan_at(s, base, pos0, ctr0)
        assert got == want and looked == want_log, (it, s.kind, pos0, ctr0, got[:5], want[:5])
        lo = counter_estimate(0, pos0, ctr0) - 200
        assert all(max(0, lo) <= c <= counter_estimate(s.M, pos0, ctr0) + 200 for _s, c, _h in want)      # real counters, inside the window's reach
        _count(seen, s, want, looked)
    assert all(v >= 3 for v in seen.values()), seen


def test_zero_origin_plans_what_no_origin_plans():
    """pos0 = ctr0 = 0 against both functions as they are called without the new arguments (identify_cases)."""
    rng = np.random.default_rng(2025)
    seen = {"cut": 0, "wide_fallback": 0, "tight": 0, "hdr_hit": 0, "hdr_miss": 0, "empty": 0}
    for it in range(300):
        s = random_scan(rng)
        want, want_log = detector_plan(s)
        ref, ref_looked, _ = reference_plan(s)
        assert (ref, ref_looked) == (want, want_log)
        assert detector_plan_at(s, 0, 0, 0) == (want, want_log), (it, s.kind)
        assert reference_plan_at(s, 0, 0, 0) == (want, want_log), (it, s.kind)
        _count(seen, s, want, want_log)
    assert all(v >= 3 for v in seen.values()), seen


def test_the_low16_gate_across_0xffff():
    """Origins 65 436 and 65 536 with a header that reads the low word of a counter on either side of 0x10000."""
    for ctr0 in (65_436, 65_536):
        for target in (65_535, 65_536, 65_537):
            M = 48_000
            peaks = np.full(32, -1, np.int32)
            peaks[0] = start = 1215 * max(0, min(38, target - ctr0)) if target >= ctr0 else 0
            base = max(0, ctr0 - 200)
            hop = np.zeros(-(-M // FRAME_LEN) + 402, np.uint8)              # every counter on band 0
            plan, looked = plan_reference(peaks, 1, M, 0, [1], [target & 0xFFFF], hop, ctr0=ctr0, hop_base=base)
            est = counter_estimate(start, 0, ctr0)
            want = [c for c in range(est - 200, est + 201) if (c & 0xFFFF) == (target & 0xFFFF)]
            assert [c for _s, c in plan] == want and target in want and looked == 1, (ctr0, target, plan)


def test_counters_above_the_last_never_appear():
    rng = np.random.default_rng(7)
    ctr0, top = CTR_END - 300, 0
    for it in range(120):
        s, base = at_scan(rng, 0, ctr0, M=int(rng.choice([48_000, 240_000])), kind=("dense", "all", "mixed")[it % 3])
        want, want_log = detector_plan_at(s, base, 0, ctr0)
        got, looked = reference_plan_at(s, base, 0, ctr0)
        assert got == want and looked == want_log, it
        assert all(0 <= c <= CTR_END - 1 for _s, c, _h in want)
        top = max([top] + [c for _s, c, _h in want])
    assert top >= CTR_END - 100                                             # the windows did reach the end of the range
    # one peak 100 counters before the end, every counter on its band: the wide window is cut at 2^32 - 1, the tight one is whole
    peaks = np.full(32, -1, np.int32)
    peaks[0] = 200 * 1215
    hop = np.zeros(-(-300_000 // FRAME_LEN) + 402, np.uint8)
    for hdr_ok, lo16, want in ((1, (CTR_END - 1) & 0xFFFF, [CTR_END - 1]), (0, 0, list(range(CTR_END - 103, CTR_END - 96)))):
        plan, _ = plan_reference(peaks, 1, 300_000, 0, [hdr_ok], [lo16], hop, ctr0=ctr0, hop_base=ctr0 - 200)
        assert [c for _s, c in plan] == want
    hop[:] = 1
    hop[CTR_END - 50 - (ctr0 - 200):] = 0                                   # the band only from 2^32 - 50 on: the wide fallback ends at the last counter
    plan, _ = plan_reference(peaks, 1, 300_000, 0, [0], [0], hop, ctr0=ctr0, hop_base=ctr0 - 200)
    assert [c for _s, c in plan] == list(range(CTR_END - 50, CTR_END))


def test_counter_estimate_in_64_bits():
    assert counter_estimate(607, 0, 0) == 0 and counter_estimate(608, 0, 0) == 1
    assert counter_estimate(0, POS_BIG, 5) == 5 + (2 * POS_BIG + 1215) // 2430 == 5 + round(POS_BIG / 1215)
    rng = np.random.default_rng(3)
    for pos0, start, ctr0 in zip(rng.integers(0, 2 ** 47, 2000).tolist(), rng.integers(0, 2 ** 24, 2000).tolist(), rng.integers(0, 2 ** 31, 2000).tolist()):
        a = pos0 + start
        q, r = divmod(a, 1215)
        assert counter_estimate(start, pos0, ctr0) == ctr0 + q + (r > 607)


def test_pack_abs():
    from echoseal_amd import memo
    for d in (0, 400):
        k0, k1 = memo.pack_abs([3], [9], [2], [2 ** 40 + 5], [d])
        assert memo.unpack(k0, k1) == tuple(np.array([v]) for v in (3, 9, 2, 2 ** 40 + 5, d))
        assert (k0, k1) == memo.pack([3], [9], [2], [2 ** 40 + 5], [d])     # the same record layout, another meaning of the last field
    for d in (-1, 401):
        with pytest.raises(ValueError, match="delta"):
            memo.pack_abs([3], [9], [2], [5], [d])
    with pytest.raises(ValueError, match="delta"):
        memo.pack_abs([1, 2], [0, 0], [0, 0], [5, 6], [400, 401])


def _no_engine(obj):
    det = obj._det if isinstance(obj, WatermarkIdentifier) else obj
    assert det._engine is None
    return obj


@pytest.mark.parametrize("bad, match", [(-1, r"\[0, 2\^32\)"), (2 ** 32, r"\[0, 2\^32\)"), (1.5, "integer"), ("7", "integer"), (True, "integer"),
                                        ([1, 2, 3], "3 counter origins")])
def test_origins_that_are_no_counters_are_refused_without_an_engine(bad, match):
    x = np.zeros(4000, np.float32)
    det, ident = WatermarkDetector(bytes(32), list_size=8), WatermarkIdentifier([bytes(32)], list_size=8)
    one = bad if isinstance(bad, list) else [bad, None]
    for call in (lambda: det.verify_batch([x, x], 48_000, one), lambda: ident.identify_batch([x, x], 48_000, one),
                 lambda: det.open_streams(2, ctr0=one), lambda: ident.open_streams(2, ctr0=one, window_s=0.1, chunk_max=1300)):
        with pytest.raises(ValueError, match=match):
            call()
    if not isinstance(bad, list):
        for call in (lambda: det.verify(x, 48_000, bad), lambda: ident.identify(x, 48_000, bad), lambda: det.open_streams(2, ctr0=bad),
                     lambda: ident.open_streams(2, ctr0=bad)):
            with pytest.raises(ValueError, match=match):
                call()
    _no_engine(det), _no_engine(ident)
    assert counter_origins(None, 2) == [None, None] and counter_origins(7, 2) == [7, 7] and counter_origins([np.int64(5), None], 2) == [5, None]
    assert counter_origins(2 ** 32 - 1, 1) == [2 ** 32 - 1]


def test_a_clip_or_a_push_that_reaches_the_end_of_the_counters_is_refused_without_an_engine():
    from echoseal_amd.monitor import host_table
    det, ident = WatermarkDetector(bytes(32), list_size=8), WatermarkIdentifier([bytes(32)], list_size=8)
    x = np.zeros(12_150, np.float32)                                        # 10 frames: ctr0 + 10 + 201 <= 2^32 - 1
    edge = CTR_END - 1 - 211
    check_counter_reach(edge, x.size)
    check_counter_reach(None, 10 ** 12)
    for ctr0 in (edge + 1, CTR_END - 1):
        for call in (lambda: det.verify(x, 48_000, ctr0), lambda: det.verify_batch([x[:100], x], 48_000, [None, ctr0]),
                     lambda: ident.identify(x, 48_000, ctr0), lambda: ident.identify_batch([x, x], 48_000, [0, ctr0])):
            with pytest.raises(ValueError, match=r"2\^32 - 1"):
                call()
    with pytest.raises(ValueError, match=r"2\^32 - 1"):                    # the length that counts is the one at fs_target
        det.verify(x[:6100], 24_000, edge + 1)
    # a push: the stream's position after the chunk, from the table's host records alone
    tab = host_table(2, 3648, 1300, ctr0=[edge, None], fs_target=48_000)
    live, mon = LiveIdentifier(ident, tab, memo_slots=0), None
    assert live.origin(0) == edge and live.origin(1) is None
    tab.n_host[:] = 12_150 - 100
    from echoseal_amd.monitor import push_arguments
    push_arguments(tab, 48_000, [x[:100], x[:1300]], [0, 1])
    with pytest.raises(ValueError, match=r"2\^32 - 1"):
        live.push([x[:101]], [0])
    from echoseal_amd.detector import LiveMonitor
    mon = LiveMonitor(det, tab)
    with pytest.raises(ValueError, match=r"2\^32 - 1"):
        mon.push([x[:101], x[:5]], [0, 1])
    for bad in (-1, 2 ** 32, 0.5, [1, 2]):
        with pytest.raises(ValueError):
            live.add(1, ctr0=bad)
        with pytest.raises(ValueError):
            mon.add(1, ctr0=bad)
    _no_engine(det), _no_engine(ident)


def test_an_origin_lifts_the_memos_window_refusal_for_its_stream():
    ident = WatermarkIdentifier([bytes(32)], list_size=8)
    long_s = (65_535 - 201) * 1215 / 48_000 + 1.0                           # ceil(W / 1215) + 201 > 65 535
    with pytest.raises(ValueError, match="memo"):
        ident.open_streams(2, window_s=long_s, memo_slots=1024)
    with pytest.raises(ValueError, match="memo"):
        ident.open_streams(2, window_s=long_s, memo_slots=1024, ctr0=[5, None])
    LiveIdentifier.check_memo(1024, 1, int(long_s * 48_000), relative=False)
    with pytest.raises(ValueError, match="memo"):
        LiveIdentifier.check_memo(1024, 1, int(long_s * 48_000))
    _no_engine(ident)


def test_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        assert name in nat.DECLARATIONS, name
        assert name in nat.SIGNATURES, name
        assert len(nat.DECLARATIONS[name]) == len(nat.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.es_abi_version() == nat.ES_ABI_VERSION == nat.CONSTANTS["ES_ABI_VERSION"] == 2      # additive
    assert len(nat.SIGNATURES["es_plan_at_batch"][1]) == len(nat.SIGNATURES["es_plan_ragged_batch"][1]) + 5      # four arrays and HR


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_new_kernels_stay_out_of_flat_and_private_memory(tmp_path, kernel):
    hits = 0
    for co in code_objects(tmp_path):
        md = kernel_metadata(co)
        names = [k for k in md if kernel in k]
        if not names:
            continue
        funcs = disassembly(co)
        for name in names:
            hits += 1
            ops = funcs[name]
            assert len(ops) > 50, name
            assert not [op for op in ops if op.startswith(("flat_", "scratch_"))], name
            m = md[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
            if kernel == "es_plan_at_kernel":
                assert m["vgpr_count"] <= 64, (name, m)
    assert hits == 1, kernel
