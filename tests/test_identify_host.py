"""CPU-side checks of the many-key detector: the C ABI surface of its entry points, the candidate planner's host twin against
WatermarkDetector._scan_plan on randomised scans, the integer counter estimate, and the code objects of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from code_objects import code_objects, disassembly, kernel_metadata
from identify_cases import detector_plan, random_scan, reference_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("es_keyring_derive_batch", "es_schedule_keyed_batch", "es_select_keyed_batch", "es_aead_check_keyed_batch", "es_plan_batch")
NEW_KERNELS = ("es_keyring_derive_kernel", "es_schedule_keyed_kernel", "es_plan_kernel", "es_aead_check_keyed_kernel", "es_select_keyed_kernel")


def test_keyed_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    hdr = open(os.path.join(ROOT, "include", "echoseal_hip.h")).read()
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name in NEW_ENTRY_POINTS:
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\)\s*;", hdr)
        assert decl, name
        assert name in nat.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(nat.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    assert lib.es_abi_version() == nat.ES_ABI_VERSION == int(re.search(r"#define\s+ES_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2
    for const in ("ES_KEYRING_BYTES", "ES_MAX_TRIES", "ES_PEAK_LIMIT"):
        assert int(re.search(rf"#define\s+{const}\s+(\d+)", hdr).group(1)) == getattr(nat, const)
    assert nat.ES_KEYRING_BYTES % 16 == 0
    from echoseal_amd import detector
    assert (nat.ES_MAX_TRIES, nat.ES_PEAK_LIMIT) == (detector.MAX_TRIES, detector.PEAK_LIMIT)


def test_identifier_surface_needs_no_gpu():
    import rtwm.identify
    from echoseal_amd.identify import KeyMatch, WatermarkIdentifier
    assert rtwm.identify.WatermarkIdentifier is WatermarkIdentifier and rtwm.identify.KeyMatch is KeyMatch
    with pytest.raises(ValueError):
        WatermarkIdentifier([bytes(32), b"short"])
    assert WatermarkIdentifier([]).identify(np.zeros(100, np.float32), 48_000) == []
    assert WatermarkIdentifier([]).identify_batch([np.zeros(100, np.float32)] * 2, 48_000) == [[], []]
    ident = WatermarkIdentifier([bytes(32), b"\x01" * 32], list_size=8)
    assert ident._pair_cap() == 32768 and ident.trace is False
    assert ident.identify(np.zeros(62, np.float32), 48_000) == [None, None]       # shorter than the preamble: nothing is tried, no GPU is touched


def test_counter_estimate_is_round():
    """(2 * start + 1215) // 2430 == round(start / 1215) for every start below 2^24 (and a spread above): 1215 is odd, so the
    quotient never lies on a tie and Python's round-half-even never comes into play."""
    from echoseal_amd.scan import counter_estimate as ctr_estimate
    start = np.arange(1 << 24, dtype=np.int64)
    assert np.array_equal((2 * start + 1215) // 2430, np.rint(start / 1215).astype(np.int64))
    rng = np.random.default_rng(0)
    for s in [0, 607, 608, 1214, 1215, 1822, 1823, (1 << 24) - 1, *rng.integers(0, 1 << 31, 20_000).tolist()]:
        assert ctr_estimate(s) == int(round(s / 1215)), s


def test_plan_reference_equals_scan_plan():
    rng = np.random.default_rng(2024)
    seen = {"cut": 0, "wide_fallback": 0, "tight": 0, "hdr_hit": 0, "unfit": 0, "empty": 0}
    for it in range(400):
        s = random_scan(rng)
        want, want_log = detector_plan(s)
        got, looked, raw = reference_plan(s)
        assert got == want, (it, s.kind, got[:5], want[:5])
        assert looked == want_log, (it, s.kind)
        n = min(int(s.npeaks) & 0xFFFF, 25)
        seen["unfit"] += int(((s.peaks[:n] + 1215) > s.M).any())
        seen["empty"] += not want
        seen["cut"] += len(want) == 400 and looked < s.fit.size
        for j in range(looked):
            mine = [c for (_s, c, h) in want if h == j]
            seen["hdr_hit"] += bool(s.hdr_ok[j] and mine)
            seen["wide_fallback"] += bool(not s.hdr_ok[j] and len(mine) > 7)
            seen["tight"] += bool(not s.hdr_ok[j] and 0 < len(mine) <= 7)
    assert all(v >= 5 for v in seen.values()), seen
    # a list that reaches MAX_TRIES in the middle of a peak: the last list is cut, later peaks are dropped
    s = random_scan(rng, "gap")
    while not (s.fit.size >= 8 and not s.hdr_ok[:6].any() and s.M >= 48_000):
        s = random_scan(rng, "gap")
    want, want_log = detector_plan(s)
    got, looked, _ = reference_plan(s)
    assert got == want and looked == want_log and len(want) == 400 and want_log < s.fit.size
    est = (2 * int(s.fit[want_log - 1]) + 1215) // 2430
    whole = int((s.hop[max(0, est - 200):est + 201] == s.band).sum())              # the last peak's list before the cut
    assert 0 < len([1 for w in want if w[2] == want_log - 1]) < whole


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
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
            if kernel == "es_plan_kernel":
                assert m["sgpr_spill_count"] == 0 and m["vgpr_count"] <= 64, (name, m)
    assert hits == 1, kernel
