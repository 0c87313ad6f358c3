"""CPU-side checks of acquisition: the C ABI surface and code objects of es_acquire_mask_batch / es_acquire_list_batch, the
host twin against brute force, the record order, the origin a found frame implies, and every refusal without an engine."""
import ctypes
import os
import re

import numpy as np
import pytest

from code_objects import code_objects, disassembly, kernel_metadata

from echoseal_amd import acquire as A
from echoseal_amd.detector import FRAME_LEN, LiveMonitor, WatermarkDetector
from echoseal_amd.scan import CTR_END, counter_estimate
from echoseal_amd.utils import band_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = b"\x5C" * 32
NEW_ENTRY_POINTS = {"es_acquire_mask_batch": 13, "es_acquire_list_batch": 11}
NEW_KERNELS = ("es_acquire_mask_kernel", "es_acquire_list_kernel", "es_acquire_count_kernel")
POS_BIG = 1216 * 2 ** 30


def test_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    hdr = open(os.path.join(ROOT, "include", "echoseal_hip.h")).read()
    lib = ctypes.CDLL(nat.LIB_PATH)
    for name, nargs in NEW_ENTRY_POINTS.items():
        decl = re.search(rf"\bint {name}\s*\(([^;]*)\)\s*;", hdr)
        assert decl, name
        assert name in nat.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(nat.SIGNATURES[name][1]) == nargs, name
        assert nat.SIGNATURES[name][0] is ctypes.c_int and hasattr(lib, name), name
    assert lib.es_abi_version() == nat.ES_ABI_VERSION == int(re.search(r"#define\s+ES_ABI_VERSION\s+(\d+)", hdr).group(1)) == 2      # additive


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
            assert len(ops) > 20, name
            assert not [op for op in ops if op.startswith(("flat_", "scratch_"))], name
            m = md[name]
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
    assert hits == 1, kernel


def test_launchers_take_their_exact_grid():
    src = open(os.path.join(ROOT, "echoseal_amd", "csrc", "es_keyring.hip")).read()
    for name in ("es_launch_acquire_mask", "es_launch_acquire_list"):
        body = src[src.index(f"int {name}("):]
        body = body[:body.index("\n}\n")]
        assert "es_grid(" not in body and "es_acquire_" in body, name


# ------------------------------------------------------------------------------------------------------------------- twin
def _brute(key, lo16, band, lo, hi):
    c = np.arange(lo, hi, dtype=np.int64)                                   # every counter of the span
    return [int(v) for v in c[(c & 0xFFFF) == lo16] if band_index(key, int(v)) == band]


@pytest.mark.parametrize("span", [(0, 1 << 20), (70_001, (1 << 19) + 5), (65_536, 65_536 * 3), (5, 5), (70_000, 70_000), (0, 1), (65_535, 65_537)])
def test_candidates_equal_brute_force(span):
    assert span[1] - span[0] <= 1 << 20
    total = 0
    for lo16 in (0, 1, 4464, 4465, 65_535):
        by_band = [A.candidates(KEY, lo16, b, span) for b in range(4)]
        for b in range(4):
            assert by_band[b] == _brute(KEY, lo16, b, *span), (lo16, b)
        want_all = [c for c in range((span[0] & ~0xFFFF) | lo16, span[1], 65_536) if c >= span[0]]
        assert sorted(sum(by_band, [])) == want_all                         # every counter with the low half is on exactly one band
        total += len(want_all)
    assert total > 0 or span[1] - span[0] <= 2
    assert A.candidates(KEY, -1, 0, span) == [] and A.candidates(KEY, 65_536, 0, span) == []


def test_span_words_and_the_mask_model():
    assert A.span_words((0, CTR_END)) == (0, 65_536, 2048)
    assert A.span_words((70_001, (1 << 22) + 5)) == (1, 64, 2)
    assert A.span_words((0, 0)) == (0, 0, 0) and A.span_words((70_000, 70_000)) == (1, 1, 1) and A.span_words((CTR_END, CTR_END)) == (65_536, 0, 0)
    assert A.span_words((65_536, 65_536 * 34)) == (1, 33, 2) and A.span_words((0, 65 * 65_536)) == (0, 65, 3)
    keys = [KEY, bytes(range(32))]
    span = (70_001, (1 << 21) + 5)
    key_idx, ok, lo16, band = [0, 1, 1, 2, 0, -1], [1, 1, 0, 1, 1, 1], [4464, 4465, 7, 7, 70_000, 7], [0, 1, 2, 3, 1, 0]
    mask, count, cands = A.mask_model(keys, key_idx, ok, lo16, band, span)
    h0, H, W = A.span_words(span)
    assert mask.shape == (6, W) and list(count[2:]) == [0, 0, 0, 0] and count[0] > 0
    for p in range(2):
        assert cands[p] == _brute(keys[key_idx[p]], lo16[p], band[p], *span)
        bits = [h0 + j for j in range(W * 32) if (int(mask[p, j >> 5]) >> (j & 31)) & 1]
        assert [(h << 16) | lo16[p] for h in bits] == cands[p] and count[p] == len(cands[p])
    assert 4464 < (70_001 & 0xFFFF) and cands[0][0] >= 2 << 16             # the first high half is excluded by the low half
    rec, ctr = np.full(int(count.sum()) + 3, -9, np.int32), np.full(int(count.sum()) + 3, 77, np.int64)
    A.list_model(cands, [int(count[1]) + 1, 0, -1, -1, 0, 0], rec, ctr)
    assert list(ctr[:count[1]]) == cands[1] and list(ctr[count[1] + 1: count[1] + 1 + count[0]]) == cands[0]
    assert rec[count[1]] == -9 and list(rec[-2:]) == [-9, -9] and set(rec[:count[1]]) == {1}


# ------------------------------------------------------------------------------------------------------------------- record order
def test_record_order():
    est = lambda st, pos0=0: counter_estimate(st, pos0)
    # eight fitting peaks over the band rows 0 0 1 1 2 2 3 3; residues: r = 100 shared by peaks 3, 4, 6; r = 7 by 1, 5; singles 0, 2; 7 not ok
    starts = np.array([10, 1300, 50, 2500, 1225, 3700, 2440, 90])
    place = np.array([0, 0, 1, 1, 2, 2, 3, 3])
    res = [5, 7, 9, 100, 100, 7, 100, 100]
    lo16 = np.array([(est(s) + r) & 0xFFFF for s, r in zip(starts, res)])
    ok = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    assert A.record_order(ok, lo16, place, starts) == [3, 4, 6, 1, 5, 0, 2]   # shared residue first; ties by band place, then peak order
    assert A.record_order(ok, lo16, place, starts, max_records=4) == [3, 4, 6, 1]
    assert A.record_order(ok, lo16, place, starts, max_records=1) == [3]
    # residues wrap: a counter just past a multiple of 65 536 agrees with the one before it
    lo_wrap = np.array([65_535, 0, 4])
    st_wrap = np.array([0, 1215, 2430])
    assert A.record_order(np.ones(3, bool), lo_wrap, np.zeros(3, int), st_wrap) == [0, 1, 2]
    assert A.record_order(np.ones(3, bool), lo_wrap, np.array([2, 1, 0]), st_wrap) == [1, 0, 2]      # the pair first, inside it by band place
    # a window at an absolute position: the estimate counts from the stream's first sample
    lo_abs = np.array([(est(s, POS_BIG) + r) & 0xFFFF for s, r in zip(starts, res)])
    assert A.record_order(ok, lo_abs, place, starts, POS_BIG) == [3, 4, 6, 1, 5, 0, 2]
    bad = np.array([70_000, -1, 4])
    assert A.record_order(np.ones(3, bool), bad, np.zeros(3, int), st_wrap) == [2]                     # a low half that is none counts as not ok
    assert A.record_order(np.zeros(0, bool), np.zeros(0, int), np.zeros(0, int), np.zeros(0, int)) == []


# ------------------------------------------------------------------------------------------------------------------- origins
@pytest.mark.parametrize("pos0", (0, 1216, POS_BIG))
def test_origin_of(pos0):
    rng = np.random.default_rng(pos0 % 977)
    for start, ctr in zip(rng.integers(0, 240_000, 300).tolist(), rng.integers(0, CTR_END, 300).tolist()):
        o = A.origin_of(ctr, start, pos0)
        k = (2 * (pos0 + start) + FRAME_LEN) // (2 * FRAME_LEN)
        assert o == max(0, ctr - k) and 0 <= o <= ctr
        if ctr >= k:
            assert counter_estimate(start, pos0, o) == ctr
    assert A.origin_of(70_003, 3 * 1215 + 4, 0) == 70_000 and A.origin_of(70_003, 4, 3 * 1215) == 70_000
    # the clamp: a frame whose counter is below the frames the position has passed gives origin 0
    assert A.origin_of(2, 5 * 1215, pos0) == 0 and A.origin_of(0, 0, pos0) == 0
    # a frame found one frame off its position (a peak at the edge of rounding): the estimate lands within 1 of the counter
    for start in (606, 607, 608, 1822, 1823):
        for ctr in (1, 2, 70_000):
            k = counter_estimate(start, pos0)
            if ctr + 1 >= k:
                assert abs(counter_estimate(start, pos0, A.origin_of(ctr, start, pos0)) - ctr) <= 1


# ------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("span, match", [((-1, 5), r"outside \[0, 2\^32\]"), ((0, CTR_END + 1), r"outside \[0, 2\^32\]"), ((9, 3), "reversed"),
                                         ((0.0, 5), "integers"), ((0, True), "integers"), (7, "pair"), ((1, 2, 3), "pair")])
def test_spans_that_are_none_are_refused_without_an_engine(span, match):
    from echoseal_amd.monitor import host_table
    det = WatermarkDetector(KEY, list_size=8)
    mon = LiveMonitor(det, host_table(2, 3648, 1300, fs_target=48_000))
    x = np.zeros(4000, np.float32)
    for call in (lambda: det.acquire(x, 48_000, span=span), lambda: det.acquire_batch([x, x], 48_000, span=span), lambda: mon.acquire(span=span),
                 lambda: mon.acquire([0], span=span)):
        with pytest.raises(ValueError, match=match):
            call()
    assert det._engine is None


def test_max_records_and_streams_are_checked_without_an_engine():
    from echoseal_amd.monitor import host_table
    det = WatermarkDetector(KEY, list_size=8)
    tab = host_table(4, 3648, 1300, fs_target=48_000, ctr0=[None, 5, None, None])
    tab.live[3] = False
    mon = LiveMonitor(det, tab)
    x = np.zeros(4000, np.float32)
    for bad in (0, -1, 1.5, True, None):
        for call in (lambda: det.acquire(x, 48_000, max_records=bad), lambda: det.acquire_batch([x], 48_000, max_records=bad),
                     lambda: mon.acquire([0], max_records=bad)):
            with pytest.raises(ValueError, match="max_records"):
                call()
    with pytest.raises(ValueError, match="closed"):
        mon.acquire([3])
    with pytest.raises(ValueError, match="twice"):
        mon.acquire([0, 0])
    with pytest.raises(ValueError, match="already has a counter origin"):
        mon.acquire([0, 1])
    with pytest.raises(ValueError, match="outside"):
        mon.acquire([4])
    assert list(mon.acquire_streams(None)) == [0, 2] and list(mon.acquire_streams([2, 0])) == [2, 0]
    # an empty span: nothing to look for, and no GPU work
    assert det.acquire(x, 48_000, span=(70_000, 70_000)) is None and det.acquire_batch([x, x], 48_000, span=(0, 0)) == [None, None]
    assert mon.acquire(span=(5, 5)) == [None, None] and mon.acquire([2], span=(CTR_END, CTR_END)) == [None] and mon.acquire([]) == []
    assert det._engine is None and [mon.origin(s) for s in range(3)] == [None, 5, None]
