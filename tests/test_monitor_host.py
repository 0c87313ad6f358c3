"""The live monitor without a GPU: the host layout of a tick, the two facts the monitor rests on (pinned against the oracle and SciPy),
the C ABI at the boundary, the Python refusals, and the new kernels' code objects."""
import ctypes
import os

import numpy as np
import pytest

from code_objects import ROOT, code_objects, disassembly, kernel_metadata

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
ENTRY_POINTS = {"es_bpf_stream_batch": 19, "es_xcorr_stream_batch": 13, "es_pick_at_batch": 12}
KERNELS = ("es_bpf_stream_kernel", "es_xcorr_stream_kernel", "es_pick_at_kernel", "es_hist_move_kernel")
W = 3648


# ------------------------------------------------------------------------------------------------ 1. layout
@pytest.mark.parametrize("chunk_max,extra", [(1300, 0), (1300, 777), (100, 0), (5000, 0), (1, 1216)])
def test_layout_over_random_push_sequences(chunk_max, extra):
    from echoseal_amd.monitor import SEG, history_columns, monitor_layout, window_start
    H = history_columns(W, chunk_max) + extra
    rng = np.random.default_rng(chunk_max + extra)
    for trial in range(20):
        n = base = 0
        since_move, moves = None, 0
        for step in range(400):
            ln = int(rng.choice([0, 1, chunk_max, int(rng.integers(0, chunk_max + 1))]))
            lay = monitor_layout([n], [base], [ln], W, H)
            move, nb, col, nn, w0 = (int(a[0]) for a in (lay.move, lay.base, lay.col, lay.n, lay.w0))
            assert nn == n + ln and nb == base + move and col == n - nb
            assert nb % SEG == 0 and w0 % SEG == 0 and move % SEG == 0 and move >= 0
            assert w0 == int(window_start(nn, W)) == SEG * -(-max(0, nn - W) // SEG)
            # every window column, the chunk and the 62 samples before the first new lag are inside the row
            assert 0 <= w0 - nb and nn - nb <= H and col >= 0
            assert max(0, n - 62) - nb >= 0
            # a move happens only when the chunk would not fit, and then it makes the chunk fit
            assert (move > 0) == ((n - base) + ln > H)
            if nn > W:
                assert W - SEG < nn - w0 <= W
            else:
                assert w0 == 0 and nb == 0
            if move:
                if since_move is not None and chunk_max <= W - SEG - 62:
                    assert since_move + ln > H - W - SEG, (since_move, ln)      # at most one move per H - W - 1216 pushed samples
                since_move, moves = 0, moves + 1
            elif since_move is not None:
                since_move += ln
            n, base = nn, nb
        assert moves >= 1 or n <= H


def test_layout_is_vectorised_and_refuses_what_cannot_fit():
    from echoseal_amd.monitor import history_columns, monitor_layout
    H = history_columns(W, 1300)
    a = monitor_layout([0, 6000, 100], [0, 0, 0], [1300, 1300, 0], W, H)
    assert a.move.tolist() == [0, 4864, 0] and a.col.tolist() == [0, 1136, 100] and a.w0.tolist() == [0, 4864, 0]      # 7 300 - 3 648 = 3 652 -> 4 x 1216
    with pytest.raises(ValueError):
        monitor_layout([0], [0], [H + 1], W, H)
    with pytest.raises(ValueError):
        monitor_layout([0], [0], [-1], W, H)


# ------------------------------------------------------------------------------------------------ 2. the two facts
CUTS = (1, 31, 32, 33, 0, 63, 64, 65, 1215, 1216)


def test_chunked_lfilter_with_carried_state_equals_the_whole_row(oracle):
    """SciPy's direct-form-II-transposed loop from carried zi, chunk by chunk, against oracle.lfilter over the whole row (the arithmetic
    the band-pass kernels are pinned to): uint64 view, all four bands."""
    from scipy.signal import lfilter
    from echoseal_amd.tables import pack_tables
    ba = pack_tables()[0]
    rng = np.random.default_rng(1)
    x = (0.1 * rng.standard_normal(6000)).astype(np.float32)
    cuts = list(CUTS) + [6000 - sum(CUTS)]
    for band in range(4):
        b, a = ba[band][:9], ba[band][9:18]
        whole = np.asarray(oracle.lfilter(b, a, x), np.float64)
        zi, parts, at = np.zeros(8), [], 0
        for ln in cuts:
            if ln:                                  # (SciPy does not hand zi back from an empty input: a chunk of 0 samples carries it as it is)
                y, zi = lfilter(b, a, x[at: at + ln].astype(np.float64), zi=zi)
                parts.append(y); at += ln
        assert np.array_equal(np.concatenate(parts).view(np.uint64), whole.view(np.uint64)), band


def test_correlation_of_a_slice_equals_the_slice_of_the_correlation_on_the_19_grid(oracle):
    """oracle.ncc sums a lag's energy in an order that follows the lag's index mod 19 (the kernel's chunk): a slice that starts at a
    multiple of 19 reproduces the whole row's values bit for bit, one that starts at 7 mod 19 does not.  If either kernel's summation
    order changes, this fails before the monitor does."""
    from echoseal_amd.tables import pack_tables
    ba, tpl = pack_tables()[:2]
    rng = np.random.default_rng(2)
    x = (0.1 * rng.standard_normal(6000)).astype(np.float32)
    y = np.asarray(oracle.lfilter(ba[1][:9], ba[1][9:18], x), np.float64)
    corr = np.asarray(oracle.ncc(y, tpl[1][:63]), np.float64)
    for w0 in (19, 608, 1216, 2432):
        assert np.array_equal(np.asarray(oracle.ncc(y[w0:], tpl[1][:63])).view(np.uint64), corr[w0:].view(np.uint64)), w0
    for w0 in (7, 1215):
        assert np.count_nonzero(np.asarray(oracle.ncc(y[w0:], tpl[1][:63])).view(np.uint64) != corr[w0:].view(np.uint64)) > 100, w0


# ------------------------------------------------------------------------------------------------ 3. boundary and refusals
def test_header_declares_and_native_binds_the_entry_points():
    import echoseal_amd._native as nat
    text = open(HEADER).read()
    assert nat.CONSTANTS["ES_ABI_VERSION"] == nat.ES_ABI_VERSION == 2
    assert nat.CONSTANTS["ES_MONITOR_REC_WORDS"] == nat.ES_MONITOR_REC_WORDS
    for name, n in ENTRY_POINTS.items():
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == n == len(nat.DECLARATIONS[name]), name
    for lines in ("rtwm/detector.py:59-60", "rtwm/detector.py:76-79", "rtwm/detector.py:83-99"):
        assert lines in text[text.index("a monitor that verifies many streams"):], lines


def test_python_refusals_need_no_engine():
    from echoseal_amd.detector import LiveMonitor, WatermarkDetector
    from echoseal_amd.monitor import MIN_WINDOW, host_table
    det = WatermarkDetector(b"\x01" * 32, list_size=8)
    with pytest.raises(ValueError, match="at least 2432 samples"):
        det.open_streams(4, window_s=(MIN_WINDOW - 1) / 48_000)
    with pytest.raises(ValueError, match="chunk_max"):
        det.open_streams(4, chunk_max=0)
    mon = LiveMonitor(det, host_table(3, 48_000, 1000))                     # the host half of a table: no device arrays, no engine
    ok = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="fs_target"):
        mon.push([ok], [0], fs=44_100)
    with pytest.raises(ValueError, match="1-D"):
        mon.push([np.zeros((2, 50), np.float32)], [0])
    with pytest.raises(ValueError, match="longer than chunk_max"):
        mon.push([np.zeros(1001, np.float32)], [0])
    with pytest.raises(ValueError, match="named twice"):
        mon.push([ok, ok], [1, 1])
    with pytest.raises(ValueError, match="outside"):
        mon.push([ok], [3])
    with pytest.raises(ValueError, match="one chunk per stream"):
        mon.push([ok], [0, 1])
    assert det._engine is None and len(mon) == 3 and mon.position(0) == 0 and mon.window(0) == (0, 0)


# ------------------------------------------------------------------------------------------------ 4. code objects
def test_new_kernels_use_no_flat_access_no_scratch_no_private_segment(tmp_path):
    found = {}
    for co in code_objects(tmp_path):
        md = kernel_metadata(co)
        mine = {k: v for k, v in md.items() if any(name in k for name in KERNELS)}
        if not mine:
            continue
        dis = disassembly(co)
        for sym, m in mine.items():
            found[sym] = m
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (sym, m)
            ops = dis[sym]
            assert ops and not [op for op in ops if op.startswith("flat_") or op.startswith("scratch_")], sym
    for name in KERNELS:
        assert any(name in sym for sym in found), (name, sorted(found))
    assert sum("es_bpf_stream_kernel" in sym for sym in found) == 2         # int16 and float32
