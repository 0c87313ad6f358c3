"""Live streams at other rates without a GPU: the prefix property of resample_poly the chunked resampler rests on, pinned
against SciPy; a NumPy restatement of the stream kernel's two-source window and commit rule; the arms the GPU test's records take; the C
ABI at the boundary; the Python refusals; the new kernels' code objects."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.signal import resample_poly

import stream_resample_cases as C
from code_objects import ROOT, code_objects, kernel_metadata
from echoseal_amd.utils import finalized, resample_geometry, resample_plan, stream_resample_plan

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
KERNELS = ("es_resample_stream_kernel", "es_resample_commit_kernel", "es_resample_ragged_kernel")


def _stream(rng, n):
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x[::13] = -0.0
    x[5::17] = 0.0
    return x


# ------------------------------------------------------------------------------------------------ 1. the fact
@pytest.mark.parametrize("fs_in,fs_target", C.FACT_PAIRS)
def test_finalized_prefix_of_resample_poly_never_changes(fs_in, fs_target):
    """resample_poly(X[:n])[:F(n)] equals resample_poly(X[:n'])[:F(n)] in the uint32 view for n' > n, output F(n) is the first whose
    newest input has not arrived, and at most y0 outputs are held back."""
    pl = stream_resample_plan(fs_in, fs_target)
    up, down, y0 = pl.up, pl.down, pl.y0
    assert (up, down, y0) == (resample_geometry(1000, fs_target, fs_in)[0], resample_geometry(1000, fs_target, fs_in)[1], resample_geometry(1000, fs_target, fs_in)[3])
    x = _stream(np.random.default_rng(fs_in), 1400)
    whole = resample_poly(x, up, down)
    assert whole.dtype == np.float32
    assert finalized(0, up, down, y0) == 0
    assert finalized(np.array(C.FACT_CUTS), up, down, y0).tolist() == [finalized(n, up, down, y0) for n in C.FACT_CUTS]
    for n in C.FACT_CUTS:
        f = finalized(n, up, down, y0)
        part = resample_poly(x[:n], up, down)
        assert 0 <= part.size - f <= y0 and part.size == -(-n * up // down), (n, f, part.size)
        assert np.array_equal(part[:f].view(np.uint32), whole[:f].view(np.uint32)), n
        for n2 in (n + 1, n + 7, n + 200):
            assert np.array_equal(resample_poly(x[:n2], up, down)[:f].view(np.uint32), whole[:f].view(np.uint32)), (n, n2)
        # F(n) is exact: output F(n) - 1 has its newest input, output F(n) does not
        if f:
            assert ((y0 + f - 1) * down) // up <= n - 1
        assert ((y0 + f) * down) // up > n - 1


def test_canonical_table_is_resample_plans_without_the_zero_taps_it_appends():
    for fs_in, fs_target in C.FACT_PAIRS + list(C.GPU_PAIRS):
        pl = stream_resample_plan(fs_in, fs_target)
        for n_in in (1, 50, 5000):
            h_tf, hpp, up, down, y0, _, ct = resample_plan(n_in, fs_target, fs_in, np.float32)
            assert (up, down, y0, ct) == (pl.up, pl.down, pl.y0, np.float32) and hpp >= pl.hpp and pl.h_tf.dtype == np.float32
            full = h_tf.reshape(up, hpp)
            assert np.array_equal(full[:, hpp - pl.hpp:].view(np.uint32), pl.h_tf.reshape(up, pl.hpp).view(np.uint32))
            assert not full[:, :hpp - pl.hpp].any()
    same = stream_resample_plan(48_000, 48_000)
    assert (same.up, same.down, same.y0, same.hpp, same.h_tf.size) == (1, 1, 0, 0, 0)


@pytest.mark.parametrize("fs_in,fs_target", C.FACT_PAIRS)
@pytest.mark.parametrize("dtype", [np.float32, np.int16])
def test_tail_and_chunk_staging_with_the_commit_rule_equals_the_whole_stream(fs_in, fs_target, dtype):
    """The stream kernel in NumPy over the cuts 1, 1, hpp - 2, hpp - 1, hpp, 0, 300 and the rest: what every push returns is
    resample_poly(whole)[F(n_old) : F(n_new)]."""
    pl = stream_resample_plan(fs_in, fs_target)
    cuts = [1, 1, pl.hpp - 2, pl.hpp - 1, pl.hpp, 0, 300]
    x = _stream(np.random.default_rng(fs_in + 1), sum(cuts) + 180)
    if dtype == np.int16:
        x = np.clip(np.round(x.astype(np.float64) * 20000), -32768, 32767).astype(np.int16)
        whole = resample_poly(x.astype(np.float32) / np.float32(32768), pl.up, pl.down)
    else:
        whole = resample_poly(x, pl.up, pl.down)
    cuts.append(x.size - sum(cuts))
    (tail, n), got = C.fresh_state(), []
    for ln in cuts:
        out, tail, n2 = C.stream_step(pl, tail, n, x[n:n + ln])
        assert n2 == n + ln and out.size == finalized(n2, pl.up, pl.down, pl.y0) - finalized(n, pl.up, pl.down, pl.y0)
        got.append(out); n = n2
    got = np.concatenate(got)
    assert n == x.size and got.size == finalized(n, pl.up, pl.down, pl.y0) > 0
    assert np.array_equal(got.view(np.uint32), whole[:got.size].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. arms
def test_gpu_streams_meet_all_four_arms_at_first_and_later_tiles():
    streams = [(fi, fo, C.gpu_cuts(fi, fo)) for fi, fo in C.GPU_PAIRS]
    assert C.coverage(streams).keys() == C.ALL_ARMS
    for (fi, fo), arm in C.GPU_PAIRS.items():
        pl, plan = stream_resample_plan(fi, fo), C.gpu_plan(fi, fo)
        assert [ln for ln, _ in plan[:6]] == [1, 1, pl.hpp - 2, pl.hpp - 1, pl.hpp, 0] and pl.hpp <= C.TAIL
        assert [w for _, w in plan if w is not None] == list(C.EXACT_COUNTS) + [C.REST_OUTPUTS]
        n = 0
        for ln, want in plan:
            got = finalized(n + ln, pl.up, pl.down, pl.y0) - finalized(n, pl.up, pl.down, pl.y0)
            if want is not None:
                # exactly, but for 8 -> 48 kHz, where F grows in sixes: there the next multiple of six
                assert got == want if (fi, fo) != (8_000, 48_000) else (want <= got < want + 6 and got % 6 == 0), (fi, fo, want, got)
                full = [t for t in C.tiles(n, ln, pl) if t[1] == C.TILE]
                assert (full or want < C.TILE) and all(t[4] == arm for t in full), (fi, fo, want)
            n += ln
    kernel = open(os.path.join(ROOT, "echoseal_amd", "csrc", "es_resample.hip")).read()
    import echoseal_amd._native as nat
    assert (C.TILE, C.WIN_MAX, C.FILT_MAX, C.TAIL) == (nat.ES_RESAMPLE_TILE, nat.ES_RESAMPLE_WIN_MAX, nat.ES_RESAMPLE_FILT_MAX, nat.ES_RSTREAM_TAIL)
    assert re.search(r"constexpr\s+int\s+RS_WIN_MAX\s*=\s*%d\s*;" % C.WIN_MAX, kernel) and re.search(r"constexpr\s+int\s+RS_FILT_MAX\s*=\s*%d\s*;" % C.FILT_MAX, kernel)


# ------------------------------------------------------------------------------------------------ 3. boundary
def test_header_declares_and_native_binds_the_entry_point():
    import echoseal_amd._native as nat
    text = open(HEADER).read()
    assert re.search(r"#define\s+ES_ABI_VERSION\s+2\b", text) and nat.ES_ABI_VERSION == 2
    m = re.search(r"\bint\s+es_resample_stream_batch\s*\(([^;]*)\)\s*;", text)
    res, args = nat.SIGNATURES["es_resample_stream_batch"]
    assert m and res is ctypes.c_int and len(args) == 17 == len([a for a in m.group(1).split(",") if a.strip()])
    for name, val in (("REC_WORDS", nat.ES_RSTREAM_REC_WORDS), ("RATE_WORDS", nat.ES_RSTREAM_RATE_WORDS), ("TAIL", nat.ES_RSTREAM_TAIL)):
        assert re.search(r"#define\s+ES_RSTREAM_%s\s+%d\b" % (name, val), text), name
    doc = text[text.index("live streams that arrive chunk by chunk"):text.index("int es_resample_stream_batch")]
    assert "rtwm/utils.py:58-66" in doc and "F(n) = max(0, (n up - 1) / down - y0 + 1)" in doc


class _HostEngine:
    """What WatermarkDetector asks of an engine to open a monitor, with the host half of the table only."""
    fs, list_size_max = 48_000, 32

    def open_monitor(self, n, *, window, chunk_max, bands, fs=None):
        from echoseal_amd.monitor import host_table
        return host_table(n, window, chunk_max, bands=bands, fs=fs, fs_target=self.fs)


def test_python_refusals_and_rates_need_no_engine():
    from echoseal_amd.detector import LiveMonitor, WatermarkDetector
    from echoseal_amd.monitor import host_table
    det = WatermarkDetector(b"\x01" * 32, list_size=8)
    with pytest.raises(ValueError, match="1000000 Hz"):
        det.open_streams(2, fs=1_000_000)                                   # hpp = 6 001 > 256
    with pytest.raises(ValueError, match="1000000 Hz"):
        stream_resample_plan(1_000_000, 48_000)
    with pytest.raises(ValueError, match="3 Hz"):
        stream_resample_plan(3, 48_000 * 1024 + 1)                          # what resample_limits refuses: up above 2^20
    with pytest.raises(ValueError, match="2 rates for 4 streams"):
        det.open_streams(4, fs=[44_100, 8_000])
    assert det._engine is None
    assert stream_resample_plan(384_000, 48_000).hpp == 169
    # accepted: rates per stream, the table's host half
    det._engine = _HostEngine()
    mon = det.open_streams(4, fs=[44_100, 8_000, 48_000, 96_000], chunk_max=1000)
    assert isinstance(mon, LiveMonitor) and [mon.rate(s) for s in range(4)] == [44_100, 8_000, 48_000, 96_000]
    assert [mon.received(s) for s in range(4)] == [0] * 4 and [mon.position(s) for s in range(4)] == [0] * 4
    assert mon.table.rs.rate_host.tolist() == [[160, 147, 0, 21, 11], [6, 1, 3360, 21, 61], [1, 1, 0, 0, 0], [1, 2, 3486, 43, 11]]
    ok = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="stream 0 was opened at 44100 Hz"):
        mon.push([ok], [0], fs=48_000)
    with pytest.raises(ValueError, match="stream 2 was opened at 48000 Hz"):
        mon.push([ok, ok], [0, 2], fs=44_100)
    with pytest.raises(ValueError, match="finalizes 1089 samples at 48000 Hz, more than chunk_max = 1000"):
        mon.push([np.zeros(1010, np.float32)], [0])                         # 44.1 kHz: F(1010) = 1089
    with pytest.raises(ValueError, match="finalizes 1139 samples"):
        mon.push([np.zeros(200, np.float32)], [1])                          # 8 kHz: 6 * 200 - 61
    with pytest.raises(ValueError, match="longer than chunk_max"):
        mon.push([np.zeros(1001, np.float32)], [2])                         # at fs_target a chunk counts as it is
    with pytest.raises(ValueError, match="named twice"):
        mon.push([ok, ok], [1, 1], fs=8_000)
    assert [mon.received(s) for s in range(4)] == [0] * 4                   # nothing moved
    # a monitor whose streams are all at fs_target still names fs_target
    plain = LiveMonitor(det, host_table(3, 48_000, 1000))
    with pytest.raises(ValueError, match="fs_target = 48000"):
        plain.push([ok], [0], fs=44_100)
    assert plain.rate(1) == 48_000 and plain.received(1) == 0
    with pytest.raises(ValueError, match="needs fs_target"):
        host_table(2, 48_000, 1000, fs=44_100)
    # a refused add leaves the table as it was: no resampler half appears on a monitor whose streams are all at fs_target
    from echoseal_amd.monitor import MonitorChain
    before = (plain.table.rs, plain.table.fs_target, plain.table.n, plain.table.live.copy())
    with pytest.raises(ValueError, match="1000000 Hz"):
        MonitorChain.add_monitor_streams(_HostEngine(), plain.table, 1, fs=1_000_000)
    with pytest.raises(ValueError, match="2 rates for 1 streams"):
        MonitorChain.add_monitor_streams(_HostEngine(), plain.table, 1, fs=[44_100, 8_000])
    assert (plain.table.rs, plain.table.fs_target, plain.table.n) == before[:3] and plain.table.rs is None and (plain.table.live == before[3]).all()
    with pytest.raises(ValueError, match="fs_target = 48000"):
        plain.push([ok], [0], fs=44_100)                                    # ... and push(fs=) words its refusal as before
    rs_before = (mon.table.rs.n, dict(mon.table.rs.offsets), mon.table.rs.filters.size)
    with pytest.raises(ValueError, match="1000000 Hz"):
        MonitorChain.add_monitor_streams(_HostEngine(), mon.table, 2, fs=[16_000, 1_000_000])
    assert (mon.table.rs.n, dict(mon.table.rs.offsets), mon.table.rs.filters.size) == rs_before


def test_host_counts_follow_the_mirror():
    from echoseal_amd.monitor import resample_counts, resampler_host
    rt = resampler_host([44_100, 8_000, 48_000], 48_000)
    ids = np.array([0, 1, 2])
    f_old, cnt = resample_counts(rt, ids, np.array([10, 10, 10]))
    assert f_old.tolist() == [0, 0, 0] and cnt.tolist() == [finalized(10, 160, 147, 11), 0, 10] == [0, 0, 10]
    rt.n_in_host[:] = [1000, 1000, 1000]
    f_old, cnt = resample_counts(rt, ids, np.array([882, 1, 0]))
    assert f_old.tolist() == [finalized(1000, 160, 147, 11), 6 * 1000 - 61, 1000] and cnt.tolist() == [960, 6, 0]
    rt.n_in_host[0] = (1 << 62) // 160
    with pytest.raises(ValueError, match="44100 Hz.*2\\^62"):
        resample_counts(rt, ids[:1], np.array([1]))


# ------------------------------------------------------------------------------------------------ 4. code objects
def test_new_kernels_have_no_private_segment_and_no_spills(tmp_path):
    """Code-object metadata only: no private segment (so no scratch) and no spilled vector register in the stream, commit and ragged
    kernels, and the instantiations that are expected."""
    found = {}
    for co in code_objects(tmp_path):
        for sym, m in kernel_metadata(co).items():
            if any(name in sym for name in KERNELS):
                found[sym] = m
                assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (sym, m)
    assert sum("es_resample_stream_kernel" in sym for sym in found) == 2 == sum("es_resample_commit_kernel" in sym for sym in found)      # int16 and float32
    assert sum("es_resample_ragged_kernel" in sym for sym in found) == 3
