"""Conditioning a queue of mixed-rate clips without a GPU: the entry point at the boundary (header, binder, exported symbol), the new
kernels' code objects, utils.condition_plan against utils.resample_plan, and a NumPy twin of the kernel's descriptor semantics
(tile-wise incremental (phase, input index) stepping) against scipy.signal.resample_poly, bit for bit."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import resample_poly

from code_objects import LIB, ROOT, _tool, code_objects, kernel_metadata

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
ENTRY_POINTS = {"es_resample_ragged_batch": 13}
NEW_KERNELS = ("es_resample_ragged_kernelIsE", "es_resample_ragged_kernelIfE", "es_resample_ragged_kernelIdE")
RATES = [(44_100, 48_000), (8_000, 48_000), (16_000, 48_000), (32_000, 48_000), (22_050, 48_000), (11_025, 48_000), (96_000, 48_000),
         (192_000, 48_000), (48_000, 44_100)]
LENGTHS = [1, 2, 3, 20, 21, 22, 63, 64, 200]


def test_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    text = open(HEADER).read()
    assert nat.CONSTANTS["ES_ABI_VERSION"] == nat.ES_ABI_VERSION == 2                             # additive: the version stays
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    nm = _tool("llvm-nm") or _tool("nm")
    syms = set(subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split()) if nm else None
    for name, nargs in ENTRY_POINTS.items():
        assert len(nat.DECLARATIONS[name]) == nargs, name
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert hasattr(lib, name), name
        assert syms is None or name in syms, name
    assert "rtwm/utils.py:58-66" in text[text.index("es_resample_ragged_batch") - 3000:]          # cites the reference lines it replaces
    # the ints (dtype, rep) and the 64-bit sizes sit where the header puts them
    args = nat.SIGNATURES["es_resample_ragged_batch"][1]
    assert args[2] is ctypes.c_int and args[8] is ctypes.c_int and all(args[k] is ctypes.c_int64 for k in (3, 5, 7, 10, 11))
    # descriptor width and tile length: header, binder and engine agree
    from echoseal_amd import engine as E
    words, tile = nat.CONSTANTS["ES_RESAMPLE_DESC_WORDS"], nat.CONSTANTS["ES_RESAMPLE_TILE"]
    assert words == nat.ES_RESAMPLE_DESC_WORDS == 8 and tile == nat.ES_RESAMPLE_TILE == E.RESAMPLE_TILE
    assert callable(E.RxEngine.resample_ragged)


def test_new_kernels_use_no_private_memory(tmp_path):
    md = {}
    for co in code_objects(tmp_path):
        md.update(kernel_metadata(co))
    for want in NEW_KERNELS:
        hits = [k for k in md if want in k]
        assert len(hits) == 1, (want, hits)
        m = md[hits[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (want, m)      # nothing goes to memory


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_condition_plan_agrees_with_resample_plan(dtype):
    from echoseal_amd.utils import condition_plan, resample_plan, resampled_length
    ctype = np.float64 if dtype == np.float64 else np.float32
    lengths = [200, 0, 64, 200, 7, 63, 200, 1, 500]
    fs = [44_100, 44_100, 48_000, 44_100, 96_000, 22_050, 88_200, 48_000, 22_050]      # 44.1 kHz three times, 22.05 kHz twice
    cp = condition_plan(lengths, fs, 48_000, dtype)
    assert cp.desc.shape == (len(lengths), 8) and cp.desc.dtype == np.int64 and cp.filters.dtype == ctype
    assert cp.desc[:, 0].tolist() == (np.cumsum(lengths) - lengths).tolist() and cp.desc[:, 1].tolist() == lengths      # back to back, unpadded
    assert cp.n_out.tolist() == cp.desc[:, 7].tolist() == [resampled_length(n, f, 48_000) for n, f in zip(lengths, fs)]
    seen = {}
    for r, (n, f) in enumerate(zip(lengths, fs)):
        plan = resample_plan(n, 48_000, f, ctype)
        off, n_in, up, down, h_off, hpp, y0, n_out = (int(v) for v in cp.desc[r])
        if plan is None:
            assert f == 48_000 and (up, down, hpp, n_out) == (1, 1, 0, n)
            continue
        h_tf, p_hpp, p_up, p_down, p_y0, p_n_out, p_ctype = plan
        assert (up, down, hpp, y0, n_out) == (p_up, p_down, p_hpp, p_y0, p_n_out) and p_ctype == ctype
        assert cp.filters[h_off:h_off + up * hpp].tobytes() == h_tf.tobytes()
        seen.setdefault(h_tf.tobytes(), set()).add(h_off)
    assert all(len(offs) == 1 for offs in seen.values())                     # identical filters appear once ...
    assert cp.filters.size == sum(len(k) for k in seen) // np.dtype(ctype).itemsize      # ... and nothing else is in the pool
    assert len(seen) < sum(f != 48_000 for f in fs)                         # (the records above do share filters)
    one = condition_plan([5, 6], 44_100, 48_000, dtype)                      # one rate for all
    assert one.desc[:, 2].tolist() == [160, 160] and one.desc[0, 4] == one.desc[1, 4]
    none = condition_plan([], [], 48_000, dtype)
    assert none.desc.shape == (0, 8) and none.filters.size == 0 and none.n_out.size == 0
    with pytest.raises(ValueError):
        condition_plan([3], [44_100, 48_000], 48_000, dtype)
    with pytest.raises(ValueError):
        condition_plan([-1], [44_100], 48_000, dtype)
    with pytest.raises(ValueError):
        condition_plan([3], [44_100], 48_000, np.int32)


def kernel_twin(pool, filters, desc, rep, out, tile):
    """What es_resample_ragged_kernel does with one descriptor table, in NumPy scalars: per record and tile the first output's (phase,
    input index) from 64-bit integers, then (down mod up, down div up) added with a carry; per output the products of the record's own
    samples in ascending input index, multiply and add rounded separately in the filters' type; float32 on store; rows r * rep + c."""
    T = filters.dtype.type
    stride = out.shape[1]
    for r, (off, n_in, up, down, h_off, hpp, y0, n_out) in enumerate(desc.tolist()):
        n_out = min(n_out, stride)
        x = pool[off:off + n_in]
        for k0 in range(0, n_out, tile):
            cnt = min(tile, n_out - k0)
            if up == down:
                vals = x[k0:k0 + cnt].astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x[k0:k0 + cnt].astype(np.float32)
            else:
                yy = y0 + k0
                p, xi = (yy * down) % up, (yy * down) // up                 # once per tile
                dm, dq = down % up, down // up
                vals = np.zeros(cnt, np.float32)
                for k in range(cnt):
                    lo, hi = max(xi - hpp + 1, 0), min(xi, n_in - 1)
                    hidx = h_off + p * hpp + (lo - (xi - hpp + 1))
                    acc = T(0)
                    for i in range(lo, hi + 1):
                        s = T(np.float32(x[i]) / np.float32(32768)) if x.dtype == np.int16 else T(x[i])
                        acc = T(acc + T(s * filters[hidx]))
                        hidx += 1
                    vals[k] = np.float32(acc)
                    p += dm; xi += dq
                    if p >= up:
                        p -= up; xi += 1
            for c in range(rep):
                out[r * rep + c, k0:k0 + cnt] = vals


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_numpy_twin_of_the_kernel_equals_scipy(dtype):
    from echoseal_amd.utils import condition_plan
    rng = np.random.default_rng(12)
    clips, fs, targets = [], [], []
    for fs_in, fs_out in RATES:
        for n in LENGTHS:
            x = rng.standard_normal(n) * 0.3
            clips.append(np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16) if dtype == np.int16 else x.astype(dtype))
            fs.append(fs_in); targets.append(fs_out)
    hpps = set()
    for fs_out in (48_000, 44_100):
        sel = [i for i, t in enumerate(targets) if t == fs_out]
        sub = [clips[i] for i in sel]
        cp = condition_plan([c.size for c in sub], [fs[i] for i in sel], fs_out, dtype)
        hpps |= set(cp.desc[:, 5].tolist())
        sentinel = np.float32(-7.25)
        for rep, tile in ((1, 1024), (2, 16)):                              # (a short tile: several tiles per record at these lengths)
            out = np.full((len(sub) * rep, int(cp.n_out.max()) + 3), sentinel, np.float32)
            with np.errstate(all="ignore"):
                kernel_twin(np.concatenate(sub), cp.filters, cp.desc, rep, out, tile)
            for r, (c, f) in enumerate(zip(sub, [fs[i] for i in sel])):
                g = math.gcd(f, fs_out)
                src = c.astype(np.float32) / np.float32(32768) if dtype == np.int16 else c
                ref = resample_poly(src, fs_out // g, f // g).astype(np.float32)
                assert ref.size == cp.n_out[r]
                for k in range(rep):
                    row = out[r * rep + k]
                    assert np.array_equal(row[:ref.size].view(np.uint8), ref.view(np.uint8)), (dtype, f, c.size, rep, tile)
                    assert (row[ref.size:] == sentinel).all()
    assert hpps == {21, 43, 85, 23}


# ---------------------------------------------------------------------------------- the kernel's arms and limits, without a GPU
def test_kernel_constants_equal_header_binder_and_the_tests_mirror():
    """RS_WIN_MAX, RS_FILT_MAX and RS_RATE_MAX decide which arm a tile takes and which record is refused: the numbers in es_resample.hip,
    include/echoseal_hip.h, _native.py and tests/resample_arms.py are the same, so a change of one cannot silently empty an arm of
    tests/test_gpu_resample_arms.py or move the host's limit away from the kernel's."""
    import echoseal_amd._native as nat
    import resample_arms as A
    kernel = open(os.path.join(ROOT, "echoseal_amd", "csrc", "es_resample.hip")).read()
    value = lambda s: eval(s, {"__builtins__": {}})                          # "4352", "1 << 20"
    k = {n: value(re.search(r"constexpr\s+int\s+RS_" + n + r"\s*=\s*([0-9<\s]+);", kernel).group(1)) for n in ("WIN_MAX", "FILT_MAX", "RATE_MAX")}
    h = {n: nat.CONSTANTS["ES_RESAMPLE_" + n] for n in ("WIN_MAX", "FILT_MAX", "RATE_MAX", "TABLE_MAX", "TILE")}
    assert k == {"WIN_MAX": A.WIN_MAX, "FILT_MAX": A.FILT_MAX, "RATE_MAX": A.RATE_MAX} == {n: h[n] for n in k} == {"WIN_MAX": 4352, "FILT_MAX": 3584, "RATE_MAX": 1 << 20}
    assert (nat.ES_RESAMPLE_WIN_MAX, nat.ES_RESAMPLE_FILT_MAX, nat.ES_RESAMPLE_RATE_MAX, nat.ES_RESAMPLE_TABLE_MAX) == (h["WIN_MAX"], h["FILT_MAX"], h["RATE_MAX"], h["TABLE_MAX"])
    assert h["TILE"] == A.TILE == nat.ES_RESAMPLE_TILE and re.search(r"constexpr\s+int\s+RS_TILE\s*=\s*ES_RESAMPLE_TILE\s*;", kernel)
    # the table limit is a literal in the kernel's refusal, and the arms are chosen by exactly these two comparisons
    assert h["TABLE_MAX"] == 1 << 30 and "up_l * hpp_l > (1ll << 30)" in kernel
    assert "x_lds = span <= RS_WIN_MAX, h_lds = up * hpp <= RS_FILT_MAX" in kernel
    assert "span = ((long long)(cnt - 1) * down + t0) / up + hpp" in kernel and "t0 = (int)(((yy % up) * down) % up)" in kernel


def test_arm_records_reach_every_arm_at_both_tile_positions():
    """The launch of tests/test_gpu_resample_arms.py, classified tile by tile with the kernel's formulas: all four arms, each with k0 == 0 and
    with k0 > 0; every rate pair's full tiles take the arm the pair is there for, and the threshold records lie on either side."""
    import resample_arms as A
    recs = A.records()
    desc, filters = A.descriptors(recs, np.float32)
    seen = A.coverage(desc)
    assert set(seen) == A.ALL_ARMS, sorted(A.ALL_ARMS - set(seen))
    assert (desc[:, 4] + desc[:, 2] * desc[:, 5] <= filters.size).all() and filters.size < 1_300_000 and desc[:, 1].max() < 25_000
    arms_of = lambda fi, fo, full=True: {t[4] for r, row in zip(recs, desc) if r[1:] == (fi, fo) for t in A.tiles(row) if t[1] == A.TILE or not full}
    for pair, arm in zip(A.PAIRS, [A.ARMS[2]] * 2 + [A.ARMS[3]] * 2 + [A.ARMS[1]] * 4 + [A.ARMS[0]] * 2):
        assert arms_of(*pair) == {arm}, pair                                 # every FULL tile of the pair takes the arm it is there for
    # a record of 2 * TILE + 1 or 3 * TILE + 5 outputs of a window-global pair ends in a short tile with its window in LDS: arms mix
    for pair in A.PAIRS[:4]:
        assert len(arms_of(*pair, full=False)) == 2, pair
    by_pair = lambda fi, fo: [row for r, row in zip(recs, desc) if r[1:] == (fi, fo)]
    assert [int(row[7]) for row in by_pair(384_000, 48_000)] == A.N_OUTS and all(row[2] == 1 for row in by_pair(384_000, 48_000))
    assert max(len(A.tiles(row)) for row in by_pair(47_999, 48_000)) >= 3 and by_pair(47_999, 48_000)[0][2] == 48_000
    assert [int(t[2]) for row in by_pair(192_000, 48_000) for t in A.tiles(row) if t[1] == A.TILE][0] == 4177      # what RS_WIN_MAX was sized for
    # the two records on either side of RS_WIN_MAX (single tiles of 352.8 -> 48 kHz) and the two pairs on either side of RS_FILT_MAX
    lo, hi = A.window_threshold()
    s_lo, s_hi = A.single_tile_span(lo, 352_800, 48_000), A.single_tile_span(hi, 352_800, 48_000)
    assert hi == lo + 1 < A.TILE and s_lo <= A.WIN_MAX < s_hi and A.single_tile_span(lo - 1, 352_800, 48_000) <= s_lo
    assert {int(row[7]) for row in by_pair(352_800, 48_000)} >= {lo, hi}
    below, above = A.table_threshold()
    size = lambda pair: {int(row[2] * row[5]) for row in by_pair(*pair)}
    assert max(size(below)) <= A.FILT_MAX < min(size(above)) and min(size(above)) - max(size(below)) < 64
    assert all(len(A.tiles(row)) == 2 for row in by_pair(*below) + by_pair(*above))
    assert recs[-1][1:] == A.SMALL_PAIR and {t[4] for t in A.tiles(desc[-1])} == {A.ARMS[3]}


def test_resample_geometry_is_resample_plan_without_the_filter():
    from echoseal_amd.utils import resample_geometry, resample_plan
    rng = np.random.default_rng(3)
    pairs = [(int(u), int(d)) for u, d in rng.integers(1, 700, (300, 2))] + [(160, 147), (147, 160), (1, 8), (441, 2000), (640, 147), (6000, 5507)]
    for up, down in pairs:
        for n in (0, 1, 2, 17, 64, 1000, int(rng.integers(1, 5000))):
            plan, geo = resample_plan(n, up, down, np.float32), resample_geometry(n, up, down)
            if plan is None:
                assert geo is None and up == down
            else:
                assert geo == (plan[2], plan[3], plan[1], plan[4], plan[5]), (n, up, down)


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_condition_plan_refuses_what_the_kernel_would_leave_unwritten(dtype, monkeypatch):
    """A record whose reduced up, down or taps per phase exceed 2^20, or whose table exceeds 2^30 values, makes the kernel write nothing.
    condition_plan refuses it by name BEFORE any filter is designed (1 048 583 is coprime to 48 000: a 21-million-tap firwin otherwise)."""
    import scipy.signal
    from echoseal_amd.utils import condition_plan, resample_limits

    def no_design(*a, **k):
        raise AssertionError("a filter was designed for a clip that is refused")
    assert math.gcd(1_048_583, 48_000) == 1 and 1_048_583 > 1 << 20
    ok = condition_plan([10, 10], [1 << 20, 384_000], 48_000, dtype)         # down = 2^20 / 128: inside
    assert ok.desc[0, 3] == 8192
    monkeypatch.setattr(scipy.signal, "firwin", no_design)
    with pytest.raises(ValueError, match=r"clip 0 \(1048583 Hz -> 48000 Hz\)"):
        condition_plan([10], [1_048_583], 48_000, dtype)
    with pytest.raises(ValueError, match=r"clip 2 \(48000 Hz -> 1048583 Hz\)"):
        condition_plan([10, 10, 5], [1_048_583, 1_048_583, 48_000], 1_048_583, dtype)      # up too large; the clips at the target rate pass
    with pytest.raises(ValueError, match=r"clip 1 \(1048575 Hz -> 1 Hz\).*taps per phase"):
        condition_plan([10, 10], [1, 1_048_575], 1, dtype)                   # up 1, down < 2^20, but 20 * down + 1 taps in one phase
    # (a table above 2^30 values cannot come from a plan inside the other limits: up * hpp is about 20 * max(up, down); the kernel's
    # own check guards against descriptors from elsewhere)
    assert resample_limits(10, 44_100, 48_000) is None and resample_limits(0, 192_000, 44_100) is None and resample_limits(7, 48_000, 48_000) is None
    assert "above 1048576" in resample_limits(10, 1_048_583, 48_000)


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_numpy_twin_equals_scipy_at_the_arm_rate_pairs(dtype):
    """The twin at the rate pairs of tests/test_gpu_resample_arms.py (falling rates with long phases, up to 48 000 phases, the two pairs
    around RS_FILT_MAX), in tiles of 16 outputs, and the record of subnormal products and signed zeros at its full size in one tile of
    1 024: the reference alone passes what the GPU test asks of the kernel."""
    import resample_arms as A
    from echoseal_amd.utils import condition_plan
    rng = np.random.default_rng(21)
    pairs = A.PAIRS + list(A.table_threshold())
    lengths = {p: [1, 3, 22, 93, 200] for p in pairs}
    lengths[(47_999, 48_000)] = [1, 93]                                     # (each length designs the 960 001-tap filter again)
    lengths[(11_025, 48_000)] = lengths[(22_050, 48_000)] = [1, 3, 22, 93]
    recs = [(n, fi, fo) for (fi, fo) in pairs for n in lengths[(fi, fo)]]
    clips = []
    for n, _, _ in recs:
        x = rng.standard_normal(n) * 0.3
        clips.append(np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16) if dtype == np.int16 else x.astype(dtype))
    tile = 16
    if dtype != np.int16:
        recs.append((A.n_in_for(A.TILE, *A.SMALL_PAIR), *A.SMALL_PAIR))
        clips.append(A.small_products_clip(dtype, recs[-1][0], rng))
    sentinel = np.float32(-7.25)
    hpps = set()
    for fs_out in sorted({r[2] for r in recs}):
        sel = [i for i, r in enumerate(recs) if r[2] == fs_out]
        sub, fs = [clips[i] for i in sel], [recs[i][1] for i in sel]
        cp = condition_plan([c.size for c in sub], fs, fs_out, dtype)
        hpps |= set(cp.desc[:, 5].tolist())
        small = [r for r, c in enumerate(sub) if c.size > 1000]
        for rows, tl in ((list(set(range(len(sub))) - set(small)), tile), (small, A.TILE)):
            if not rows:
                continue
            desc = cp.desc[rows]
            out = np.full((len(rows), int(desc[:, 7].max()) + 3), sentinel, np.float32)
            with np.errstate(all="ignore"):
                kernel_twin(np.concatenate(sub), cp.filters, desc, 1, out, tl)
            for k, r in enumerate(rows):
                g = math.gcd(fs[r], fs_out)
                src = sub[r].astype(np.float32) / np.float32(32768) if dtype == np.int16 else sub[r]
                ref = resample_poly(src, fs_out // g, fs[r] // g).astype(np.float32)
                assert ref.size == desc[k, 7]
                assert np.array_equal(out[k, :ref.size].view(np.uint8), ref.view(np.uint8)), (dtype, fs[r], fs_out, sub[r].size, tl)
                assert (out[k, ref.size:] == sentinel).all()
                if r in small:                                              # the products ARE subnormal, and something came of them
                    h = cp.filters[desc[k, 4]:desc[k, 4] + desc[k, 2] * desc[k, 5]]
                    assert np.abs(sub[r]).max() * np.abs(h).max() < np.finfo(dtype).tiny and (ref.any() or dtype == np.float64)
                    assert np.signbit(ref).any() and not np.signbit(ref).all()
    assert {169, 155, 92, 96, 85, 78} <= hpps and len(recs) > 50
