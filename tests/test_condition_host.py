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
    assert re.search(r"#define\s+ES_ABI_VERSION\s+2\b", text) and nat.ES_ABI_VERSION == 2        # additive: the version stays
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build())"
    lib = ctypes.CDLL(LIB)
    nm = _tool("llvm-nm") or _tool("nm")
    syms = set(subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split()) if nm else None
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == nargs, name
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
    words = int(re.search(r"#define\s+ES_RESAMPLE_DESC_WORDS\s+(\d+)", text).group(1))
    tile = int(re.search(r"#define\s+ES_RESAMPLE_TILE\s+(\d+)", text).group(1))
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
