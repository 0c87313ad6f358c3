"""The level mix without a GPU: the host WatermarkEmbedder.process pinned to outputs captured from the reference
(tests/golden/embed_mix.npz, tools/gen_golden_embed.py), the summation order the HIP kernel (es_mix.hip) rests on checked against
this NumPy, and es_mix_batch at the boundary (header, binder, exported symbol)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from code_objects import LIB, ROOT, _tool

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "embed_mix.npz")


def golden_cases():
    g = np.load(GOLDEN)
    for i in range(int(g["count"])):
        t = f"case{i}"
        yield (g["key"].tobytes(), int(g[f"{t}/block"]), int(g[f"{t}/ctr0"]), g[f"{t}/x"], g[f"{t}/payloads"], g[f"{t}/y"],
               int(g[f"{t}/ctr_end"]))


def host_embedder(key, ctr0, payloads):
    """A host embedder that starts at counter ctr0 and replays `payloads`, one per generated frame."""
    from echoseal_amd.embedder import WatermarkEmbedder
    tx = WatermarkEmbedder(key)
    tx.frame_ctr = ctr0
    it = iter(payloads)
    tx._build_payload = lambda: bytes(next(it))
    return tx


def host_process(tx, x, block):
    with np.errstate(all="ignore"):
        return np.concatenate([tx.process(x[s:s + block]) for s in range(0, x.size, block)])


def test_host_process_reproduces_the_reference_bit_for_bit():
    seen = set()
    for key, block, ctr0, x, payloads, y, ctr_end in golden_cases():
        tx = host_embedder(key, ctr0, payloads)
        mine = host_process(tx, x, block)
        assert mine.dtype == np.float32 and mine.tobytes() == y.tobytes(), block
        assert tx.frame_ctr == ctr_end
        seen.add(block)
        changed = y != x
        assert changed[:block].all()                      # digital silence carries the watermark at the floor
        assert not changed[-(x.size % block):].any()      # the clipping end is left alone (scale = 0)
    assert seen == {1024, 480, 1215, 9000}


def test_fixture_exercises_every_branch_of_the_gain():
    """floor, RMS-proportional gain, headroom limit, scale = 0, a NaN block and a block with an infinity all occur."""
    from echoseal_amd.utils import db_to_lin
    kinds = set()
    for key, block, ctr0, x, payloads, y, _ in golden_cases():
        for s in range(0, x.size, block):
            xb, yb = x[s:s + block], y[s:s + block]
            if np.isnan(xb).any():
                assert np.isnan(yb).all(); kinds.add("nan"); continue
            if np.isinf(xb).any():
                assert yb.tobytes() == xb.tobytes(); kinds.add("inf"); continue
            mx = float(np.max(np.abs(xb)))
            rms = float(np.sqrt(np.mean(xb * xb)) + 1e-12)
            if mx >= 0.98:
                assert yb.tobytes() == xb.tobytes(); kinds.add("zero")
            elif db_to_lin(-10.0) * rms <= db_to_lin(-35.0):
                kinds.add("floor")
            elif (yb != xb).any():
                kinds.add("rms-or-headroom")
    assert kinds == {"nan", "inf", "zero", "floor", "rms-or-headroom"}


# ---------------------------------------------------------------------------------------------- NumPy's float32 summation order
def pairwise_f32(a):
    """One ufunc inner-loop call of float32 add.reduce over `a` (at most one buffer of 8192 elements)."""
    n = a.size
    if n < 8:
        res = np.float32(-0.0)
        for v in a:
            res = np.float32(res + v)
        return res
    if n <= 128:
        r = a[:8].copy()
        n8 = n - n % 8
        for i in range(8, n8, 8):
            r += a[i:i + 8]                               # eight independent float32 accumulators
        res = np.float32(np.float32(np.float32(r[0] + r[1]) + np.float32(r[2] + r[3])) + np.float32(np.float32(r[4] + r[5]) + np.float32(r[6] + r[7])))
        for v in a[n8:]:
            res = np.float32(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return np.float32(pairwise_f32(a[:n2]) + pairwise_f32(a[n2:]))


def sum_f32_model(a):
    total = np.float32(0.0)
    for s in range(0, a.size, 8192):
        total = np.float32(total + pairwise_f32(a[s:s + 8192]))
    return total


def split_depth(n):
    if n <= 128:
        return 0
    n2 = (n // 2) & ~7
    return 1 + max(split_depth(n2), split_depth(n - n2))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 127, 128, 129, 1024, 8191, 8192, 8193, 16_385, 240_000])
def test_sum_order_model_equals_numpy(n):
    """The order es_mix.hip sums in IS np.add.reduce's on float32: if another NumPy sums differently this fails, and the kernel's
    promise (bit-identical to the host process()) has to be re-derived."""
    for seed in range(5):
        rng = np.random.default_rng(1000 * n + seed)
        a = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)
        a = a * a
        want = np.add.reduce(a)
        assert sum_f32_model(a).tobytes() == want.tobytes(), (n, seed)
        assert np.mean(a).tobytes() == np.float32(np.float64(want) / n).tobytes(), (n, seed)      # the count divides in float64


def test_split_tree_of_a_chunk_is_at_most_seven_deep():
    """es_mix_block_kernel lays the split tree of a chunk out as a binary heap of 255 nodes."""
    assert max(split_depth(n) for n in range(1, 8193)) == 7


# ---------------------------------------------------------------------------------------------- the boundary
def _decl_args(text, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_header_binder_and_library_agree_on_es_mix_batch():
    import echoseal_amd._native as nat
    text = open(HEADER).read()
    assert re.search(r"#define\s+ES_ABI_VERSION\s+2\b", text) and nat.ES_ABI_VERSION == 2
    assert _decl_args(text, "es_mix_batch") == 13
    assert "rtwm/embedder.py:44-75" in text
    res, args = nat.SIGNATURES["es_mix_batch"]
    assert res is ctypes.c_int and len(args) == 13
    assert args[8] is ctypes.c_double and args[9] is ctypes.c_double and args[4] is ctypes.c_int
    assert os.path.exists(LIB), "build the HIP library first (__graft_entry__.build())"
    assert hasattr(ctypes.CDLL(LIB), "es_mix_batch")
    nm = _tool("llvm-nm") or _tool("nm")
    if nm:
        syms = set(subprocess.run([nm, "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout.split())
        assert "es_mix_batch" in syms


def test_host_layer_offers_the_feature():
    from echoseal_amd.embedder import WatermarkEmbedder
    from echoseal_amd.engine import EmbedResult, RxEngine
    import rtwm.embedder
    assert callable(RxEngine.mix) and callable(RxEngine.embed) and callable(WatermarkEmbedder.embed)
    assert rtwm.embedder.WatermarkEmbedder is WatermarkEmbedder
    assert [f for f in EmbedResult.__dataclass_fields__] == ["audio", "ctr", "off", "tail", "scale"]
