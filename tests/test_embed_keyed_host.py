"""The keyed, ragged transmit chain without a GPU: the three entry points at the boundary (header, binder, exported symbol), their
kernels' code objects, the frame layout of embed_batch against the host WatermarkEmbedder, the cut into launches, and
WatermarkIssuer's construction."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from code_objects import LIB, ROOT, _tool, code_objects, kernel_metadata
from test_embed_mix import host_embedder, host_process

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
ENTRY_POINTS = {"es_aead_seal_keyed_batch": 9, "es_tx_frames_keyed_batch": 13, "es_mix_ragged_batch": 15}
NEW_KERNELS = ("es_aead_seal_keyed_kernel", "es_tx_symbols_keyed_kernel", "es_mix_ragged_wave_kernel", "es_mix_ragged_block_kernelILb0",
               "es_mix_ragged_block_kernelILb1")
FL = 1215
KEY = bytes(range(32))


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
    # each cites the reference lines it replaces
    for cite in ("rtwm/crypto.py:33-37", "rtwm/embedder.py:78-141", "rtwm/embedder.py:44-75"):
        assert cite in text[text.index("es_aead_seal_keyed_batch") - 1500:], cite
    # the doubles of the mix and the int of its block sit where the header puts them
    args = nat.SIGNATURES["es_mix_ragged_batch"][1]
    assert args[5] is ctypes.c_int and args[10] is ctypes.c_double and args[11] is ctypes.c_double and args[2] is ctypes.c_int64


def test_new_kernels_use_no_private_memory(tmp_path):
    md = {}
    for co in code_objects(tmp_path):
        md.update(kernel_metadata(co))
    for want in NEW_KERNELS:
        hits = [k for k in md if want in k]
        assert len(hits) == 1, (want, hits)
        m = md[hits[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (want, m)      # nothing goes to memory


@pytest.mark.parametrize("block", [1024, 700])
@pytest.mark.parametrize("ctr0", [0, 65_530, 2 ** 32 - 2])
def test_embed_layout_equals_the_host_embedder(block, ctr0):
    """frames per clip, their counters, the counter after the clip and the chips left pending: what process() does, whatever the block"""
    from echoseal_amd.engine import embed_layout
    lengths = [0, 1, 1214, 1215, 1216, 2430, 7001]
    lay = embed_layout(lengths, ctr0)
    assert lay.nf.tolist() == [-(-n // FL) for n in lengths] and lay.clip.size == lay.ctr.size == int(lay.nf.sum())
    first = np.cumsum(lay.nf) - lay.nf
    assert lay.chip_base.tolist() == (first * FL).tolist() and lay.chip_cnt.tolist() == (lay.nf * FL).tolist()
    rng = np.random.default_rng(ctr0 % 1000 + block)
    for i, n in enumerate(lengths):
        tx = host_embedder(KEY, ctr0, rng.integers(0, 256, (int(lay.nf[i]), 55), dtype=np.uint8))
        made = []
        replay = tx._build_payload
        tx._build_payload = lambda: (made.append(tx.frame_ctr), replay())[1]
        if n:                                                           # (no samples: no process() call, a fresh embedder)
            host_process(tx, (rng.standard_normal(n) * 0.1).astype(np.float32), block)
        assert made == lay.ctr[lay.clip == i].tolist(), (n, made)
        assert tx.frame_ctr == int(lay.ctr_next[i]), n
        pending = 0 if tx._chip_buf is None else tx._chip_buf.size
        assert pending == (FL - int(lay.off[i])) % FL, n
    # a counter per clip
    per = embed_layout(lengths, [ctr0 + 7 * i for i in range(len(lengths))])
    assert per.ctr.tolist() == [(ctr0 + 7 * int(c) + int(k)) % 2 ** 32 for c, k in zip(per.clip, np.arange(per.clip.size) - first[per.clip])]
    assert per.ctr_next.tolist() == [(ctr0 + 7 * i + int(f)) % 2 ** 32 for i, f in enumerate(per.nf)]
    with pytest.raises(ValueError):
        embed_layout([5, -1], 0)


def test_launch_cut_keeps_input_order():
    from echoseal_amd import engine as E
    assert E.EMBED_ROW_SAMPLES >= 1 << 24
    lengths = [7001, 0, 12_345, 500, 1216, 1, 7000, 3000, 1215]
    ctr0 = [100 * i for i in range(len(lengths))]
    whole = E.embed_layout(lengths, ctr0)
    assert len(E.embed_launches(lengths, ctr0)) == 1                    # the default budget takes them all in one launch
    for budget in (21_003, 1, 10 ** 9):
        launches = E.embed_launches(lengths, ctr0, budget)
        assert len(launches) == {21_003: 3, 1: 9, 10 ** 9: 1}[budget]
        seen = [None] * len(lengths)
        for idx, sub in launches:
            assert len(idx) == 1 or len(idx) * max(lengths[i] for i in idx) <= budget
            assert sub.chip_base.tolist() == ((np.cumsum(sub.nf) - sub.nf) * FL).tolist()      # the launch's own flat frame list
            for j, i in enumerate(idx):
                assert seen[i] is None
                seen[i] = (int(sub.nf[j]), sub.ctr[sub.clip == j].tolist(), int(sub.ctr_next[j]), int(sub.off[j]))
        # put back by index, every clip has the frames the layout of the whole batch gives it
        assert seen == [(int(whole.nf[i]), whole.ctr[whole.clip == i].tolist(), int(whole.ctr_next[i]), int(whole.off[i])) for i in range(len(lengths))]


def test_issuer_needs_no_gpu_to_construct_and_refuses_what_it_cannot_do():
    from echoseal_amd.embedder import TxParams
    from echoseal_amd.engine import RxEngine
    from echoseal_amd.issuer import WatermarkIssuer
    import rtwm.issuer
    assert rtwm.issuer.WatermarkIssuer is WatermarkIssuer
    w = WatermarkIssuer([bytes([k]) * 32 for k in range(5)], TxParams(target_rel_db=-12.0))
    assert len(w.keys) == 5 and w._ring is None and w._engine is None      # nothing derived, no engine made
    assert WatermarkIssuer([]).keys == []
    for bad in ([b"short"], [bytes(32), bytes(33)], [bytes(31)]):
        with pytest.raises(ValueError, match="32 bytes"):
            WatermarkIssuer(bad)
    for kw in (dict(N=512), dict(K=256), dict(fs=44_100)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            WatermarkIssuer([KEY], TxParams(**kw))
    with pytest.raises(ValueError, match="preamble"):
        WatermarkIssuer([KEY], TxParams(preamble=np.ones(63, np.uint8)))

    class OtherEngine:                                                  # the limit is the ENGINE's code and rate
        code_k, fs = 256, 48_000
    with pytest.raises(ValueError, match="K"):
        WatermarkIssuer([KEY], engine=OtherEngine())
    assert WatermarkIssuer([KEY], TxParams(K=256), engine=OtherEngine()).p.K == 256
    with pytest.raises(ValueError, match="key index"):
        w.mark_batch([np.zeros(10, np.float32)], [5])
    with pytest.raises(ValueError, match="one key index"):
        w.mark_batch([np.zeros(10, np.float32)], [0, 1])
    assert w.mark_batch([], []) == [] and w._engine is None
    assert all(callable(getattr(RxEngine, m)) for m in ("seal_keyed", "make_frames_keyed", "mix_ragged", "embed_batch"))
