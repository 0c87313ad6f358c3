"""Live streams without a GPU: the frame layout of a tick (stream_layout) against a brute-force simulation of the buffer rule of
WatermarkEmbedder.process (rtwm/embedder.py:44-62: make a frame whenever the chip buffer runs short), and the two entry points at the
boundary (header, binder, exported symbol)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from code_objects import LIB, ROOT, _tool, code_objects, kernel_metadata

HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
ENTRY_POINTS = {"es_mix_stream_batch": 20, "es_stream_commit_batch": 15}
NEW_KERNELS = ("es_mix_stream_wave_kernel", "es_mix_stream_block_kernelILb0", "es_mix_stream_block_kernelILb1", "es_stream_commit_kernel")
FL = 1215


def simulate(off, ctr, n):
    """One process()-style call of n samples on a stream that has used `off` chips of its current frame: the chip buffer holds the
    other 1215 - off (nothing where off == 0).  -> (counters of the frames made, source of the first sample, next ctr, next off);
    the source is ("tail", index into the current frame) or ("new", 0): chip 0 of the first new frame."""
    buf = [("tail", i) for i in range(off, FL)] if off else []
    made = []
    while len(buf) < n:                                                 # the rule of process()
        buf += [("new", len(made) * FL + i) for i in range(FL)]
        made.append(ctr)
        ctr = (ctr + 1) % 2 ** 32
    first = buf[0] if n else None
    left = len(buf) - n
    return made, first, ctr, (FL - left) % FL


def check(off, ctr, lens):
    from echoseal_amd.engine import stream_layout
    lay = stream_layout(off, ctr, lens)
    first = np.cumsum(lay.nf) - lay.nf
    assert lay.chip_base.tolist() == (first * FL).tolist() and lay.chip_cnt.tolist() == (lay.nf * FL).tolist()
    assert lay.rec.size == lay.ctr.size == int(lay.nf.sum())
    for r, (o, c, n) in enumerate(zip(off, ctr, lens)):
        made, src, c_next, o_next = simulate(int(o), int(c), int(n))
        assert int(lay.nf[r]) == len(made), (o, c, n)
        assert lay.ctr[lay.rec == r].tolist() == made, (o, c, n)
        assert (int(lay.ctr_next[r]), int(lay.off_next[r])) == (c_next, o_next), (o, c, n)
        if n:                                                           # row = [current frame | new frames]; position `start` is sample 0's chip
            s = int(lay.start[r])
            assert (("tail", s) if s < FL else ("new", s - FL)) == src, (o, c, n)


def test_stream_layout_edges():
    offs, ctrs, lens = np.meshgrid([0, 1, 1214], [0, 2 ** 32 - 2, 2 ** 32 - 1], [0, 1, 1214, 1215, 1216, 2430, 2431], indexing="ij")
    check(offs.ravel(), ctrs.ravel(), lens.ravel())


def test_stream_layout_random():
    rng = np.random.default_rng(5)
    n = 3000
    off = rng.integers(0, FL, n)
    off[rng.random(n) < 0.2] = 0
    ctr = rng.integers(0, 2 ** 32, n)
    ctr[rng.random(n) < 0.1] = 2 ** 32 - 1
    check(off, ctr, rng.integers(0, 5000, n))


def test_stream_layout_is_a_chain():
    """successive chunks of one stream: the layout of chunk k starts where chunk k-1 left the stream, and the whole is one embedder"""
    from echoseal_amd.engine import stream_layout
    rng = np.random.default_rng(6)
    off, ctr, made = 0, 2 ** 32 - 3, []
    lens = [0, 7, 1208, 1215, 1, 3000, 0, 2431]
    for n in lens:
        lay = stream_layout([off], [ctr], [n])
        made += lay.ctr.tolist()
        off, ctr = int(lay.off_next[0]), int(lay.ctr_next[0])
    total = sum(lens)
    assert made == [(2 ** 32 - 3 + k) % 2 ** 32 for k in range(-(-total // FL))] and off == total % FL


def test_stream_layout_refuses():
    from echoseal_amd.engine import stream_layout
    for bad in (([FL], [0], [1]), ([-1], [0], [1]), ([0], [0], [-1]), ([0, 0], [0], [1, 1])):
        with pytest.raises(ValueError):
            stream_layout(*bad)


def test_shared_host_steps_of_the_embeds(monkeypatch):
    """the helpers of echoseal_amd.transmit that need no engine: counters per row, clips, payload lists, session nonces, fresh plaintexts"""
    torch = pytest.importorskip("torch")
    from echoseal_amd import transmit as T
    assert T._rows_ctr0(7, 3).tolist() == [7, 7, 7] and T._rows_ctr0(7, 3).dtype == np.int64
    assert T._rows_ctr0([1, 2 ** 32 + 5, 3], 3).tolist() == [1, 2 ** 32 + 5, 3]                 # not yet reduced mod 2^32
    assert T._rows_ctr0(np.array([4]), 1).tolist() == [4] and T._rows_ctr0(0, 0).size == 0
    for bad in ([1, 2], [1, 2, 3, 4], [5]):
        with pytest.raises(ValueError, match="ctr0: a scalar or one value per stream"):
            T._rows_ctr0(bad, 3, "stream")
    x = np.zeros(100, np.float32)
    got = T._clips_1d([x, torch.zeros(5), x[:0]], "clips")
    assert [tuple(t.shape) for t in got] == [(100,), (5,), (0,)] and all(t.dtype == torch.float32 for t in got)
    assert T._clips_1d([], "clips") == []
    for bad, word in ((x.astype(np.float64), "float32"), (x.astype(np.int16), "float32"), (x.reshape(2, 50), "1-D")):
        with pytest.raises(ValueError, match="chunks must be .*" + word):
            T._clips_1d([x, bad], "chunks")
    nf = np.array([2, 0, 1])
    rows = [np.zeros((2, 55), np.uint8), None, np.zeros((3, 55), np.uint8)]
    assert [p.shape for p in T._clip_payloads(rows, nf, "payloads: refused")] == [(2, 55), (0, 55), (3, 55)]
    for bad in ([np.zeros((1, 55), np.uint8), None, rows[2]], rows[:2], [rows[0], None, np.zeros((1, 54), np.uint8)],
                [rows[0], None, np.zeros((1, 55), np.int8)]):
        with pytest.raises(ValueError, match="payloads: refused"):
            T._clip_payloads(bad, nf, "payloads: refused")
    n8 = T._session_nonces([b"A" * 8, bytearray(b"B" * 8)], 2, "refused")
    assert n8.dtype == np.uint8 and n8.shape == (2, 8) and n8.tobytes() == b"A" * 8 + b"B" * 8
    fresh = T._session_nonces(None, 3, "refused")
    assert fresh.shape == (3, 8) and len({r.tobytes() for r in fresh}) == 3 and T._session_nonces(None, 0, "refused").shape == (0, 8)
    for bad, n in (([b"A" * 7], 1), ([b"A" * 9], 1), ([b"A" * 8], 2), ([b"A" * 8] * 3, 2)):
        with pytest.raises(ValueError, match="refused"):
            T._session_nonces(bad, n, "refused")
    ctr = np.array([0, 1, 2 ** 32 - 1], np.int64)
    rows8 = np.arange(24, dtype=np.uint8).reshape(3, 8)
    seen = []
    for nonce_rows, want in ((rows8, rows8), (None, np.zeros((3, 8), np.uint8)), (rows8[:1], np.repeat(rows8[:1], 3, axis=0))):
        nonces, plain = T._fresh_plain(ctr, nonce_rows)
        assert (nonces.dtype, nonces.shape, plain.dtype, plain.shape) == (np.uint8, (3, 12), np.uint8, (3, 27))
        assert all(plain[k, :4].tobytes() == b"ESAL" and plain[k, 4:8].tobytes() == int(c).to_bytes(4, "big") for k, c in enumerate(ctr))
        assert np.array_equal(plain[:, 8:16], want)
        assert nonces.flags.writeable and plain.flags.writeable         # torch.from_numpy takes them as they are
        seen += [r.tobytes() for r in nonces]
    assert len(set(seen)) == 9                                          # a fresh AEAD nonce per blob, call after call
    # the draws from `secrets` come in the order of the reference embedder: the pad bytes of all frames, then the AEAD nonces
    calls = []
    monkeypatch.setattr(T.secrets, "token_bytes", lambda n: (calls.append(n), bytes([len(calls)]) * n)[1])
    nonces, plain = T._fresh_plain(ctr, None)
    assert calls == [33, 36] and (plain[:, 16:27] == 1).all() and (nonces == 2).all()


def test_entry_points_declared_bound_and_exported():
    import echoseal_amd._native as nat
    text = open(HEADER).read()
    assert nat.CONSTANTS["ES_ABI_VERSION"] == nat.ES_ABI_VERSION == 2                             # additive: the version stays
    assert nat.CONSTANTS["ES_STREAM_REC_WORDS"] == nat.ES_STREAM_REC_WORDS == 5
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
    assert "rtwm/embedder.py:34-36,44-75" in text[text.index("Live streams"):]
    args = nat.SIGNATURES["es_mix_stream_batch"][1]                     # the int of the block and the doubles sit where the header puts them
    assert args[5] is ctypes.c_int and args[15] is ctypes.c_double and args[16] is ctypes.c_double and args[7] is ctypes.c_int64


def test_new_kernels_use_no_private_memory_and_old_ones_are_still_there(tmp_path):
    md = {}
    for co in code_objects(tmp_path):
        md.update(kernel_metadata(co))
    for want in NEW_KERNELS + ("es_mix_wave_kernel", "es_mix_ragged_wave_kernel", "es_mix_block_kernelILb1", "es_mix_ragged_block_kernelILb1"):
        hits = [k for k in md if want in k]
        assert len(hits) == 1, (want, hits)
        m = md[hits[0]]
        assert m["private_segment_fixed_size"] == 0, (want, m)          # no scratch: what the allocator moves stays in registers


def test_engine_and_issuer_have_the_interface():
    from echoseal_amd.engine import RxEngine, StreamTable
    from echoseal_amd.issuer import LiveStreams, WatermarkIssuer
    import rtwm.issuer
    assert rtwm.issuer.LiveStreams is LiveStreams
    assert {"key", "ctr", "off", "tail", "nonce8", "ctr_host", "off_host"} <= set(StreamTable.__dataclass_fields__)
    assert all(callable(getattr(RxEngine, m)) for m in ("open_streams", "embed_step", "add_streams", "close_streams"))
    assert all(callable(getattr(LiveStreams, m)) for m in ("push", "state", "add", "close"))
    w = WatermarkIssuer([bytes(32)])
    with pytest.raises(ValueError, match="key index"):                  # refused before an engine is made
        w._key_indices([1])
    assert w._engine is None
