"""The level mix on the GPU (es_mix_batch, RxEngine.mix / embed, WatermarkEmbedder.embed) against the host
WatermarkEmbedder.process and the outputs captured from the reference (tests/golden/embed_mix.npz).  Every comparison is exact."""
import numpy as np
import pytest
import torch

from test_embed_mix import golden_cases, host_embedder, host_process

pytestmark = pytest.mark.gpu
FL = 1215
KEY = bytes(range(32))


def host_mix(x, chips, block, alpha_db=-10.0, floor_db=-35.0):
    """process() over successive blocks of one recording with a given chip stream -> (out, scale float64 per block)."""
    from echoseal_amd.embedder import EPS, MIX_HEADROOM, TxParams, WatermarkEmbedder
    from echoseal_amd.utils import db_to_lin
    tx = WatermarkEmbedder(KEY, TxParams(target_rel_db=alpha_db, floor_rel_dbfs=floor_db))
    tx._chip_buf = chips.astype(np.float32)
    tx._build_payload = None                                # the stream must suffice: generating a frame would raise
    outs, scales = [], []
    with np.errstate(all="ignore"):
        for s in range(0, x.size, block):
            xb, cb = x[s:s + block], chips[s:s + block]
            outs.append(tx.process(xb))
            # the gain as process() computes it (rtwm/embedder.py:51, 64-73), restated only to read it out ...
            in_rms = float(np.sqrt(np.mean(xb * xb)) + EPS)
            scale = max(db_to_lin(alpha_db) * in_rms, db_to_lin(floor_db))
            headroom = max(MIX_HEADROOM - float(np.max(np.abs(xb))), 0.0)
            peak = float(np.max(np.abs(cb))) + EPS
            scale = min(scale, headroom / peak) if peak > 0.0 else 0.0
            assert (xb + cb * scale).tobytes() == outs[-1].tobytes()      # ... and tied to what process() returned
            scales.append(scale)
    return np.concatenate(outs), np.array(scales, np.float64)


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def chip_stream(rng, n):
    """Something like band-passed +-1 chips: bounded, both signs, the odd exact zero."""
    c = rng.standard_normal(n).astype(np.float32) * np.float32(0.6)
    c[rng.integers(0, n, max(1, n // 50))] = 0.0
    return c


def audio(rng, n, kind):
    if kind == "silence":
        return np.zeros(n, np.float32)
    amp = {"tiny": 1e-21, "quiet": 1e-3, "mid": 0.2, "loud": 0.6, "clip": 1.5}[kind]
    return (rng.uniform(-1, 1, n) * amp).astype(np.float32)


def test_mix_equals_fixture_and_host_process(engine):
    for key, block, ctr0, x, payloads, y, _ in golden_cases():
        tx = host_embedder(key, ctr0, payloads)
        ctrs = [(ctr0 + k) % 2 ** 32 for k in range(len(payloads))]
        chips = tx.make_frames(ctrs, payloads).reshape(-1)
        out, scale = engine.mix(dev(engine, x[None]), dev(engine, chips[None]), block=block, want_scale=True)
        got = out[0].cpu().numpy()
        assert got.tobytes() == y.tobytes(), block
        assert got.tobytes() == host_process(host_embedder(key, ctr0, payloads), x, block).tobytes(), block
        want_scale = host_mix(x, chips[:x.size], block)[1]
        assert scale[0].cpu().numpy().tobytes() == want_scale.tobytes(), block


@pytest.mark.parametrize("block", [1, 7, 8, 63, 128, 129, 1000, 1024, 1215, 4800, 8192, 8193, 20_000, 0])
def test_mix_random_sweep_against_host(engine, block):
    """Block lengths around every boundary of the summation order (0 = one block, the whole recording), n not a multiple of the
    block, non-zero chip offsets, several recordings per launch, every loudness from digital silence to clipping."""
    rng = np.random.default_rng(77 + block)
    kinds = ["silence", "tiny", "quiet", "mid", "loud", "clip"]
    for R, n in ((1, 30_011 if block != 1 else 301), (5, 2 * max(block, 1) + 37 if block else 26_001), (3, 4096 + 4 * (block % 5))):
        if block == 1:
            n = min(n, 400)
        blk = block or n
        x = np.stack([np.concatenate([audio(rng, len(p), kinds[(r + j) % 6]) for j, p in enumerate(np.array_split(np.arange(n), 7))])
                      for r in range(R)])
        off = rng.integers(0, 3000, R)
        stride = n + 3000 + 5
        chips = np.stack([chip_stream(rng, stride) for _ in range(R)])
        out, scale = engine.mix(dev(engine, x), dev(engine, chips), block=blk, chip_off=dev(engine, off.astype(np.int64)), want_scale=True)
        out, scale = out.cpu().numpy(), scale.cpu().numpy()
        for r in range(R):
            want, ws = host_mix(x[r], chips[r, off[r]:off[r] + n], blk)
            assert out[r].tobytes() == want.tobytes(), (block, R, n, r)
            assert scale[r].tobytes() == ws.tobytes(), (block, R, n, r)


def test_mix_many_recordings_in_place_and_special_values(engine):
    rng = np.random.default_rng(5)
    R, n = 300, 5 * 1024 + 256                               # full blocks on the one-wave-per-block kernel, a short last block
    x = (rng.uniform(-1, 1, (R, n)) * rng.uniform(0, 1.2, (R, 1))).astype(np.float32)
    chips = np.stack([chip_stream(rng, n + 7) for _ in range(R)])
    x[3, 100] = np.nan; x[4, 2000] = np.inf; x[5, 3000] = -np.inf; x[5, 3001] = np.nan
    chips[6, 1500] = np.nan                                  # peak is NaN: scale = 0
    chips[7, 10] = np.inf                                    # peak is inf: scale = 0, and inf * 0 is an invalid operation
    x[8] = 0.0; chips[8, :1024] = 0.0                        # silent block, silent chips
    off = (np.arange(R) % 8).astype(np.int64)
    xd = dev(engine, x)
    out = engine.mix(xd, dev(engine, chips), chip_off=dev(engine, off)).cpu().numpy()
    for r in range(R):
        assert out[r].tobytes() == host_mix(x[r], chips[r, off[r]:off[r] + n], 1024)[0].tobytes(), r
    same = engine.mix(xd, dev(engine, chips), chip_off=dev(engine, off), out=xd)
    assert same.data_ptr() == xd.data_ptr() and xd.cpu().numpy().tobytes() == out.tobytes()
    # other gains than the defaults
    got = engine.mix(dev(engine, x[:9]), dev(engine, chips[:9]), target_rel_db=-3.5, floor_rel_dbfs=-60.0, block=480).cpu().numpy()
    for r in range(9):
        assert got[r].tobytes() == host_mix(x[r], chips[r, :n], 480, -3.5, -60.0)[0].tobytes(), r


def test_mix_clamps_offsets_that_leave_the_row(engine):
    rng = np.random.default_rng(6)
    n, stride = 2048 + 100, 2500
    x = audio(rng, n, "mid")[None]
    chips = chip_stream(rng, stride)[None]
    for off in (-300, 700):
        idx = np.clip(off + np.arange(n), 0, stride - 1)
        for block in (1024, 500):
            got = engine.mix(dev(engine, x), dev(engine, chips), block=block, chip_off=dev(engine, np.array([off], np.int64))).cpu().numpy()
            assert got[0].tobytes() == host_mix(x[0], chips[0, idx], block)[0].tobytes(), (off, block)


def seeded_payloads(rng, R, nf):
    return rng.integers(0, 256, (R, nf, 55), dtype=np.uint8)


def test_embed_equals_host_embedder_and_continues(engine):
    rng = np.random.default_rng(9)
    R, n, block = 4, 7000, 1024
    x = np.stack([audio(rng, n, k) for k in ("silence", "quiet", "mid", "loud")])
    ctr0 = np.array([0, 41, 65_530, 2 ** 32 - 2], np.int64)          # the last recording wraps the 32-bit counter
    pl = seeded_payloads(rng, R, 8)
    res = engine.embed(KEY, dev(engine, x), ctr0=ctr0, block=block, payloads=dev(engine, pl))
    got = res.audio.cpu().numpy()
    for r in range(R):
        tx = host_embedder(KEY, int(ctr0[r]), pl[r])
        assert got[r].tobytes() == host_process(tx, x[r], block).tobytes(), r
        assert int(res.ctr[r]) == tx.frame_ctr and tx._chip_buf.size == (FL - int(res.off[r])) % FL
        assert res.tail[r, int(res.off[r]):].cpu().numpy().tobytes() == tx._chip_buf.tobytes()
    assert int(res.ctr[3]) == (2 ** 32 - 2 + 6) % 2 ** 32 == 4
    # two calls that continue the state == one call over the concatenation when the cut is a block boundary ...
    cut = 3 * block
    nf1 = -(-cut // FL)
    a = engine.embed(KEY, dev(engine, x[:, :cut]), ctr0=ctr0, block=block, payloads=dev(engine, pl[:, :nf1]))
    b = engine.embed(KEY, dev(engine, x[:, cut:]), ctr0=a.ctr, block=block, payloads=dev(engine, pl[:, nf1:]), carry=a)
    assert np.concatenate((a.audio.cpu().numpy(), b.audio.cpu().numpy()), axis=1).tobytes() == got.tobytes()
    assert np.array_equal(b.ctr, res.ctr) and np.array_equal(b.off, res.off) and torch.equal(b.tail, res.tail)
    # ... and two host process() sequences otherwise
    cut = 2500
    nf1 = -(-cut // FL)
    a = engine.embed(KEY, dev(engine, x[:, :cut]), ctr0=ctr0, block=block, payloads=dev(engine, pl[:, :nf1]))
    b = engine.embed(KEY, dev(engine, x[:, cut:]), ctr0=a.ctr, block=block, payloads=dev(engine, pl[:, nf1:]), carry=a)
    for r in range(R):
        tx = host_embedder(KEY, int(ctr0[r]), pl[r])
        assert a.audio[r].cpu().numpy().tobytes() == host_process(tx, x[r, :cut], block).tobytes(), r
        assert b.audio[r].cpu().numpy().tobytes() == host_process(tx, x[r, cut:], block).tobytes(), r
        assert int(b.ctr[r]) == tx.frame_ctr


def test_embed_makes_its_own_payloads(engine):
    """No payloads given: plaintext b"ESAL" | ctr | nonce8 | pad11 under the session's key, sealed on the device; with seed= the
    frames of synthetic_frames."""
    from echoseal_amd.crypto import SecureChannel
    x = np.zeros((2, 3000), np.float32)
    res = engine.embed(KEY, dev(engine, x), ctr0=[5, 900], seed=20260101, want_scale=True)
    frames, _ = engine.synthetic_frames(KEY, 5, 3)
    assert torch.equal(engine.mix(dev(engine, x[:1]), frames.reshape(1, -1)), res.audio[:1])
    assert res.scale.shape == (2, 3) and np.array_equal(res.ctr, [8, 903]) and np.array_equal(res.off, [3000 - 2 * FL] * 2)
    rnd = engine.embed(KEY, dev(engine, x), session_nonce=b"sessionN")
    rnd2 = engine.embed(KEY, dev(engine, x), session_nonce=b"sessionN")
    assert not torch.equal(rnd.audio, rnd2.audio)                    # fresh randomness per call, as the reference
    assert SecureChannel(KEY) is not None and rnd.audio.shape == (2, 3000)
    one = engine.embed(KEY, np.zeros(100, np.float32), seed=1)
    assert one.audio.shape == (100,)


def test_round_trip_clips_equal_host_clips_and_verify_alike(engine):
    """The pull request reports what verify() returned; the reference promises nothing for such clips, so only equality is asserted."""
    from rtwm.detector import WatermarkDetector
    from rtwm.embedder import WatermarkEmbedder
    rng = np.random.default_rng(2026)
    for name, x in (("silence", np.zeros(12_000, np.float32)), ("quiet noise", (rng.standard_normal(12_000) * 0.01).astype(np.float32))):
        pl = seeded_payloads(rng, 1, 12)[0]
        host = host_process(host_embedder(KEY, 0, pl), x, 1024)
        tx = host_embedder(KEY, 0, pl)
        gpu = tx.embed(x, block=1024, engine=engine)
        assert gpu.dtype == np.float32 and gpu.tobytes() == host.tobytes(), name
        ref = host_embedder(KEY, 0, pl)
        host_process(ref, x, 1024)
        assert tx.frame_ctr == ref.frame_ctr and tx._chip_buf.tobytes() == ref._chip_buf.tobytes()
        more = audio(rng, 1500, "mid")                               # the embedder's state continues across embed() and process()
        assert tx.embed(more, block=1024, engine=engine).tobytes() == host_process(ref, more, 1024).tobytes()
        v_host = WatermarkDetector(KEY, list_size=8, engine=engine).verify(host, 48_000)
        v_gpu = WatermarkDetector(KEY, list_size=8, engine=engine).verify(gpu, 48_000)
        print(f"verify({name}): host clip {v_host}, GPU clip {v_gpu}")
        assert v_gpu == v_host
    assert isinstance(WatermarkEmbedder(KEY), WatermarkEmbedder)


def test_invalid_arguments_are_refused_before_any_launch(engine):
    import echoseal_amd._native as nat
    lib, ctx = engine._lib, engine._ctx
    x = torch.zeros((2, 2048), dtype=torch.float32, device=engine.device)
    big = torch.zeros(2 * 2048 + 1024, dtype=torch.float32, device=engine.device)
    chips = torch.ones((2, 2048), dtype=torch.float32, device=engine.device)
    out = torch.full_like(x, 7.0)
    off = torch.zeros(2, dtype=torch.int64, device=engine.device)
    st = torch.cuda.current_stream(engine.device).cuda_stream
    p = lambda t: t.data_ptr()

    def call(xp=p(x), R=2, n=2048, block=1024, cp=p(chips), stride=2048, offp=None, outp=p(out), scalep=None):
        return lib.es_mix_batch(ctx, xp, R, n, block, cp, stride, offp, 0.3, 0.01, outp, scalep, st)
    for kw, word in ((dict(block=0), "block"), (dict(block=-5), "block"), (dict(R=-1), "negative"), (dict(n=-1), "negative"),
                     (dict(stride=-1), "negative"), (dict(xp=None), "null"), (dict(cp=None), "null"), (dict(outp=None), "null"),
                     (dict(stride=2047), "shorter"), (dict(stride=0, offp=p(off)), "shorter"),
                     (dict(xp=p(big), outp=p(big) + 4 * 1024), "overlap"), (dict(xp=p(big) + 4 * 1024, outp=p(big)), "overlap")):
        assert call(**kw) == -1, kw                                  # ES_EINVAL
        assert word in lib.es_last_error(ctx).decode(), (kw, lib.es_last_error(ctx))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                  # nothing was launched
    assert call(R=0) == 0 and call(n=0) == 0 and call(R=0, xp=None, cp=None, outp=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(stride=2047, offp=p(off), n=2047) == 0 and call(xp=p(out)) == 0      # a device offset is not checked; exact aliasing is fine
    with pytest.raises(nat.NativeError, match="block"):
        engine.mix(x, chips, block=0)
    with pytest.raises(ValueError):
        engine.mix(x.double(), chips)
    torch.cuda.synchronize()


def test_front_end_context_and_graph_capture(engine):
    from echoseal_amd.engine import RxEngine
    rng = np.random.default_rng(12)
    R, n = 6, 4 * 1024 + 300
    x = dev(engine, np.stack([audio(rng, n, "mid") for _ in range(R)]))
    chips = dev(engine, np.stack([chip_stream(rng, n + 64) for _ in range(R)]))
    off = dev(engine, np.arange(R, dtype=np.int64) * 3)
    want, wscale = engine.mix(x, chips, chip_off=off, want_scale=True)
    front = RxEngine(engine.device, list_size_max=0)
    got, gscale = front.mix(x, chips, chip_off=off, want_scale=True)
    assert torch.equal(got, want) and torch.equal(gscale, wscale)
    # a context that never saw es_set_tables serves the call too
    lib = front._lib
    raw = lib.es_create(engine.device.index, 0)
    assert raw
    try:
        out = torch.empty_like(x)
        assert lib.es_mix_batch(raw, x.data_ptr(), R, n, 1024, chips.data_ptr(), chips.shape[1], off.data_ptr(), 10.0 ** (-10.0 / 20.0),
                                10.0 ** (-35.0 / 20.0), out.data_ptr(), None, torch.cuda.current_stream(engine.device).cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    finally:
        lib.es_destroy(raw)
    # captured into a graph and replayed once: the same bits
    for block in (1024, 700):
        ref = front.mix(x, chips, chip_off=off, block=block)
        out = torch.zeros_like(x)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            front.mix(x, chips, chip_off=off, block=block, out=out)
        torch.cuda.synchronize()
        assert not bool(out.any())                                   # capture only recorded the launches
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), block
    front.close()


# ------------------------------------------------------------------ the frame generator only enqueues
KEY_A, KEY_B = bytes(range(32)), bytes(range(100, 132))


def frame_inputs(engine, seed):
    """Four frames' device inputs: counters around a low-16 wrap, sealed-payload bytes (any 55 bytes make a frame)."""
    rng = np.random.default_rng(seed)
    ctr = torch.tensor([65534, 65535, 65536, 7], dtype=torch.int64, device=engine.device)
    return ctr, dev(engine, rng.integers(0, 256, (4, 55), dtype=np.uint8))


def test_make_frames_of_two_keys_on_two_streams_do_not_share_a_header_pn(engine):
    """The header PN travels by value with each launch: key A's frames on a stream that is still busy and key B's on another, with no
    host synchronisation in between, are each what the same call gives alone."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.engine import RxEngine
    front = RxEngine(engine.device, list_size_max=0)
    sec_a, sec_b = SecureChannel(KEY_A), SecureChannel(KEY_B)
    (ctr_a, pay_a), (ctr_b, pay_b) = frame_inputs(engine, 1), frame_inputs(engine, 2)
    alone_a = front.make_frames(sec_a, KEY_A, ctr_a, pay_a)
    alone_b = front.make_frames(sec_b, KEY_B, ctr_b, pay_b)
    busy = torch.zeros(1 << 26, dtype=torch.float32, device=engine.device)
    torch.cuda.synchronize()
    assert not torch.equal(alone_a[:, 63:191], alone_b[:, 63:191])          # the two header PNs differ, so a mix-up would show
    s1, s2 = torch.cuda.Stream(engine.device), torch.cuda.Stream(engine.device)
    with torch.cuda.stream(s1):
        for _ in range(32):                                                 # a few milliseconds of other work in front of key A's launches
            busy.add_(1.0)
        got_a = front.make_frames(sec_a, KEY_A, ctr_a, pay_a)
    with torch.cuda.stream(s2):
        got_b = front.make_frames(sec_b, KEY_B, ctr_b, pay_b)
    torch.cuda.synchronize()
    assert torch.equal(got_a, alone_a) and torch.equal(got_b, alone_b)
    assert bool((busy == 32.0).all())
    front.close()


def graph_chain(graph):
    """-> (node types in no particular order, is the graph one chain: every node but one root has exactly one predecessor, every node
    but one leaf exactly one successor).  Asked of the HIP runtime the library is linked to."""
    import ctypes
    import echoseal_amd._native as nat
    hip, g, n = nat.load(), ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    ne = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(ne)) == 0
    src, dst = (ctypes.c_void_p * ne.value)(), (ctypes.c_void_p * ne.value)()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(ne)) == 0
    types = []
    for node in nodes:
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t)) == 0
        types.append(t.value)
    chain = ne.value == n.value - 1 and len(set(src)) == ne.value and len(set(dst)) == ne.value
    return types, chain


def test_a_fresh_context_captures_its_first_schedule_and_frames_as_one_chain(engine):
    """Everything a context owns is made by es_create: the first es_schedule_keyed_batch of a context, es_schedule_batch and
    es_tx_frames_batch record into a stream capture as kernel launches on the capture stream alone, and the replays give the eager bits."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.engine import RxEngine
    sec = SecureChannel(KEY_A)
    ring = engine.keyring([KEY_A, KEY_B])                                   # derived by another context: the fresh one below has run nothing
    key_idx = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=engine.device)
    ctr, pay = frame_inputs(engine, 3)
    want_pn, want_band = engine.schedule_keyed(ring, key_idx, ctr)
    want = engine.make_frames(sec, KEY_A, ctr, pay)
    torch.cuda.synchronize()
    front = RxEngine(engine.device, list_size_max=0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        pn, band = front.schedule_keyed(ring, key_idx, ctr)
        frames = front.make_frames(sec, KEY_A, ctr, pay)
    types, chain = graph_chain(graph)
    assert len(types) >= 5 and set(types) == {0}, types                     # hipGraphNodeTypeKernel: no copy from host memory, no host node
    assert chain, "the capture forked: a side stream or an unordered node"
    for _ in range(2):
        for t in (pn, band, frames):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pn, want_pn) and torch.equal(band, want_band) and torch.equal(frames, want)
    del graph
    front.close()
