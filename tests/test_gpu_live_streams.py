"""GPU: live streams -- RxEngine.open_streams / embed_step and WatermarkIssuer.open_streams / LiveStreams.push.

The definition is the loop a tick replaces: per stream, embed(key, chunk, ctr0=prev.ctr, carry=prev), `prev` the EmbedResult of the
stream's previous chunk.  Returned audio, the table's ctr / off / tail and the block gains are compared with that chain bit for bit
after every tick; one stream is compared with the host WatermarkEmbedder.process directly."""
import collections

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_embed_mix import host_embedder, host_process

FL = 1215
KEYS = [b"\xAA" * 32, bytes(range(32)), bytes(range(100, 132))]
KEY_IDX = [0, 1, 2, 0, 1, 2]                                            # streams 0 and 3 (1 and 4, 2 and 5) share a key
CTR0 = [0, 5, 2 ** 32 - 2, 1000, 0, 7]
SEED = 20260101
# chunk lengths [tick][stream], None = the stream is absent from the tick; all from {0, 1, 7, 1024, 1214, 1215, 1216, 2431, 3000}
TICKS = [[1215, 1,    1214, 1215, None, 2431],
         [1,    1214, 1,    None, 1,    1214],
         [7,    2431, 3000, 1024, 1214, 0],
         [3000, 0,    7,    None, 1216, 1215],
         [1024, 1216, 2431, 7,    0,    3000]]
AMPL = [0.0, 1e-3, 0.05, 0.2, 0.6, 0.05]                               # silence (floor), quiet, mid, loud (headroom), mid


def test_the_schedule_has_the_cases_it_is_meant_to_have():
    """every stream enters chunks with off == 0 and with off > 0, ends one exactly on a frame edge and has one that makes no frame"""
    for s in range(6):
        off, seen = 0, set()
        for tick in TICKS:
            n = tick[s]
            if n is None:
                seen.add("absent")
                continue
            start = off if off else FL
            seen.add("off0" if off == 0 else "off>0")
            if n and (start + n) % FL == 0:
                seen.add("edge")
            if -(-(start + n) // FL) - 1 == 0:
                seen.add("no new frame")
            off = (start + n) % FL
        assert {"off0", "off>0", "edge", "no new frame"} <= seen, (s, seen)
        assert ("absent" in seen) == (s in (3, 4))


def _chunk(rng, n, ampl):
    x = (ampl * rng.standard_normal(n)).astype(np.float32)
    return np.clip(x, -1.0, 1.0)


def _bits(t, view):
    return t.detach().cpu().contiguous().numpy().view(view)


def _chain_and_ticks(engine, keys, key_idx, ctr0, ticks, ampl, block, *, on_device=False):
    """Runs the ticks through embed_step and every stream's chunks through the embed(carry=) chain; compares all bits after every tick."""
    rng = np.random.default_rng(17)
    table = engine.open_streams(keys, key_idx, ctr0=ctr0)
    S = len(key_idx)
    prev = [None] * S
    kw = dict(block=block, seed=SEED, want_scale=True)
    for t, tick in enumerate(ticks):
        sid = [s for s in range(S) if tick[s] is not None]
        chunks = [_chunk(rng, tick[s], ampl[s]) for s in sid]
        got = engine.embed_step(table, sid, [torch.from_numpy(c).to(engine.device) for c in chunks] if on_device else chunks, **kw)
        assert len(got) == len(sid)
        for s, c, g in zip(sid, chunks, got):
            ref = engine.embed(keys[key_idx[s]], c[None, :], ctr0=ctr0[s] if prev[s] is None else prev[s].ctr, carry=prev[s], **kw)
            prev[s] = ref
            where = (t, s, c.size)
            assert g.audio.shape == (c.size,) and np.array_equal(_bits(g.audio, np.uint32), _bits(ref.audio[0], np.uint32)), where
            assert (g.ctr, g.off) == (int(ref.ctr[0]), int(ref.off[0])), where
            nblk = -(-c.size // block)
            assert g.scale.shape == (nblk,), where
            if nblk:
                assert np.array_equal(_bits(g.scale, np.uint64), _bits(ref.scale[0], np.uint64)), where
        torch.cuda.synchronize()
        for s in range(S):                                              # the whole table, absent streams included
            if prev[s] is None:
                want = (ctr0[s] % 2 ** 32, 0, np.zeros(FL, np.uint32))
            else:
                want = (int(prev[s].ctr[0]), int(prev[s].off[0]), _bits(prev[s].tail[0], np.uint32))
            assert (int(table.ctr[s]), int(table.off[s])) == want[:2] == (int(table.ctr_host[s]), int(table.off_host[s])), (t, s)
            assert np.array_equal(_bits(table.tail[s], np.uint32), want[2]), (t, s)
    return table


@pytest.mark.parametrize("block", [1024, 7, 1215])
def test_ticks_equal_the_embed_carry_chain(engine, block):
    table = _chain_and_ticks(engine, KEYS, KEY_IDX, CTR0, TICKS, AMPL, block)
    assert int(table.ctr_host[2]) < 10                                  # stream 2 has wrapped the 32-bit counter


def test_ticks_cut_into_several_launches_equal_the_chain(engine, monkeypatch):
    """A launch budget of 2431 padded samples cuts every tick into at least two launches: a bucket that mixes an empty chunk with a real
    one, a chunk that exceeds the budget on its own, streams of one tick committed by different launches -- the same bits as one launch."""
    import echoseal_amd.transmit as T
    from echoseal_amd.scan import ragged_buckets
    present = [[n for n in tick if n is not None] for tick in TICKS]
    cuts = [[[lens[i] for i in bucket] for bucket in ragged_buckets(lens, 1, 2431)] for lens in present]
    assert all(len(c) >= 2 for c in cuts), cuts
    assert cuts[0] == [[1, 1214], [1215, 1215], [2431]] and cuts[2] == [[0, 7], [1024, 1214], [2431], [3000]]
    monkeypatch.setattr(T, "EMBED_ROW_SAMPLES", 2431)
    _chain_and_ticks(engine, KEYS, KEY_IDX, CTR0, TICKS, AMPL, 1024)


@pytest.mark.parametrize("block,on_device", [(1024, True), (9000, False)])
def test_every_kernel_path_equals_the_chain(engine, block, on_device):
    """block 1024: a lone stream from off == 0 has its new frames at pool offset 0, so whole blocks take the aligned 16-byte reads; the
    next chunk starts inside the pending frame, so a block reads both sources.  block 9000: blocks longer than one summation chunk."""
    ticks = [[2048, 10_000], [2048, 1], [4096, 9001]]
    _chain_and_ticks(engine, KEYS[:2], [1, 0], [3, 2 ** 32 - 1], ticks, [0.1, 0.3], block, on_device=on_device)


def test_equals_the_host_embedder(engine):
    """One stream through the public interface with explicit payloads, against WatermarkEmbedder.process over block slices of each chunk
    with _build_payload handing out the same blobs in order."""
    from echoseal_amd.engine import stream_layout
    from echoseal_amd.issuer import WatermarkIssuer
    rng = np.random.default_rng(23)
    block, ctr0 = 480, 65_534
    live = WatermarkIssuer(KEYS, engine=engine).open_streams([1], ctr0=ctr0)
    lens = [1000, 215, 0, 1215, 3333, 1]
    pl = rng.integers(0, 256, (-(-sum(lens) // FL), 55), dtype=np.uint8)
    tx = host_embedder(KEYS[1], ctr0, pl)
    used = 0
    for n in lens:
        ctr, off = live.state()
        nf = int(stream_layout(off, ctr, [n]).nf[0])
        x = _chunk(rng, n, 0.1)
        got, = live.push([x], block=block, payloads=[pl[used:used + nf]])
        used += nf
        want = host_process(tx, x, block) if n else np.zeros(0, np.float32)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), n
        ctr, off = live.state()
        assert int(ctr[0]) == tx.frame_ctr and (FL - int(off[0])) % FL == tx._chip_buf.size, n
        torch.cuda.synchronize()
        if off[0]:                                                      # the pending chips are the rest of the table's frame
            assert live.table.tail[0, int(off[0]):].cpu().numpy().tobytes() == tx._chip_buf.tobytes(), n
    assert used == pl.shape[0]


class _CountingLib:
    """The native library handed through, the calls of its entry points counted by name."""

    def __init__(self, lib) -> None:
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


def _snapshot(table, rows):
    torch.cuda.synchronize()
    r = torch.as_tensor(rows, device=table.tail.device)
    return [t[r].cpu().numpy().tobytes() for t in (table.key, table.ctr, table.off, table.tail, table.nonce8)] + \
           [table.ctr_host[rows].tobytes(), table.off_host[rows].tobytes()]


def test_untouched_neighbours_and_empty_pushes(engine, monkeypatch):
    rng = np.random.default_rng(3)
    table = engine.open_streams(KEYS, KEY_IDX, ctr0=CTR0)
    engine.embed_step(table, range(6), [_chunk(rng, 700 + 100 * s, 0.1) for s in range(6)], seed=SEED)      # every stream has a pending frame
    before = _snapshot(table, [0, 2, 5])
    moved = _snapshot(table, [1, 3, 4])
    engine.embed_step(table, [4, 1, 3], [_chunk(rng, n, 0.1) for n in (3000, 1, 1215)], seed=SEED)
    assert _snapshot(table, [0, 2, 5]) == before and _snapshot(table, [1, 3, 4]) != moved
    lib = _CountingLib(engine._lib)
    monkeypatch.setattr(engine, "_lib", lib)
    whole = _snapshot(table, list(range(6)))
    res = engine.embed_step(table, [5, 0], [np.zeros(0, np.float32)] * 2, seed=SEED, want_scale=True)
    assert not lib.calls and _snapshot(table, list(range(6))) == whole
    assert [(r.audio.numel(), r.ctr, r.off, r.scale.numel()) for r in res] == [(0, int(table.ctr_host[s]), int(table.off_host[s]), 0) for s in (5, 0)]
    assert engine.embed_step(table, [], []) == [] and not lib.calls


def test_one_sequence_per_tick_whatever_the_streams_and_keys(engine, monkeypatch):
    rng = np.random.default_rng(4)
    keys16 = [bytes([k]) * 32 for k in range(16)]
    small = engine.open_streams(keys16[:1], [0, 0])
    large = engine.open_streams(keys16, [s % 16 for s in range(64)], ctr0=list(range(64)))
    lib = _CountingLib(engine._lib)
    monkeypatch.setattr(engine, "_lib", lib)

    def refuse(*a, **k):
        raise AssertionError("embed / embed_batch called inside a tick")
    monkeypatch.setattr(engine, "embed", refuse)
    monkeypatch.setattr(engine, "embed_batch", refuse)
    counts = []
    for table in (small, large):
        for lens in ([1024] * table.n, [1024 + 37 * (s % 5) for s in range(table.n)]):      # ... and whatever the lengths
            lib.calls.clear()
            engine.embed_step(table, range(table.n), [_chunk(rng, n, 0.1) for n in lens], seed=SEED)
            counts.append(dict(lib.calls))
    sequence = ("es_aead_seal_keyed_batch", "es_polar_encode_batch", "es_schedule_keyed_batch", "es_tx_frames_keyed_batch",
                "es_mix_stream_batch", "es_stream_commit_batch")
    assert all(c == {name: 1 for name in sequence} for c in counts), counts
    torch.cuda.synchronize()
    assert large.ctr_host.tolist() == [s + 2 for s in range(64)] == large.ctr.cpu().tolist()


def test_random_payloads_carry_the_streams_own_nonce(engine, monkeypatch):
    from echoseal_amd.crypto import SecureChannel
    nonces = [bytes([65 + s]) * 8 for s in range(4)]
    key_idx, ctr0 = [0, 1, 2, 1], [0, 2 ** 32 - 2, 77, 500]
    table = engine.open_streams(KEYS, key_idx, ctr0=ctr0, session_nonces=nonces)
    sealed = []
    seal = engine.seal_keyed

    def recording(ring, kidx, nonce, plain):
        blobs = seal(ring, kidx, nonce, plain)
        sealed.append((kidx.cpu().numpy().copy(), blobs.cpu().numpy().copy()))
        return blobs
    monkeypatch.setattr(engine, "seal_keyed", recording)
    rng = np.random.default_rng(8)
    for sid, lens in (([0, 1, 2, 3], [1300, 2500, 10, 1215]), ([3, 1], [1216, 100]), ([2, 0, 3], [3000, 1, 2431])):
        engine.embed_step(table, sid, [_chunk(rng, n, 0.1) for n in lens])
    assert len(sealed) == 3
    opened = collections.defaultdict(list)
    for kidx, blobs in sealed:
        for k, blob in zip(kidx, blobs):
            plain = SecureChannel(KEYS[int(k)]).open(blob.tobytes())    # raises where the blob was not sealed under that key
            assert len(plain) == 27 and plain[:4] == b"ESAL"
            opened[plain[8:16]].append(int.from_bytes(plain[4:8], "big"))
    # total samples per stream -> frames made; consecutive counters per stream, each under the stream's own nonce
    totals = [1300 + 1, 2500 + 100, 10 + 3000, 1215 + 1216 + 2431]
    assert set(opened) == set(nonces)
    for s in range(4):
        assert opened[nonces[s]] == [(ctr0[s] + k) % 2 ** 32 for k in range(-(-totals[s] // FL))], s
    assert len({b[:12].tobytes() for _, bl in sealed for b in bl}) == sum(len(bl) for _, bl in sealed)       # a fresh AEAD nonce per blob


def test_refusals_come_before_any_launch(engine, monkeypatch):
    from echoseal_amd.issuer import WatermarkIssuer
    table = engine.open_streams(KEYS, KEY_IDX, ctr0=CTR0)
    live = WatermarkIssuer(KEYS, engine=engine).open_streams([0, 1, 2])
    live.close([1])
    lib = _CountingLib(engine._lib)
    monkeypatch.setattr(engine, "_lib", lib)
    x = np.zeros(100, np.float32)
    for sid, chunks, match in (([1, 1], [x, x], "twice"), ([6], [x], "outside"), ([-1], [x], "outside"), ([0], [x, x], "one stream id"),
                               ([0], [x.astype(np.float64)], "float32"), ([0], [x.astype(np.int16)], "float32"), ([0], [x.reshape(2, 50)], "1-D")):
        with pytest.raises(ValueError, match=match):
            engine.embed_step(table, sid, chunks, seed=SEED)
    with pytest.raises(ValueError, match="payloads"):
        engine.embed_step(table, [0], [np.zeros(3000, np.float32)], payloads=[np.zeros((2, 55), np.uint8)])
    with pytest.raises(ValueError, match="closed"):
        live.push([x], [1], seed=SEED)
    with pytest.raises(ValueError, match="one stream id"):
        live.push([x, x, x], seed=SEED)                                 # streams=None names the open streams: two of them
    with pytest.raises(ValueError, match="key index"):
        live.add([3])
    assert not lib.calls
    assert live.state()[0].tolist() == [0, 0, 0] and table.ctr_host.tolist() == [c % 2 ** 32 for c in CTR0]
    # a closed row is handed out again, then the table grows; the new streams start fresh
    assert live.add([2, 0], ctr0=[9, 10]).tolist() == [1, 3] and len(live) == 4
    out = live.push([np.zeros(1300, np.float32)] * 4, seed=SEED)
    assert [o.shape for o in out] == [(1300,)] * 4 and live.state()[0].tolist() == [2, 11, 2, 12] and live.state()[1].tolist() == [85] * 4
    one = WatermarkIssuer(KEYS, engine=engine).open_streams([2], ctr0=9)
    assert one.push([np.zeros(1300, np.float32)], seed=SEED)[0].tobytes() == out[1].tobytes()


def test_entry_points_refuse_records_the_kernels_could_only_clamp(engine):
    """the C ABI itself: rec_host is checked before anything is enqueued, ES_EINVAL with a reason"""
    table = engine.open_streams(KEYS, [0, 1])
    x = torch.zeros((1, 1024), dtype=torch.float32, device=engine.device)
    pool = torch.zeros(2 * FL, dtype=torch.float32, device=engine.device)
    good = (0, 0, 1024, 0, FL)                                          # sid, off, len, chip_base, chip_cnt
    rec_d = torch.tensor(good, dtype=torch.int64, device=engine.device).reshape(5, 1).contiguous()
    p = lambda t: t.data_ptr()

    def mix(rec, total=pool.numel()):
        rec = np.array([rec], np.int64)
        return engine._lib.es_mix_stream_batch(engine._ctx, p(x), 1, 1024, p(rec_d[2]), 1024, p(rec_d[0]), table.n, p(table.tail), p(table.off),
                                               p(pool), total, p(rec_d[3]), p(rec_d[4]), rec.ctypes.data, 0.3, 0.01, p(x), None, engine._stream())

    def commit(rec, total=pool.numel()):
        rec = np.array([rec], np.int64)
        return engine._lib.es_stream_commit_batch(engine._ctx, 1, 1024, p(rec_d[2]), p(rec_d[0]), table.n, p(table.tail), p(table.ctr),
                                                  p(table.off), p(pool), total, p(rec_d[3]), p(rec_d[4]), rec.ctypes.data, engine._stream())
    bad = {"sid": [(2, 0, 1024, 0, FL), (-1, 0, 1024, 0, FL)], "off": [(0, FL, 1024, 0, 2 * FL), (0, -1, 1024, 0, FL)],
           "length": [(0, 0, 1025, 0, FL), (0, 0, -1, 0, 0)], "chip_cnt": [(0, 0, 1024, 0, 0), (0, 0, 1024, 0, 2 * FL), (0, 5, 1024, 0, FL)],
           "pool": [(0, 0, 1024, FL + 1, FL), (0, 0, 1024, -1, FL)]}
    for word, recs in bad.items():
        for rec in recs:
            for call in (mix, commit):
                assert call(rec) == -1, rec                             # ES_EINVAL
                assert word in engine._lib.es_last_error(engine._ctx).decode(), (word, rec)
    assert mix(good, FL - 1) == -1 and "pool" in engine._lib.es_last_error(engine._ctx).decode()
    torch.cuda.synchronize()
    assert int(table.ctr[0]) == 0 and int(table.off[0]) == 0            # nothing ran
    assert mix(good) == 0 and commit(good) == 0
    torch.cuda.synchronize()
    assert (int(table.ctr[0]), int(table.off[0]), int(table.ctr[1]), int(table.off[1])) == (1, 1024, 0, 0)
