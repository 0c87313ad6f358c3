"""Marking clips of unequal length, each under its own key, on the GPU: es_aead_seal_keyed_batch, es_tx_frames_keyed_batch,
es_mix_ragged_batch, RxEngine.embed_batch and WatermarkIssuer against the single-key, equal-length entry points they batch
(aead_seal, make_frames, mix, embed) and the host WatermarkEmbedder.process.  Every comparison is of bytes."""
import numpy as np
import pytest
import torch

from test_embed_mix import host_embedder, host_process

pytestmark = pytest.mark.gpu
FL = 1215
KEYS = [bytes(range(32)), bytes(range(100, 132)), b"\x5a" * 32]
MIX_LENS = [0, 1, 7, 1023, 1024, 1025, 2052, 4099, 9000]
CLIP_LENS = [0, 1, 500, 1215, 1216, 3000, 7000, 7001, 12_345]
CLIP_KEY = [0, 1, 2, 2, 0, 1, 1, 0, 2]
CLIP_CTR0 = [0, 41, 65_530, 2 ** 32 - 2, 7, 65_535, 2 ** 32 - 1, 300, 65_530]


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def raw(t):
    return t.cpu().numpy().tobytes()


@pytest.fixture(scope="module", params=["full", "front-end"])
def eng(request, engine):
    """Every test runs on the session's engine and on a front-end context (no list-decoder scratch)."""
    if request.param == "full":
        yield engine
        return
    from echoseal_amd.engine import RxEngine
    front = RxEngine(engine.device, list_size_max=0)
    yield front
    front.close()


# ------------------------------------------------------------------------------------------------------------------ 1. keyed seal
def test_keyed_seal_equals_aead_seal_per_key(eng):
    from echoseal_amd.crypto import SecureChannel
    rng = np.random.default_rng(1)
    n = 37
    ring = eng.keyring(KEYS)
    kidx = rng.integers(0, 3, n)
    assert set(kidx.tolist()) == {0, 1, 2}
    nonces, plain = rng.integers(0, 256, (n, 12), dtype=np.uint8), rng.integers(0, 256, (n, 27), dtype=np.uint8)
    got = eng.seal_keyed(ring, kidx, dev(eng, nonces), dev(eng, plain)).cpu().numpy()
    for k, key in enumerate(KEYS):
        sel = np.flatnonzero(kidx == k)
        want = eng.aead_seal(SecureChannel(key)._aead._key, dev(eng, nonces[sel]), dev(eng, plain[sel])).cpu().numpy()
        assert got[sel].tobytes() == want.tobytes(), k
    # key indices the host cannot see: outside [0, N) a zero blob
    kd = dev(eng, kidx.astype(np.int32))
    kd[5], kd[20] = -1, 3
    odd = eng.seal_keyed(ring, kd, dev(eng, nonces), dev(eng, plain)).cpu().numpy()
    assert not odd[5].any() and not odd[20].any()
    keep = np.setdiff1d(np.arange(n), [5, 20])
    assert odd[keep].tobytes() == got[keep].tobytes()
    with pytest.raises(ValueError, match="key index"):
        eng.seal_keyed(ring, [0, 3], dev(eng, nonces[:2]), dev(eng, plain[:2]))
    assert eng.seal_keyed(ring, [], dev(eng, nonces[:0]), dev(eng, plain[:0])).shape == (0, 55)


# ------------------------------------------------------------------------------------------------------------------ 2. keyed frames
def test_keyed_frames_equal_make_frames_per_key(eng):
    from echoseal_amd.crypto import SecureChannel
    rng = np.random.default_rng(2)
    ctrs = [0, 1, 65_535, 65_536, 2 ** 32 - 1]
    kidx = np.array([k for _ in ctrs for k in (2, 0, 1)])                # interleaved keys
    cc = np.repeat(np.array(ctrs, np.int64), 3)
    pl = rng.integers(0, 256, (cc.size, 55), dtype=np.uint8)
    ring = eng.keyring(KEYS)
    got = eng.make_frames_keyed(ring, kidx, cc, dev(eng, pl)).cpu().numpy()
    assert got.shape == (15, FL) and got.dtype == np.float32
    for k, key in enumerate(KEYS):
        sel = np.flatnonzero(kidx == k)
        want = eng.make_frames(SecureChannel(key), key, cc[sel], dev(eng, pl[sel])).cpu().numpy()
        assert got[sel].tobytes() == want.tobytes(), k
    # a device key index outside the ring: header PN of zero bytes -- the frames of in-range keys are untouched
    kd = dev(eng, kidx.astype(np.int32))
    kd[4] = 3
    odd = eng.make_frames_keyed(ring, kd, cc, dev(eng, pl)).cpu().numpy()
    keep = np.setdiff1d(np.arange(15), [4])
    assert odd[keep].tobytes() == got[keep].tobytes() and np.isfinite(odd[4]).all()


# ------------------------------------------------------------------------------------------------------------------ 3. ragged mix
POISON = np.array([np.nan, np.inf, -np.inf, 1e30], np.float32)
SENTINEL = np.float32(-777.25)


@pytest.fixture(scope="module")
def mix_case(engine):
    """Nine records in rows of 9000 samples, their chips in one pool at aligned and unaligned bases, one chip stream too short; and per
    block length what `mix` gives each record alone (computed once on the session's engine)."""
    rng = np.random.default_rng(3)
    stride = 9000
    R = len(MIX_LENS)
    x = np.empty((R, stride), np.float32)
    base, cnt, pool = [], [], []
    at = 0
    for r, n in enumerate(MIX_LENS):
        amp = [0.0, 1e-3, 0.2, 0.6, 1.5][r % 5]
        x[r, :n] = (rng.uniform(-1, 1, n) * amp).astype(np.float32)
        x[r, n:] = POISON[(np.arange(stride - n) + r) % 4]             # the padding may hold anything
        at += (0, 3, 4, 1, 8, 2, 0, 5, 4)[r]                            # gaps: bases that are and are not multiples of four floats
        c = -(-n // FL) * FL if n != 4099 else 3000                     # the record of 4099 samples runs out of chips: its reads clamp
        base.append(at); cnt.append(c)
        pool.append(np.zeros(at - sum(map(len, pool)), np.float32))
        pool.append((rng.standard_normal(c) * 0.6).astype(np.float32))
        at += c
    pool = np.concatenate(pool)
    base, cnt = np.array(base, np.int64), np.array(cnt, np.int64)
    assert {int(b) % 4 for b in base} >= {0, 1, 3} and pool.size == base[-1] + cnt[-1]
    want = {}
    for block in (1, 700, 1024, 9000):
        for r, n in enumerate(MIX_LENS):
            if n:                                                       # chip_off given: a chip row shorter than the record is allowed and clamps
                o, s = engine.mix(dev(engine, x[r:r + 1, :n]), dev(engine, pool[None, base[r]:base[r] + cnt[r]]), block=block,
                                  chip_off=torch.zeros(1, dtype=torch.int64), want_scale=True)
                want[block, r] = (o[0].cpu().numpy(), s[0].cpu().numpy())
            else:
                want[block, r] = (np.zeros(0, np.float32), np.zeros(0, np.float64))
    return x, pool, base, cnt, want


@pytest.mark.parametrize("block", [1, 700, 1024, 9000])
def test_ragged_mix_equals_mix_on_each_record(eng, mix_case, block):
    x, pool, base, cnt, want = mix_case
    lens = np.array(MIX_LENS, np.int64)
    R, stride = x.shape
    for order in (np.arange(R), np.arange(R)[::-1].copy()):
        xd = dev(eng, x[order])
        out = torch.full_like(xd, float(SENTINEL))
        got, scale = eng.mix_ragged(xd, lens[order], dev(eng, pool), base[order], cnt[order], block=block, want_scale=True, out=out)
        assert got.data_ptr() == out.data_ptr() and scale.shape == (R, -(-stride // block))
        got, scale = got.cpu().numpy(), scale.cpu().numpy()
        for j, r in enumerate(order):
            n = MIX_LENS[r]
            o, s = want[block, r]
            assert got[j, :n].tobytes() == o.tobytes(), (block, r)
            assert (got[j, n:] == SENTINEL).all(), (block, r)           # nothing is written past the record
            assert scale[j, :s.size].tobytes() == s.tobytes(), (block, r)
        full = list(order).index(R - 1)                                 # the row of 9000 samples: `mix` outright
        assert got[full].tobytes() == want[block, R - 1][0].tobytes()
        # in place: the padding survives, bit for bit
        same = eng.mix_ragged(xd, lens[order], dev(eng, pool), base[order], cnt[order], block=block, out=xd)
        assert same.data_ptr() == xd.data_ptr()
        inplace = xd.cpu().numpy()
        for j, r in enumerate(order):
            n = MIX_LENS[r]
            assert inplace[j, :n].tobytes() == want[block, r][0].tobytes() and inplace[j, n:].tobytes() == x[r, n:].tobytes(), (block, r)


def test_ragged_mix_clamps_what_the_host_cannot_see(eng, mix_case):
    """Lengths past the row, negative lengths, chip ranges that leave the pool or are empty: clamped on the device, nothing out of bounds."""
    x, pool, base, cnt, want = mix_case
    R, stride = x.shape
    xd = dev(eng, np.nan_to_num(x, nan=0.1, posinf=0.2, neginf=-0.2) * np.float32(1e-3))
    lens = np.array([stride + 5, -3, 2048, 2048, 2048, 2048, 100, 100, 100], np.int64)
    b = np.array([0, 0, -500, pool.size - 1000, pool.size, 40, 2 ** 62, -2 ** 62, 8], np.int64)
    c = np.array([stride, 50, 4000, 2 ** 62, 10, 0, 10, 10, -4], np.int64)
    out = torch.full_like(xd, float(SENTINEL))
    got = eng.mix_ragged(xd, lens, dev(eng, pool), b, c, block=1024, out=out).cpu().numpy()
    xh = xd.cpu().numpy()

    def alone(r, n, idx):
        return eng.mix(dev(eng, xh[r:r + 1, :n]), dev(eng, pool[None, idx]), block=1024).cpu().numpy()[0]
    assert got[0].tobytes() == alone(0, stride, np.arange(stride)).tobytes()                          # the length is clamped to the row
    assert (got[1] == SENTINEL).all()                                                                  # a negative length is 0
    assert got[2, :2048].tobytes() == alone(2, 2048, np.clip(np.arange(2048) - 500, 0, 3499)).tobytes()     # chips [-500, 3500) cut to the pool
    assert got[3, :2048].tobytes() == alone(3, 2048, np.clip(pool.size - 1000 + np.arange(2048), 0, pool.size - 1)).tobytes()
    for r in (4, 5, 6, 7, 8):                                                                          # no chip at all: a record of length 0
        assert (got[r] == SENTINEL).all(), r
    assert (got[2, 2048:] == SENTINEL).all() and (got[3, 2048:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------------------------ 4. embed_batch
@pytest.fixture(scope="module")
def clip_case():
    """Nine clips of three keys with payloads, and per block length what the host embedder makes of each (computed once)."""
    rng = np.random.default_rng(4)
    clips = [(rng.uniform(-1, 1, n) * [0.0, 1e-3, 0.2, 0.6][i % 4]).astype(np.float32) for i, n in enumerate(CLIP_LENS)]
    payloads = [rng.integers(0, 256, (-(-n // FL), 55), dtype=np.uint8) for n in CLIP_LENS]
    host = {}
    for block in (1024, 700):
        for i, x in enumerate(clips):
            tx = host_embedder(KEYS[CLIP_KEY[i]], CLIP_CTR0[i], payloads[i])
            y = host_process(tx, x, block) if x.size else np.zeros(0, np.float32)
            host[block, i] = (y, tx.frame_ctr, 0 if tx._chip_buf is None else tx._chip_buf.size)
    return clips, payloads, host


def check_against_host(res, host, block):
    for i, r in enumerate(res):
        y, ctr, pending = host[block, i]
        assert r.audio.dtype == torch.float32 and r.audio.shape == (CLIP_LENS[i],)
        assert raw(r.audio) == y.tobytes(), (block, i)
        assert r.ctr == ctr and (FL - r.off) % FL == pending, (block, i)


@pytest.mark.parametrize("block", [1024, 700])
def test_embed_batch_equals_embed_and_the_host_embedder(eng, clip_case, block, monkeypatch):
    import echoseal_amd.transmit as E
    clips, payloads, host = clip_case
    res = eng.embed_batch(KEYS, CLIP_KEY, clips, ctr0=CLIP_CTR0, block=block, payloads=payloads, want_scale=True)
    assert len(res) == len(clips)
    check_against_host(res, host, block)
    for i, x in enumerate(clips):                                       # the loop this call replaces
        one = eng.embed(KEYS[CLIP_KEY[i]], x, ctr0=CLIP_CTR0[i], block=block, payloads=dev(eng, payloads[i][None]), want_scale=True)
        assert raw(res[i].audio) == raw(one.audio), (block, i)
        assert res[i].ctr == int(one.ctr[0]) and res[i].off == int(one.off[0]), (block, i)
        assert res[i].scale.shape == (-(-x.size // block),)
        if x.size:
            assert raw(res[i].scale) == raw(one.scale[0]), (block, i)
    # a key ring made by the caller, a scalar counter, clips on the device
    ring = eng.keyring(KEYS)
    a = eng.embed_batch(ring, CLIP_KEY, [dev(eng, x) for x in clips], ctr0=9, block=block, payloads=payloads)
    b = eng.embed_batch(KEYS, CLIP_KEY, clips, ctr0=[9] * len(clips), block=block, payloads=payloads)
    assert [raw(r.audio) for r in a] == [raw(r.audio) for r in b] and [r.ctr for r in a] == [9 + len(p) for p in payloads]
    # three launches instead of one: the same bits, in input order
    monkeypatch.setattr(E, "EMBED_ROW_SAMPLES", 21_003)
    assert len(E.embed_launches(CLIP_LENS, 0)) == 3
    check_against_host(eng.embed_batch(KEYS, CLIP_KEY, clips, ctr0=CLIP_CTR0, block=block, payloads=payloads), host, block)


def test_embed_batch_seeded_and_fresh_payloads(eng, clip_case, monkeypatch):
    import echoseal_amd.transmit as E
    clips = clip_case[0]
    want = [eng.embed(KEYS[CLIP_KEY[i]], x, ctr0=CLIP_CTR0[i], seed=77) for i, x in enumerate(clips)]
    for budget in (E.EMBED_ROW_SAMPLES, 21_003):
        monkeypatch.setattr(E, "EMBED_ROW_SAMPLES", budget)
        res = eng.embed_batch(KEYS, CLIP_KEY, clips, ctr0=CLIP_CTR0, seed=77)
        for i, (r, w) in enumerate(zip(res, want)):
            assert raw(r.audio) == raw(w.audio) and r.ctr == int(w.ctr[0]) and r.off == int(w.off[0]), (budget, i)
    # neither payloads nor seed: fresh randomness per call, as the reference
    a = eng.embed_batch(KEYS, CLIP_KEY, clips, session_nonces=[b"sessionN"] * len(clips))
    b = eng.embed_batch(KEYS, CLIP_KEY, clips, session_nonces=[b"sessionN"] * len(clips))
    c = eng.embed_batch(KEYS, CLIP_KEY, clips)
    assert [tuple(r.audio.shape) for r in a] == [(n,) for n in CLIP_LENS] == [tuple(r.audio.shape) for r in c]
    assert [r.ctr for r in a] == [-(-n // FL) for n in CLIP_LENS] and [r.off for r in a] == [n % FL for n in CLIP_LENS]
    assert raw(a[-1].audio) != raw(b[-1].audio) and raw(a[5].audio) != raw(b[5].audio)
    assert all(np.isfinite(r.audio.cpu().numpy()).all() for r in c)
    with pytest.raises(ValueError, match="key index"):
        eng.embed_batch(KEYS, [0, 3], clips[:2])
    with pytest.raises(ValueError, match="payloads"):
        eng.embed_batch(KEYS, [0], [clips[5]], payloads=[np.zeros((1, 55), np.uint8)])
    assert eng.embed_batch(KEYS, [], []) == []


# ------------------------------------------------------------------------------------------------------------------ 5. the issuer
def test_issuer_marks_as_the_loop_of_host_embedders(eng):
    from rtwm.issuer import WatermarkIssuer
    rng = np.random.default_rng(5)
    lens, kidx, ctr0 = [2000, 1, 5000, 1216], [1, 0, 1, 0], [3, 65_535, 0, 2 ** 32 - 1]
    clips = [(rng.uniform(-1, 1, n) * 0.3).astype(np.float32) for n in lens]
    payloads = [rng.integers(0, 256, (-(-n // FL), 55), dtype=np.uint8) for n in lens]
    w = WatermarkIssuer(KEYS[:2], engine=eng)
    got = w.mark_batch(clips, kidx, ctr0=ctr0, payloads=payloads)
    for i, g in enumerate(got):
        want = host_process(host_embedder(KEYS[kidx[i]], ctr0[i], payloads[i]), clips[i], 1024)
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.tobytes() == want.tobytes(), i
    assert w.mark(clips[2], 1, ctr0=0, payloads=payloads[2]).tobytes() == got[2].tobytes()
    assert w.mark(clips[0], 1, seed=5).tobytes() == raw(eng.embed(KEYS[1], clips[0], seed=5).audio)


# ------------------------------------------------------------------------------------------------------------------ 6. arguments
def test_invalid_arguments_are_refused_before_any_launch(eng):
    lib, ctx = eng._lib, eng._ctx
    st = torch.cuda.current_stream(eng.device).cuda_stream
    p = lambda t: t.data_ptr()
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device=eng.device)
    ring = eng.keyring(KEYS)
    x = z(2, 2048, dt=torch.float32)
    big = z(2 * 2048 + 1024, dt=torch.float32)
    chips = torch.ones(4 * FL, dtype=torch.float32, device=eng.device)
    out = torch.full_like(x, 7.0)
    lens, base, cnt = z(2, dt=torch.int64) + 2048, z(2, dt=torch.int64), z(2, dt=torch.int64) + 2 * FL

    def mix(xp=p(x), R=2, n=2048, lp=p(lens), block=1024, cp=p(chips), total=4 * FL, bp=p(base), np_=p(cnt), outp=p(out)):
        return lib.es_mix_ragged_batch(ctx, xp, R, n, lp, block, cp, total, bp, np_, 0.3, 0.01, outp, None, st)
    for kw, word in ((dict(block=0), "block"), (dict(block=-5), "block"), (dict(R=-1), "negative"), (dict(n=-1), "negative"),
                     (dict(total=-1), "negative"), (dict(xp=None), "null"), (dict(lp=None), "null"), (dict(cp=None), "null"),
                     (dict(bp=None), "null"), (dict(np_=None), "null"), (dict(outp=None), "null"),
                     (dict(xp=p(big), outp=p(big) + 4 * 1024), "overlap"), (dict(xp=p(big) + 4 * 1024, outp=p(big)), "overlap")):
        assert mix(**kw) == -1, kw                                      # ES_EINVAL
        assert word in lib.es_last_error(ctx).decode() and "es_mix_ragged_batch" in lib.es_last_error(ctx).decode(), kw
    assert mix(R=0) == 0 and mix(n=0) == 0 and mix(R=0, xp=None, lp=None, cp=None, bp=None, np_=None, outp=None) == 0 and mix(total=0) == 0

    nonces, plain, blobs = z(4, 12), z(4, 27), z(4, 55) + 9
    kd = z(4, dt=torch.int32)

    def seal(rp=p(ring.ring), N=3, kp=p(kd), np_=p(nonces), pp=p(plain), n=4, bp=p(blobs)):
        return lib.es_aead_seal_keyed_batch(ctx, rp, N, kp, np_, pp, n, bp, st)
    for kw, word in ((dict(n=-1), "negative"), (dict(N=-1), "negative"), (dict(N=0), "empty key ring"), (dict(rp=None), "null"),
                     (dict(kp=None), "null"), (dict(np_=None), "null"), (dict(pp=None), "null"), (dict(bp=None), "null")):
        assert seal(**kw) == -1, kw
        assert word in lib.es_last_error(ctx).decode() and "es_aead_seal_keyed_batch" in lib.es_last_error(ctx).decode(), kw
    assert seal(n=0) == 0 and seal(n=0, N=0, rp=None, kp=None, np_=None, pp=None, bp=None) == 0

    code, pn, band, ctr = z(4, 1024), z(4, 152), z(4), z(4, dt=torch.int32)
    y_ws, frames = z(4, FL, dt=torch.float64), z(4, FL, dt=torch.float32) + 7
    pre8 = bytes(8)

    def tx(cp=p(code), pp=p(pn), bp=p(band), tp=p(ctr), pre=pre8, rp=p(ring.ring), N=3, kp=p(kd), B=4, yp=p(y_ws), fp=p(frames)):
        return lib.es_tx_frames_keyed_batch(ctx, cp, pp, bp, tp, pre, rp, N, kp, B, yp, fp, st)
    for kw, word in ((dict(B=-1), "negative"), (dict(N=-1), "negative"), (dict(N=0), "empty key ring"), (dict(cp=None), "null"),
                     (dict(pp=None), "null"), (dict(bp=None), "null"), (dict(tp=None), "null"), (dict(pre=None), "null"),
                     (dict(rp=None), "null"), (dict(kp=None), "null"), (dict(yp=None), "null"), (dict(fp=None), "null")):
        assert tx(**kw) == -1, kw
        assert word in lib.es_last_error(ctx).decode() and "es_tx_frames_keyed_batch" in lib.es_last_error(ctx).decode(), kw
    assert tx(B=0) == 0 and tx(B=0, N=0, rp=None, kp=None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((blobs == 9).all()) and bool((frames == 7.0).all())      # nothing was launched
    assert mix(xp=p(out)) == 0                                          # exact aliasing is fine
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        eng.mix_ragged(x, [1, 2, 3], chips, [0, 0], [5, 5])


# ------------------------------------------------------------------------------------------------------------------ 7. capture
def test_keyed_frames_and_ragged_mix_are_capturable(eng):
    """es_tx_frames_keyed_batch + es_mix_ragged_batch only enqueue: captured on one stream and replayed once, the same bits."""
    from echoseal_amd.engine import embed_layout
    from echoseal_amd.utils import db_to_lin, mseq_63
    rng = np.random.default_rng(7)
    lens = np.array([3000, 1024, 5000, 77], np.int64)
    kidx, ctr0 = [2, 0, 1, 1], [0, 65_534, 5, 2 ** 32 - 1]
    lay = embed_layout(lens, ctr0)
    F, stride = lay.clip.size, 5000
    ring = eng.keyring(KEYS)
    x = dev(eng, (rng.uniform(-1, 1, (4, stride)) * 0.3).astype(np.float32))
    kd = dev(eng, np.array(kidx, np.int32)[lay.clip])
    cd = eng._ctr_dev(lay.ctr)
    blobs = dev(eng, rng.integers(0, 256, (F, 55), dtype=np.uint8))
    code = eng.polar_encode(blobs)
    pn, band = eng.schedule_keyed(ring, kd, lay.ctr)
    ld, bd, nd = dev(eng, lens), dev(eng, lay.chip_base), dev(eng, lay.chip_cnt)
    y_ws = torch.empty((F, FL), dtype=torch.float64, device=eng.device)
    frames = torch.zeros((F, FL), dtype=torch.float32, device=eng.device)
    pre8 = np.packbits(np.concatenate((mseq_63().astype(np.uint8), np.zeros(1, np.uint8)))).tobytes()
    for block in (1024, 700):
        ref = eng.mix_ragged(x, lens, eng.make_frames_keyed(ring, kd, lay.ctr, blobs), lay.chip_base, lay.chip_cnt, block=block, out=torch.zeros_like(x))
        out = torch.zeros_like(x)
        frames.zero_()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st = torch.cuda.current_stream(eng.device).cuda_stream
            assert eng._lib.es_tx_frames_keyed_batch(eng._ctx, code.data_ptr(), pn.data_ptr(), band.data_ptr(), cd.data_ptr(), pre8,
                                                     ring.ring.data_ptr(), ring.n, kd.data_ptr(), F, y_ws.data_ptr(), frames.data_ptr(), st) == 0
            assert eng._lib.es_mix_ragged_batch(eng._ctx, x.data_ptr(), 4, stride, ld.data_ptr(), block, frames.data_ptr(), F * FL, bd.data_ptr(),
                                                nd.data_ptr(), db_to_lin(-10.0), db_to_lin(-35.0), out.data_ptr(), None, st) == 0
        torch.cuda.synchronize()
        assert not bool(out.any()) and not bool(frames.any())           # capture only recorded the launches
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref), block
