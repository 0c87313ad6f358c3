"""GPU: the capped launches of the transmit chain, the key ring family, the keyed AEAD and the memo, each past its grid cap.

A launcher that sizes its grid with es_grid strides over what a larger batch adds; these tests launch past(cap) items (tests/grid_caps.py)
and compare bytes, twice over:
  * sub-cap check: the large launch equals the same entry point on consecutive slices of at most one trip's items, every row;
  * host or oracle check: the host code, the oracle or the one-key entry point on every row where that is cheap, else on the index set
    of grid_caps.index_set (the rows around every trip boundary, the ends, 16 seeded rows).
The rescale branch of es_tx_finish_kernel (peak > 3.0), which the shipped band-pass tables never reach, runs here under tables with
scaled numerators, on a front-end engine of its own."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import grid_caps as G
from echoseal_amd import memo as M

M32 = 1 << 32
FL = 1215
KEYS = [bytes(range(32)), bytes(range(100, 132)), b"\x5a" * 32]


def dev(engine, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)


def same_rows(got, want, what):
    """Byte equality of two arrays row by row; a failure names the first differing rows."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        n = got.shape[0]
        bad = np.flatnonzero((got.reshape(n, -1).view(np.uint8) != want.reshape(n, -1).view(np.uint8)).any(axis=1))
        raise AssertionError(f"{what}: {bad.size} of {n} rows differ, first {bad[:8].tolist()}")


def sliced(fn, n, step):
    """fn(slice) -> tensor or tuple of tensors, over consecutive slices of at most `step` rows, concatenated on the host."""
    parts = [fn(s) for s in G.slices(n, step)]
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate([p[i].cpu().numpy() for p in parts]) for i in range(len(parts[0])))
    return np.concatenate([p.cpu().numpy() for p in parts])


def mixed_counters(rng, n):
    """Counters that mix small values, values around 65 535 / 65 536 and values above 2^31; 0, 65 535, 65 536 and 2^32 - 1 occur."""
    c = np.where(np.arange(n) % 3 == 0, rng.integers(0, 300, n),
                 np.where(np.arange(n) % 3 == 1, rng.integers(65_530, 65_542, n), rng.integers(1 << 31, M32, n))).astype(np.int64)
    c[rng.permutation(n)[:4]] = [0, 65_535, 65_536, M32 - 1]
    return c


# ------------------------------------------------------------------------------------------------------------- frame generator
def test_frame_generator_past_the_cap(engine):
    """make_frames on past(64 * cu) frames: es_tx_finish_kernel takes a second trip, es_tx_symbols_kernel up to five."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.embedder import WatermarkEmbedder
    t = G.trip(engine.device)
    B = G.past(t["tx_finish"])
    rng = np.random.default_rng(101)
    key = KEYS[0]
    sec = SecureChannel(key)
    ctr = mixed_counters(rng, B)
    pl = rng.integers(0, 256, (B, 55), dtype=np.uint8)
    band = engine.schedule(sec._prng.sub_key, key, torch.from_numpy(ctr))[1].cpu().numpy()
    assert set(band.tolist()) == {0, 1, 2, 3}
    pld = dev(engine, pl)
    got = engine.make_frames(sec, key, ctr, pld).cpu().numpy()
    assert got.shape == (B, FL) and got.dtype == np.float32
    same_rows(got, sliced(lambda s: engine.make_frames(sec, key, ctr[s], pld[s]), B, t["tx_symbols"]), "make_frames vs its slices")
    idx = G.index_set(B, [t["tx_symbols"], t["tx_finish"]], seed=1)
    assert (idx >= t["tx_finish"]).sum() >= 3
    same_rows(got[idx], WatermarkEmbedder(key).make_frames(ctr[idx], pl[idx]), f"make_frames vs the host embedder on rows {idx.tolist()}")


def test_keyed_frame_generator_past_the_cap(engine):
    """make_frames_keyed on past(64 * cu) frames of three keys: a block's consecutive trips need different header PNs."""
    from echoseal_amd.embedder import WatermarkEmbedder
    t = G.trip(engine.device)
    T, B = t["tx_symbols"], G.past(t["tx_finish"])
    rng = np.random.default_rng(102)
    f = np.arange(B)
    kidx = (f + (f // T) * (1 if (T + 1) % 3 else 2)) % 3
    assert (kidx[:-T] != kidx[T:]).all() and set(kidx.tolist()) == {0, 1, 2}
    ctr = mixed_counters(rng, B)
    pl = rng.integers(0, 256, (B, 55), dtype=np.uint8)
    ring = engine.keyring(KEYS)
    band = engine.schedule_keyed(ring, kidx, ctr, want_pn=False)[1].cpu().numpy()
    assert set(band.tolist()) == {0, 1, 2, 3}
    pld, kd = dev(engine, pl), dev(engine, kidx.astype(np.int32))
    odd = T + 7                                                         # a device key index outside the ring, on a block's second trip
    kd_odd = kd.clone()
    kd_odd[odd] = 3
    got = engine.make_frames_keyed(ring, kd_odd, ctr, pld).cpu().numpy()
    want = sliced(lambda s: engine.make_frames_keyed(ring, kd[s], ctr[s], pld[s]), B, T)
    assert np.isfinite(got[odd]).all()
    keep = np.setdiff1d(f, [odd])
    same_rows(got[keep], want[keep], "make_frames_keyed vs its slices")
    idx = np.setdiff1d(G.index_set(B, [T, t["tx_finish"]], seed=2), [odd])
    tx = [WatermarkEmbedder(k) for k in KEYS]
    host = np.stack([tx[kidx[i]].make_frames([ctr[i]], [pl[i]])[0] for i in idx])
    same_rows(got[idx], host, f"make_frames_keyed vs the host embedder on rows {idx.tolist()}")


def test_frame_generator_rescale_branch(engine, oracle):
    """The peak rule of es_tx_finish_kernel on both sides of `peak > 3.0` (echoseal_amd/embedder.py:120-123), which no +-1 chip
    sequence reaches under the shipped tables: a front-end engine of its own is given each band's numerator times a gain g[band] =
    3.0 / (median unscaled peak of the band's frames), so that half of each band's 256 frames rescale.  Reference per frame, float64:
    oracle.lfilter(g * b, a, chips), peak = max|y| + 1e-12, y *= 1 / peak if peak > 3.0, cast to float32.
    The edge: for one frame the gain is bisected on the host to two ADJACENT doubles g_lo < g_hi with peak(g_lo) <= 3.0 < peak(g_hi)
    (the bisection halves until no double lies between, so it always ends there); the device runs under each and equals its reference."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.embedder import WatermarkEmbedder
    from echoseal_amd.engine import RxEngine
    from echoseal_amd.utils import band_index
    key = KEYS[1]
    rng = np.random.default_rng(103)
    B = 256
    ctr = mixed_counters(rng, B)
    pl = rng.integers(0, 256, (B, 55), dtype=np.uint8)
    tx = WatermarkEmbedder(key)
    band = np.array([band_index(key, int(c)) for c in ctr])
    chips = np.stack([tx._frame_symbols(int(c), bytes(p)) for c, p in zip(ctr, pl)]).astype(np.float32)
    front = RxEngine(engine.device, list_size_max=0)
    ba, tpl, taps, ntaps, frozen = front._tables
    assert (ba[:, 9] == 1.0).all()

    def filtered(i, g):
        return oracle.lfilter(ba[band[i], :9] * g, ba[band[i], 9:], chips[i])

    def peak_of(y):
        return float(np.max(np.abs(y))) + 1e-12

    def reference(i, g):
        y = filtered(i, g)
        peak = peak_of(y)
        if peak > 3.0:
            y = y * (1.0 / peak)
        return y.astype(np.float32), peak > 3.0

    def set_gains(g):
        ba2 = ba.copy()
        ba2[:, :9] *= np.asarray(g, np.float64)[:, None]
        torch.cuda.synchronize()
        assert front._lib.es_set_tables(front._ctx, ba2.ctypes.data, tpl.ctypes.data, taps.ctypes.data, ntaps.ctypes.data, frozen.ctypes.data) == 0

    try:
        peak0 = np.array([peak_of(filtered(i, 1.0)) for i in range(B)])
        assert set(band.tolist()) == {0, 1, 2, 3} and peak0.max() < 3.0     # the shipped tables never rescale
        g = np.array([3.0 / np.median(peak0[band == b]) for b in range(4)])
        ref = [reference(i, g[band[i]]) for i in range(B)]
        scaled = np.array([r[1] for r in ref])
        for b in range(4):
            share = scaled[band == b].mean()
            assert 0.2 <= share <= 0.8, (b, share)
        sec = SecureChannel(key)
        set_gains(g)
        got = front.make_frames(sec, key, ctr, dev(front, pl)).cpu().numpy()
        bad = [i for i in range(B) if got[i].tobytes() != ref[i][0].tobytes()]
        assert not bad, (len(bad), [(i, int(band[i]), bool(scaled[i])) for i in bad[:8]])
        # the edge
        i = int(np.flatnonzero(scaled)[0])
        lo, hi = 0.5 * g[band[i]], g[band[i]]
        assert peak_of(filtered(i, lo)) <= 3.0 < peak_of(filtered(i, hi))
        while True:
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if peak_of(filtered(i, mid)) > 3.0:
                hi = mid
            else:
                lo = mid
        assert np.nextafter(lo, np.inf) == hi and peak_of(filtered(i, lo)) <= 3.0 < peak_of(filtered(i, hi))
        for ge, want_scaled in ((lo, False), (hi, True)):
            gg = g.copy()
            gg[band[i]] = ge
            set_gains(gg)
            want, was = reference(i, ge)
            one = front.make_frames(sec, key, ctr[i:i + 1], dev(front, pl[i:i + 1])).cpu().numpy()[0]
            assert was == want_scaled and one.tobytes() == want.tobytes(), (i, ge, want_scaled, np.flatnonzero(one != want)[:4])
    finally:
        torch.cuda.synchronize()
        front.close()


# ---------------------------------------------------------------------------------------------------------------- polar encode
def test_polar_encode_past_the_cap(engine, oracle):
    t = G.trip(engine.device)
    B = G.past(t["polar_encode"])
    info = np.random.default_rng(104).integers(0, 256, (B, 55), dtype=np.uint8)
    d = dev(engine, info)
    got = engine.polar_encode(d).cpu().numpy()
    same_rows(got, sliced(lambda s: engine.polar_encode(d[s]), B, t["polar_encode"]), "polar_encode vs its slices")
    bits = np.unpackbits(info, axis=1)

    def cmp(lo, hi):
        return [i for i in range(lo, hi) if not np.array_equal(got[i], oracle.polar_encode(bits[i]))]
    bad = oracle.map_records(cmp, B, chunk=256)
    assert not bad, (len(bad), bad[:8])


# -------------------------------------------------------------------------------------------------------------------- key ring
def test_key_ring_past_the_cap(engine):
    from test_gpu_identify import check_ring_row
    t = G.trip(engine.device)
    n = G.past(t["lane"])
    keys = np.random.default_rng(105).integers(0, 256, (n, 32), dtype=np.uint8)
    edge = t["lane"]
    keys[edge] = 0; keys[edge + 1] = 0xFF; keys[0] = 0xFF; keys[n - 1] = 0     # the all-zero and the all-0xFF key, on either trip
    kd = dev(engine, keys)
    ring = engine.keyring(kd).ring.cpu().numpy()
    same_rows(ring, sliced(lambda s: engine.keyring(kd[s]).ring, n, t["lane"]), "key ring vs its slices")
    for k in G.index_set(n, [t["lane"]], seed=5):
        check_ring_row(ring[k], keys[k].tobytes(), int(k))


# -------------------------------------------------------------------------------------------------------------- keyed schedule
def test_keyed_schedule_past_the_cap(engine):
    from echoseal_amd.crypto import SecureChannel
    t = G.trip(engine.device)
    n = G.past(t["lane"])
    rng = np.random.default_rng(106)
    keys = KEYS + [bytes(32), b"\xFF" * 32]
    ring = engine.keyring(keys)
    kidx = rng.integers(0, 5, n)
    ctr = rng.integers(0, M32, n).astype(np.int64)
    special = np.array([0, 65_535, 65_536, M32 - 1], np.int64)
    ctr[:4] = special; ctr[t["lane"] - 2: t["lane"] + 2] = special; ctr[-4:] = special
    kd, cd = dev(engine, kidx.astype(np.int32)), dev(engine, ctr)
    pn, band = engine.schedule_keyed(ring, kd, cd)
    none, band_only = engine.schedule_keyed(ring, kd, cd, want_pn=False)
    pn_only, none2 = engine.schedule_keyed(ring, kd, cd, want_band=False)
    assert none is None and none2 is None
    assert torch.equal(band_only, band) and torch.equal(pn_only, pn)
    pn, band = pn.cpu().numpy(), band.cpu().numpy()
    for k, key in enumerate(keys):
        sel = np.flatnonzero(kidx == k)
        assert 0 < sel.size <= t["lane"]
        p1, b1 = engine.schedule(SecureChannel(key)._prng.sub_key, key, ctrs=torch.from_numpy(ctr[sel]))
        same_rows(pn[sel], p1.cpu().numpy(), f"PN rows of key {k}")
        same_rows(band[sel], b1.cpu().numpy(), f"bands of key {k}")
    assert set(band.tolist()) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------------------------ hop window
def test_hop_window_past_the_cap(engine):
    from echoseal_amd.utils import band_index
    t = G.trip(engine.device)
    rng = np.random.default_rng(107)
    keys = [bytes(32), b"\xFF" * 32] + [rng.bytes(32) for _ in range(31)]
    N, C = len(keys), 406
    HR = -(-G.past(t["lane"]) // (N * C))
    assert N * HR * C > t["lane"]
    base = rng.integers(0, M32 - C, HR).astype(np.int64)
    base[[0, HR // 2, HR - 1]] = [0, 65_500, M32 - 100]
    ring = engine.keyring(keys)
    hop = engine.hop_window(ring, base, C).cpu().numpy()
    assert hop.shape == (N, HR, C)
    ctr = (base[None, :, None] + np.arange(C)[None, None, :] + np.zeros((N, 1, 1), np.int64)).reshape(-1)
    kidx = np.repeat(np.arange(N), HR * C)
    inside = ctr < M32
    assert (~inside).sum() == N * (C - 100)
    flat = hop.reshape(-1)
    assert (flat[~inside] == 0xFF).all()
    where = np.flatnonzero(inside)
    band = sliced(lambda s: engine.schedule_keyed(ring, kidx[where[s]], ctr[where[s]], want_pn=False)[1], where.size, t["lane"])
    same_rows(flat[where], band, "hop window vs the keyed schedule")
    for e in G.index_set(flat.size, [t["lane"]], seed=7):
        assert flat[e] == (band_index(keys[kidx[e]], int(ctr[e])) if inside[e] else 0xFF), int(e)


# ------------------------------------------------------------------------------------------------------------------ keyed AEAD
def test_keyed_aead_past_the_cap(engine):
    """aead_check_keyed (flat and grouped), seal_keyed and select_keyed at L = 1 on past(cap) rows of three interleaved keys: per key a
    block of 4 099 rows built as test_grid_stride_check_and_seal / test_select_grid_stride build theirs (crafted vectors included),
    row i = row i mod 4099 of its key's block, so that a second-trip row differs from its first-trip row.  Every row against the
    one-key entry points, run per key below the cap."""
    from aead_edges import crafted_vectors
    from echoseal_amd.crypto import SecureChannel
    from test_gpu_aead_edges import PERIOD, _mixed_block, _scl_result, _select_frames
    t = G.trip(engine.device)
    cap = t["lane"]
    n = G.past(cap)
    assert cap % PERIOD
    rng = np.random.default_rng(108)
    ring = engine.keyring(KEYS)
    akeys = [SecureChannel(k)._aead._key for k in KEYS]
    kidx = rng.integers(0, 3, n)
    row = np.arange(n) % PERIOD
    sels = [np.flatnonzero(kidx == k) for k in range(3)]
    assert all(0 < s.size <= cap for s in sels)

    def interleave(blocks):
        """blocks[k]: arrays of PERIOD rows for key k -> arrays of n rows, row i from blocks[kidx[i]] at row[i]."""
        out = [np.empty((n,) + a.shape[1:], a.dtype) for a in blocks[0]]
        for k, s in enumerate(sels):
            for o, a in zip(out, blocks[k]):
                o[s] = a[row[s]]
        return out

    crafted = [crafted_vectors(a) for a in akeys]
    blobs, clean, plain, ctr = interleave([_mixed_block(rng, crafted[k], key=akeys[k]) for k in range(3)])
    kd, bd, cd = dev(engine, kidx.astype(np.int32)), dev(engine, blobs), torch.from_numpy(ctr)
    # flat check
    ok, pt = engine.aead_check_keyed(ring, kd, bd, cd, want_plain=True)
    ok, pt = ok.cpu().numpy(), pt.cpu().numpy()
    for k, s in enumerate(sels):
        o1, p1 = engine.aead_check(akeys[k], bd[torch.from_numpy(s).to(engine.device)], torch.from_numpy(ctr[s]), want_plain=True)
        same_rows(ok[s], o1.cpu().numpy(), f"verdicts of key {k}")
        same_rows(pt[s], p1.cpu().numpy(), f"plaintexts of key {k}")
        assert 0 < int(o1.sum()) < s.size
    # grouped check [B, 3, 55], key and counter per frame: the row, the row as it was sealed with a corrupted tag, the row as it was sealed
    Bg = n // 3 + 1
    assert Bg * 3 > cap
    grp = np.stack((blobs[:Bg], clean[:Bg], clean[:Bg]), axis=1)
    grp[:, 1, 50] ^= 0x10
    gd = dev(engine, grp)
    gok, gpt = engine.aead_check_keyed(ring, kd[:Bg], gd, torch.from_numpy(ctr[:Bg]), want_plain=True)
    gok, gpt = gok.cpu().numpy(), gpt.cpu().numpy()
    for k in range(3):
        s = sels[k][sels[k] < Bg]
        o1, p1 = engine.aead_check(akeys[k], gd[torch.from_numpy(s).to(engine.device)], torch.from_numpy(ctr[s]), want_plain=True)
        same_rows(gok[s], o1.cpu().numpy(), f"grouped verdicts of key {k}")
        same_rows(gpt[s], p1.cpu().numpy(), f"grouped plaintexts of key {k}")
    assert not gok[:, 1].any() and 0 < int(gok[:, 0].sum()) < int(gok[:, 2].sum()) < Bg
    # seal: per key aead_seal, and the host-sealed rows themselves
    nd, pd = dev(engine, clean[:, :12]), dev(engine, plain)
    sealed = engine.seal_keyed(ring, kd, nd, pd).cpu().numpy()
    for k, s in enumerate(sels):
        st = torch.from_numpy(s).to(engine.device)
        same_rows(sealed[s], engine.aead_seal(akeys[k], nd[st], pd[st]).cpu().numpy(), f"blobs of key {k}")
    same_rows(sealed, clean, "seal_keyed vs the host-sealed rows")
    # select at L = 1
    frames = [_select_frames(1, PERIOD, akeys[k], [v for v in crafted[k] if v.branch], rng)[0] for k in range(3)]
    arrs = interleave(frames)
    payload, sok, which = engine.select(_scl_result(engine, arrs), ring=ring, key_idx=kd, ctrs=torch.from_numpy(arrs[6]))
    payload, sok, which = payload.cpu().numpy(), sok.cpu().numpy(), which.cpu().numpy()
    seen = set()
    for k, s in enumerate(sels):
        p1, o1, w1 = engine.select(_scl_result(engine, [a[s] for a in arrs]), key32=akeys[k], ctrs=torch.from_numpy(arrs[6][s]))
        same_rows(payload[s], p1.cpu().numpy(), f"selected payloads of key {k}")
        same_rows(sok[s], o1.cpu().numpy(), f"selection verdicts of key {k}")
        same_rows(which[s], w1.cpu().numpy(), f"selected rows of key {k}")
        seen |= set(o1.cpu().numpy().tolist())
    assert seen == {-2, -1, 0, 1}


# ------------------------------------------------------------------------------------------------------------------------ memo
def _u64(x):
    return x.detach().cpu().contiguous().numpy().view(np.uint64)


@pytest.mark.parametrize("slots", [1, 64, 4096])
def test_memo_contested_across_workgroups(engine, slots):
    """Three inserts of past(256 * 64) records with probes between: records from the tiny field ranges of test_gpu_memo._records (512
    distinct records at most), so that nearly every slot is contested by records of different workgroups of 256 and the lowest record
    index has to win across them; every seventh record masked; exact duplicates workgroups apart."""
    n = G.past(G.MEMO_BLOCK * 64)
    rng = np.random.default_rng(109 + slots)
    mem, twin = engine.open_memo(slots), M.MemoModel(slots)
    assert (_u64(mem.table) == M.EMPTY).all()
    for call in range(3):
        k0, k1 = M.pack(rng.integers(0, 4, n), rng.integers(0, 4, n), rng.integers(0, 2, n), rng.integers(0, 8, n), rng.integers(0, 2, n))
        k0[::7] = M.EMPTY
        src = np.arange(1, 50) * 3                                           # exact duplicates in other workgroups
        k0[src + 40 * G.MEMO_BLOCK], k1[src + 40 * G.MEMO_BLOCK] = k0[src], k1[src]
        live = np.flatnonzero(k0 != M.EMPTY)
        wrote = twin.insert(k0, k1)
        # on the host: who took each live record's slot, and from which workgroup
        s = M.slot(k0[live], k1[live], slots)
        winner = np.full(slots, -1, np.int64)
        winner[s[::-1]] = live[::-1]                                         # the lowest record index of each slot
        assert np.array_equal(np.flatnonzero(wrote), np.sort(winner[winner >= 0]))
        lost_across = (winner[s] // G.MEMO_BLOCK != live // G.MEMO_BLOCK).sum()
        assert lost_across > live.size // 2, (call, int(lost_across), live.size)
        engine.memo_insert(mem, k0, k1)
        assert np.array_equal(_u64(mem.table), twin.table), call
        assert (mem.claim.cpu().numpy().view(np.uint32) == 0xFFFFFFFF).all(), call
        hit = engine.memo_probe(mem, k0, k1).cpu().numpy().astype(bool)
        assert np.array_equal(hit, twin.probe(k0, k1)), call
        assert hit[wrote].all() and not hit[k0 == M.EMPTY].any()
        assert np.array_equal(_u64(mem.table), twin.table), call
