"""GPU: the AEAD validator, the sealer and candidate selection of es_aead.hip at their edges.

- Crafted blobs whose Poly1305 accumulator needs the final conditional subtraction (tests/aead_edges.py), under four keys,
  with every single-bit tag flip, ciphertext and nonce corruptions, off-by-one counters, forged magics and extreme counters.
- Launches above the grid cap (num_cu * 8 blocks of 256 lanes), so that lanes take a second trip round the grid-stride loop:
  inputs tile a block of known verdicts with an odd period, so that a second-trip row differs from its first-trip row.
- Selection at L = 1 .. 1024 over frames built to take every branch of the reference's selection
  (rtwm/fastpolar.py:268-276, 332-359): undecoded and skipped records, partial lists, metric ties (-0.0 against +0.0),
  +inf and NaN metrics.  Each frame equals the oracle, the host replay and the class it was built for.
Expected values come from the big-integer host primitives and the C oracle."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from aead_edges import KEY, KEYS, crafted_vectors, seal_rows
from echoseal_amd.primitives import chacha20poly1305_encrypt

M32 = 1 << 32
PERIOD = 4099          # rows of a tiled block: odd (prime), so a grid stride of whole blocks of 256 never maps a row onto its copy


@pytest.fixture(scope="module")
def vectors():
    return {name: crafted_vectors(key) for name, key in KEYS.items()}


def _grid_cap(engine):
    return torch.cuda.get_device_properties(engine.device).multi_processor_count * 8 * 256


def _u8(rows):
    return np.stack([np.frombuffer(r, np.uint8) for r in rows])


def _seal(key, plain, nonce):
    return nonce + chacha20poly1305_encrypt(key, nonce, plain)


def _check(engine, key, blobs, ctrs):
    ok, plain = engine.aead_check(key, torch.from_numpy(np.ascontiguousarray(blobs)).to(engine.device),
                                  torch.from_numpy(np.asarray(ctrs, np.int64)), want_plain=True)
    return ok.cpu().numpy(), plain.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- validator
def _validator_rows(key, vs, rng):
    """(blobs, ctrs, want_ok, want_plain) over the crafted vectors of one key and what corrupts them."""
    rows = []

    def add(blob, ctr, ok, plain):
        rows.append((bytes(blob), int(ctr) % M32, ok, plain if plain is not None else b"\x00" * 27))

    for v in vs:
        add(v.blob, v.ctr, 1, v.plain)
        add(v.blob, v.ctr + 1, 0, v.plain)                               # the tag verifies: plaintext returned, counter rejected
        add(v.blob, v.ctr - 1, 0, v.plain)
    for v in (next(v for v in vs if v.branch), next(v for v in vs if not v.branch)):
        for bit in range(128):                                           # every single-bit tag flip
            b = bytearray(v.blob); b[39 + bit // 8] ^= 1 << (bit % 8); add(b, v.ctr, 0, None)
        for i in range(27):                                              # one bit in each ciphertext byte
            b = bytearray(v.blob); b[12 + i] ^= 1 << (i % 8); add(b, v.ctr, 0, None)
        for i in range(12):                                              # and in each nonce byte
            b = bytearray(v.blob); b[i] ^= 0x80 >> (i % 8); add(b, v.ctr, 0, None)
    ctr = 0x01020304
    tail = rng.bytes(19)
    for pt in (b"ESAM" + ctr.to_bytes(4, "big") + tail, b"DSAL" + ctr.to_bytes(4, "big") + tail,
               b"ESAL" + ctr.to_bytes(4, "little") + tail):              # forged magic, little-endian counter
        add(_seal(key, pt, rng.bytes(12)), ctr, 0, pt)
    for c in (0, 1 << 31, M32 - 1):                                      # extreme counters, accepted when they match
        pt = b"ESAL" + c.to_bytes(4, "big") + rng.bytes(19)
        blob = _seal(key, pt, rng.bytes(12))
        add(blob, c, 1, pt)
        add(blob, c ^ 1, 0, pt)
    blobs, ctrs, ok, plain = zip(*rows)
    return _u8(blobs), np.array(ctrs, np.int64), np.array(ok, np.uint8), _u8(plain)


def test_validator_edges(engine, oracle, vectors):
    rng = np.random.default_rng(5)
    for name, vs in vectors.items():
        key = KEYS[name]
        blobs, ctrs, want_ok, want_plain = _validator_rows(key, vs, rng)
        ok, plain = _check(engine, key, blobs, ctrs)
        bad = np.flatnonzero((ok != want_ok) | (plain != want_plain).any(axis=1))
        assert not len(bad), (name, [(int(i), int(ok[i]), int(want_ok[i])) for i in bad[:8]])
        o_ok, o_plain = oracle.validate_blobs(key, blobs, ctrs)
        assert np.array_equal(o_ok, want_ok) and np.array_equal(o_plain, want_plain), name
        assert int(want_ok.sum()) == len(vs) + 3 and sum(v.branch for v in vs) >= 5


def test_sealer_reproduces_crafted_blobs(engine, vectors):
    """Sealing the crafted plaintexts runs the sealer's own Poly::finish through the final subtraction."""
    for name, vs in vectors.items():
        nonces = _u8([v.nonce for v in vs]); plain = _u8([v.plain for v in vs])
        got = engine.aead_seal(KEYS[name], torch.from_numpy(nonces), torch.from_numpy(plain)).cpu().numpy()
        for v, g in zip(vs, got):
            assert g.tobytes() == v.blob, (name, v.residue)


# -------------------------------------------------------------------------------------------------------- grid-stride loops
def _mixed_block(rng, vs, n=PERIOD, key=KEY):
    """n rows under `key`: its crafted vectors vs, then sealed rows with per-row counters, some sealed with a wrong magic or
    checked against a wrong counter, some with one flipped bit.  -> (blobs, clean blobs, plaintexts, ctrs)."""
    k = len(vs)
    ctr = rng.integers(0, M32, n).astype(np.int64)
    plain = np.zeros((n, 27), np.uint8)
    plain[:, :4] = np.frombuffer(b"ESAL", np.uint8)
    plain[::7, 3] = ord("X")
    plain[:, 4:8] = ctr.astype(">u4").view(np.uint8).reshape(n, 4)
    plain[:, 8:] = rng.integers(0, 256, (n, 19), dtype=np.uint8)
    nonces = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    clean = np.empty((n, 55), np.uint8)
    clean[k:] = seal_rows(key, nonces[k:], plain[k:])
    for i, v in enumerate(vs):
        clean[i] = np.frombuffer(v.blob, np.uint8); plain[i] = np.frombuffer(v.plain, np.uint8); ctr[i] = v.ctr
    blobs = clean.copy()
    bad = np.arange(k, n, 3)
    pos = rng.integers(0, 55 * 8, len(bad))
    blobs[bad, pos // 8] ^= (1 << (pos % 8)).astype(np.uint8)
    ctr[k::5] = (ctr[k::5] + 1) % M32
    return blobs, clean, plain, ctr


def test_grid_stride_check_and_seal(engine, oracle, vectors):
    """aead_check (flat and grouped) and aead_seal with more rows than the capped grid has lanes: every row compared."""
    cap = _grid_cap(engine)
    rng = np.random.default_rng(11)
    blobs, clean, plain, ctr = _mixed_block(rng, vectors["aa"])
    want_ok, want_plain = oracle.validate_blobs(KEY, blobs, ctr)
    assert 0 < int(want_ok.sum()) < PERIOD and (want_plain.any(axis=1) & (want_ok == 0)).any()
    assert want_ok[:len(vectors["aa"])].all()
    n = cap + 4099
    assert n > cap and cap % PERIOD
    idx = np.arange(n) % PERIOD
    ok, pt = _check(engine, KEY, blobs[idx], ctr[idx])
    assert np.array_equal(ok, want_ok[idx]), np.flatnonzero(ok != want_ok[idx])[:8]
    assert np.array_equal(pt, want_plain[idx])
    got = engine.aead_seal(KEY, torch.from_numpy(clean[idx, :12]), torch.from_numpy(plain[idx])).cpu().numpy()
    assert np.array_equal(got, clean[idx]), np.flatnonzero((got != clean[idx]).any(axis=1))[:8]

    # grouped [B, 1024, 55], one counter per B: G patterns of 1024 rows sealed for their own counter, B * 1024 > cap
    G, R = 7, 1024
    gctr = np.array([0, 1 << 31, M32 - 1, *rng.integers(0, M32, G - 3)], np.int64)
    gplain = np.zeros((G, R, 27), np.uint8)
    gplain[:, :, :4] = np.frombuffer(b"ESAL", np.uint8)
    gplain[:, :, 4:8] = gctr.astype(">u4").view(np.uint8).reshape(G, 1, 4)
    gplain[:, 1::9, 7] ^= 1                                              # sealed for another counter
    gplain[:, 2::9, 0] = ord("e")                                        # wrong magic
    gplain[:, :, 8:] = rng.integers(0, 256, (G, R, 19), dtype=np.uint8)
    gblobs = seal_rows(KEY, rng.integers(0, 256, (G * R, 12), dtype=np.uint8), gplain.reshape(G * R, 27)).reshape(G, R, 55)
    gblobs[:, 4::9, 50] ^= 0x10                                          # corrupted tag
    gwant, gwant_plain = oracle.validate_blobs(KEY, gblobs.reshape(-1, 55), np.repeat(gctr, R))
    gwant = gwant.reshape(G, R); gwant_plain = gwant_plain.reshape(G, R, 27)
    assert 0 < int(gwant.sum()) < G * R
    B = cap // R + 5
    assert B * R > cap and (cap // R) % G                                # a second trip lands on another pattern
    gi = np.arange(B) % G
    ok, pt = engine.aead_check(KEY, torch.from_numpy(gblobs[gi]).to(engine.device), torch.from_numpy(gctr[gi]), want_plain=True)
    assert np.array_equal(ok.cpu().numpy(), gwant[gi]) and np.array_equal(pt.cpu().numpy(), gwant_plain[gi])


# ---------------------------------------------------------------------------------------------------------------- selection
MODES = ("undecoded", "skipped", "partial", "crc-ties", "zero-ties", "all-inf", "nan", "crafted-last", "hard-wrong-ctr")


def _select_frames(L, B, akey, crafted, rng):
    """B frames of list size L, frame f in mode MODES[f % len(MODES)] (variants by f // len(MODES)).
    -> arrays (hi, ho, ci, cm, co, nc, ctr), modes, want {use_key: [(ok, which)]}."""
    hi = rng.integers(0, 256, (B, 55), dtype=np.uint8); ho = np.zeros(B, np.uint8)
    ci = rng.integers(0, 256, (B, L, 55), dtype=np.uint8); co = np.zeros((B, L), np.uint8)
    cm = np.abs(rng.normal(0, 10, (B, L))) + 1.0; nc = np.full(B, L, np.int32)
    ctr = rng.integers(0, M32, B).astype(np.int64)
    plain = np.zeros((B, 27), np.uint8)
    plain[:, :4] = np.frombuffer(b"ESAL", np.uint8)
    plain[:, 4:8] = ctr.astype(">u4").view(np.uint8).reshape(B, 4)
    plain[:, 8:] = rng.integers(0, 256, (B, 19), dtype=np.uint8)
    valid = seal_rows(akey, rng.integers(0, 256, (B, 12), dtype=np.uint8), plain)    # valid under (akey, ctr[f])
    modes, want = [], {False: [], True: []}
    for f in range(B):
        mode, var = MODES[f % len(MODES)], f // len(MODES)
        both = None
        if mode == "undecoded":                     # ncand < 0: nothing of the record is defined, valid blobs ignored
            nc[f] = -1; hi[f] = valid[f]; ci[f, 0] = valid[f]; co[f, 0] = 1
            both = (-2, -1)
        elif mode == "skipped" or (mode == "partial" and L == 1):
            nc[f] = 0; ci[f, 0] = valid[f]; co[f, 0] = 1     # list loop skipped, hard candidate fails
            both = (-1, -1)
        elif mode == "partial":                     # a valid, CRC-ok, smallest-metric row past ncand must be ignored
            n = nc[f] = L // 2
            ci[f, n] = valid[f]; co[f, n] = 1; cm[f, n] = -1e300
            ci[f, L - 1] = valid[f]; co[f, L - 1] = 1
            both = (0, int(np.argmin(cm[f, :n])))
        elif mode == "crc-ties":                    # CRC-ok rows that never validate, equal metrics: the first one wins
            pre, ties = ([0], [1, L // 2, L - 1]) if L >= 4 else ([], list(range(L)))
            co[f, pre] = 1; cm[f, pre] = 7.0
            co[f, ties] = 1; cm[f, ties] = -5.0
            if L >= 6:
                cm[f, 2] = -50.0                    # a smaller non-CRC metric must not win
            want[False].append((1, (pre + ties)[0])); want[True].append((0, ties[0]))
        elif mode == "zero-ties":                   # -0.0 == +0.0: the earlier index wins, whatever its sign
            a, b = (L // 3, L - 1) if L >= 2 else (0, 0)
            first, second = (-0.0, 0.0) if var % 2 == 0 else (0.0, -0.0)
            cm[f, b] = second; cm[f, a] = first
            if var % 3 == 2:                        # the same tie among CRC-ok rows
                co[f, a] = co[f, b] = 1
                want[False].append((1, a)); want[True].append((0, a))
            else:
                both = (0, a)
        elif mode == "all-inf":                     # best_any = (inf, hard): the hard candidate, which = -1
            cm[f, :] = np.inf
            both = (0, -1)
        elif mode == "nan":
            v = var % 3 if L >= 4 else 0
            if v == 0:                              # no CRC-ok row: NaN never compares below the best (L = 1: NaN alone)
                cm[f, 0] = cm[f, L // 2] = np.nan
                if L >= 2:
                    cm[f, L - 1] = -3.0
                both = (0, L - 1 if L >= 2 else -1)
            else:                                   # CRC-ok rows [NaN, 1, -1] (the NaN stays best) or [2, NaN, 1]
                rows = [0, L // 2, L - 1]
                co[f, rows] = 1
                cm[f, rows] = [np.nan, 1.0, -1.0] if v == 1 else [2.0, np.nan, 1.0]
                cm[f, 1] = np.nan                   # and a NaN among the rest
                want[False].append((1, 0)); want[True].append((0, 0 if v == 1 else L - 1))
        elif mode == "crafted-last":                # the branch-taking crafted blob is the only valid candidate, at L - 1
            c = crafted[var % len(crafted)]
            ctr[f] = c.ctr; ci[f, L - 1] = np.frombuffer(c.blob, np.uint8); co[f, L - 1] = 1
            if L >= 2:
                co[f, 0] = 1                        # a CRC-ok decoy first
            want[False].append((1, 0)); want[True].append((1, L - 1))
        elif mode == "hard-wrong-ctr":              # a valid hard candidate checked against the next counter
            hi[f] = valid[f]; ho[f] = 1; ctr[f] = (ctr[f] + 1) % M32
            want[False].append((1, -1)); want[True].append((0, int(np.argmin(cm[f]))))
        if both is not None:
            want[False].append(both); want[True].append(both)
        modes.append(mode)
    return (hi, ho, ci, cm, co, nc, ctr), modes, want


def _want_payload(arrs, f, ok, which):
    hi, ci = arrs[0], arrs[2]
    return bytes(55) if ok == -2 else (hi[f] if which < 0 else ci[f, which]).tobytes()


def _scl_result(engine, arrs):
    from echoseal_amd.engine import SclResult
    hi, ho, ci, cm, co, nc, _ = arrs
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(engine.device) for a in (hi, ho, ci, cm, co, nc)]
    return SclResult(*d)


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 257, 1024])
def test_select_edges(engine, oracle, L):
    """engine.select == oracle.select_validated == engine.select_payload (the host replay with a validator built on
    SecureChannel.open) == the (ok, which) each frame was built for, with validator None and with the AEAD validator.
    Undecoded records (ncand < 0) are the kernel's own: ok = -2, a zero payload; the host replay raises on them."""
    from echoseal_amd import _native as nat
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.engine import select_payload
    sec = SecureChannel(KEY)
    akey = sec._aead._key
    crafted = [v for v in crafted_vectors(akey, per_residue=1) if v.branch]
    rng = np.random.default_rng(1000 + L)
    B = 3 * len(MODES)
    arrs = _select_frames(L, B, akey, crafted, rng)
    (hi, ho, ci, cm, co, nc, ctr), modes, want = arrs
    res = _scl_result(engine, arrs[0])
    for use_key in (False, True):
        payload, ok, which = engine.select(res, key32=akey if use_key else None,
                                           ctrs=torch.from_numpy(ctr) if use_key else None)
        payload = payload.cpu().numpy(); ok = ok.cpu().numpy(); which = which.cpu().numpy()
        for f in range(B):
            wok, ww = want[use_key][f]
            got = (int(ok[f]), int(which[f]), payload[f].tobytes())
            assert got == (wok, ww, _want_payload(arrs[0], f, wok, ww)), (L, use_key, f, modes[f], got[:2], (wok, ww))

            def val(p, c=int(ctr[f])):
                pt = sec.open(p)
                return pt.startswith(b"ESAL") and int.from_bytes(pt[4:8], "big") == c
            validator = val if use_key else None
            if nc[f] < 0:
                with pytest.raises(nat.NativeError):
                    select_payload(res, f, validator)
                continue
            op, ook, ow = oracle.select_validated(akey if use_key else None, ctr[f], hi[f], ho[f], ci[f], co[f], cm[f], nc[f])
            assert (op, ook, ow) == (got[2], wok, ww), (L, use_key, f, modes[f])
            if nc[f] == 0:
                with pytest.raises(RuntimeError):
                    select_payload(res, f, validator)
                continue
            hp, hok = select_payload(res, f, validator)
            assert hp == got[2] and hok == (wok == 1), (L, use_key, f, modes[f])
        assert set(modes) == set(MODES)
        classes = {(o, w >= 0) for o, w in want[use_key]}                 # the modes do not collapse into one outcome
        assert {(-2, False), (-1, False), (0, False), (0, True), (1, True)} <= classes
        assert ((1, False) in classes) == (not use_key)                    # the hard candidate: accepted on CRC alone


def test_select_grid_stride(engine, oracle):
    """L = 1 selection with the AEAD validator on more frames than the capped grid has lanes: every frame compared."""
    from echoseal_amd.crypto import SecureChannel
    akey = SecureChannel(KEY)._aead._key
    crafted = [v for v in crafted_vectors(akey, per_residue=1) if v.branch]
    cap = _grid_cap(engine)
    rng = np.random.default_rng(17)
    arrs, modes, want = _select_frames(1, PERIOD, akey, crafted, rng)
    hi, ho, ci, cm, co, nc, ctr = arrs
    wp = np.zeros((PERIOD, 55), np.uint8); wo = np.zeros(PERIOD, np.int8); ww = np.zeros(PERIOD, np.int32)
    for f in range(PERIOD):
        wo[f], ww[f] = want[True][f]
        wp[f] = np.frombuffer(_want_payload(arrs, f, int(wo[f]), int(ww[f])), np.uint8)
        if nc[f] >= 0:
            assert oracle.select_validated(akey, ctr[f], hi[f], ho[f], ci[f], co[f], cm[f], nc[f]) == (wp[f].tobytes(), int(wo[f]), int(ww[f]))
    B = cap + 4099
    assert B > cap and cap % PERIOD
    idx = np.arange(B) % PERIOD
    big = tuple(a[idx] for a in arrs)
    payload, ok, which = engine.select(_scl_result(engine, big), key32=akey, ctrs=torch.from_numpy(big[6]))
    assert np.array_equal(ok.cpu().numpy(), wo[idx]), np.flatnonzero(ok.cpu().numpy() != wo[idx])[:8]
    assert np.array_equal(which.cpu().numpy(), ww[idx]) and np.array_equal(payload.cpu().numpy(), wp[idx])
    assert len(set(zip(wo.tolist(), ww.tolist()))) >= 4
