"""GPU: the many-key detector, bit for bit against the single-key path it is defined by.

- key ring: every field of every row against the host derivation (SecureChannel, StreamPRNG.sub_key, HMAC pad states, pn_bits(0, 128),
  band_index(key, 0));
- keyed schedule / select / AEAD check against the unkeyed calls run once per key;
- the plan kernel against identify.plan_reference (itself held to WatermarkDetector._scan_plan by tests/test_identify_host.py) on
  randomised scans and on the real peaks and headers of the golden clips;
- identify_batch against a fresh WatermarkDetector per key and clip: booleans, _trace, _hdr_trace, at several batch caps;
- a true positive: clean LLRs of a blob sealed under one key match exactly that key."""
import hashlib
import hmac
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from identify_cases import plan_inputs
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.identify import WatermarkIdentifier, plan_reference

KEY = b"\xAA" * 32
GOLD = os.path.join(os.path.dirname(__file__), "golden")
N_KEYS = 33                     # not a multiple of the wave size
LIST = 2


def _keys(own=(KEY,)):
    rng = np.random.default_rng(33)
    fixed = [bytes(32), b"\xFF" * 32, *own]
    return fixed + [rng.bytes(32) for _ in range(N_KEYS - len(fixed))]


# ------------------------------------------------------------------------------------------------------------------- key ring
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _compress(state, block):
    """One SHA-256 compression (FIPS 180-4 6.2.2) in plain Python: hashlib does not hand out intermediate states."""
    m = 0xFFFFFFFF
    ror = lambda x, n: ((x >> n) | (x << (32 - n))) & m
    w = [int.from_bytes(block[4 * i:4 * i + 4], "big") for i in range(16)]
    for i in range(16, 64):
        w.append((w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ (w[i - 2] >> 10))) & m)
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        t1 = (h + (ror(e, 6) ^ ror(e, 11) ^ ror(e, 25)) + ((e & f) ^ (~e & m & g)) + _K[i] + w[i]) & m
        t2 = ((ror(a, 2) ^ ror(a, 13) ^ ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & m
        a, b, c, d, e, f, g, h = (t1 + t2) & m, a, b, c, (d + t1) & m, e, f, g
    return [(x + y) & m for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def _pad_states(key):
    """SHA-256 states after the HMAC pad blocks, checked against hashlib: finishing HMAC(key, msg) from them gives hmac.new's digest."""
    ip = _compress(_IV, bytes(b ^ 0x36 for b in key.ljust(64, b"\0")))
    op = _compress(_IV, bytes(b ^ 0x5c for b in key.ljust(64, b"\0")))
    msg = b"\x00\x00\x01\x02"
    inner = _compress(ip, msg + b"\x80" + bytes(51) + ((64 + 4) * 8).to_bytes(8, "big"))
    outer = _compress(op, b"".join(x.to_bytes(4, "big") for x in inner) + b"\x80" + bytes(23) + ((64 + 32) * 8).to_bytes(8, "big"))
    assert b"".join(x.to_bytes(4, "big") for x in outer) == hmac.new(key, msg, hashlib.sha256).digest()
    return ip, op


def check_ring_row(row, key, k):
    """One key-ring row (uint8 [ES_KEYRING_BYTES], host) against the host derivation of `key`, field by field; k names the row."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.primitives import _aes128_round_keys
    from echoseal_amd.utils import band_index
    sec = SecureChannel(key)
    assert row[0:32].tobytes() == sec._aead._key, k
    rk = row[32:208].view(np.uint32)
    assert np.array_equal(rk[:4], np.frombuffer(sec._prng.sub_key, ">u4")), k
    assert np.array_equal(rk, np.frombuffer(_aes128_round_keys(sec._prng.sub_key).tobytes(), ">u4")), k
    ip, op = _pad_states(key)
    assert row[208:240].view(np.uint32).tolist() == ip and row[240:272].view(np.uint32).tolist() == op, k
    assert row[272:288].tobytes() == np.packbits(sec.pn_bits(0, 128)).tobytes(), k
    assert row[288] == band_index(key, 0) and not row[289:].any(), k


def test_ring_rows_equal_host_derivation(engine):
    from echoseal_amd import _native as nat
    assert _compress(_IV, b"abc\x80" + bytes(59) + b"\x18") == [int.from_bytes(hashlib.sha256(b"abc").digest()[4 * i:4 * i + 4], "big") for i in range(8)]
    keys = _keys()
    kr = engine.keyring(keys)
    ring = kr.ring.cpu().numpy()
    assert ring.shape == (N_KEYS, nat.ES_KEYRING_BYTES) and kr.n == N_KEYS
    for k, key in enumerate(keys):
        check_ring_row(ring[k], key, k)
    assert np.array_equal(kr.hop0.cpu().numpy(), ring[:, 288]) and np.array_equal(kr.hdr_pn.cpu().numpy(), ring[:, 272:288])
    with pytest.raises(ValueError):
        engine.keyring([bytes(31)])
    assert engine.keyring([]).n == 0


# --------------------------------------------------------------------------------------------------- keyed schedule / select / check
def test_keyed_schedule_equals_per_key_schedule(engine):
    from echoseal_amd.crypto import SecureChannel
    keys = _keys()
    ring = engine.keyring(keys)
    ctrs = np.array([0, 1, 255, 65_535, 65_536, 2 ** 32 - 1], np.int64)
    rng = np.random.default_rng(4)
    kk, cc = np.meshgrid(np.arange(N_KEYS), ctrs, indexing="ij")
    perm = rng.permutation(kk.size)
    kk, cc = kk.reshape(-1)[perm], cc.reshape(-1)[perm]
    pn, band = engine.schedule_keyed(ring, kk, torch.from_numpy(cc))
    pn = pn.cpu().numpy(); band = band.cpu().numpy()
    none, band_only = engine.schedule_keyed(ring, kk, torch.from_numpy(cc), want_pn=False)
    pn_only, none2 = engine.schedule_keyed(ring, kk, torch.from_numpy(cc), want_band=False)
    assert none is None and none2 is None
    assert np.array_equal(band_only.cpu().numpy(), band) and np.array_equal(pn_only.cpu().numpy(), pn)
    for k, key in enumerate(keys):
        sel = np.flatnonzero(kk == k)
        p1, b1 = engine.schedule(SecureChannel(key)._prng.sub_key, key, ctrs=torch.from_numpy(cc[sel]))
        assert np.array_equal(pn[sel], p1.cpu().numpy()) and np.array_equal(band[sel], b1.cpu().numpy()), k
    assert len(set(band.tolist())) == 4
    # a key index the host can see is refused; one it cannot see gives band 0 and a zero PN row
    with pytest.raises(ValueError):
        engine.schedule_keyed(ring, [0, N_KEYS], [0, 0])
    bad = torch.tensor([-1, N_KEYS, 2 ** 31 - 1, 2], dtype=torch.int32, device=engine.device)
    pn, band = engine.schedule_keyed(ring, bad, torch.zeros(4, dtype=torch.int64))
    p1, b1 = engine.schedule(SecureChannel(keys[2])._prng.sub_key, keys[2], ctrs=torch.zeros(1, dtype=torch.int64))
    assert not pn[:3].any() and not band[:3].any() and torch.equal(pn[3], p1[0]) and band[3] == b1[0]


def test_keyed_select_and_check_equal_per_key_calls(engine):
    from aead_edges import crafted_vectors
    from echoseal_amd.crypto import SecureChannel
    from test_gpu_aead_edges import MODES, _scl_result, _select_frames
    keys = _keys()
    ring = engine.keyring(keys)
    use = [0, 1, 2, 17, 32]
    L, B = 8, 2 * len(MODES)
    per_key, kidx = [], []
    for k in use:
        akey = SecureChannel(keys[k])._aead._key
        crafted = [v for v in crafted_vectors(akey, per_residue=1) if v.branch]
        arrs, _modes, _want = _select_frames(L, B, akey, crafted, np.random.default_rng(700 + k))
        per_key.append(arrs); kidx += [k] * B
    cat = [np.concatenate([a[i] for a in per_key]) for i in range(7)]
    perm = np.random.default_rng(9).permutation(len(kidx))
    kidx = np.array(kidx)[perm]
    cat = [a[perm] for a in cat]
    res = _scl_result(engine, cat)
    payload, ok, which = engine.select(res, ring=ring, key_idx=kidx, ctrs=torch.from_numpy(cat[6]))
    blobs = torch.from_numpy(np.ascontiguousarray(cat[2])).to(engine.device)
    cok, cplain = engine.aead_check_keyed(ring, kidx, blobs, torch.from_numpy(cat[6]), want_plain=True)
    fok, fplain = engine.aead_check_keyed(ring, np.repeat(kidx, L), blobs.reshape(-1, 55), torch.from_numpy(np.repeat(cat[6], L)), want_plain=True)
    assert torch.equal(cok.reshape(-1), fok) and torch.equal(cplain.reshape(-1, 27), fplain)
    seen = set()
    for k in use:
        sel = np.flatnonzero(kidx == k)
        akey = SecureChannel(keys[k])._aead._key
        sub = _scl_result(engine, [a[sel] for a in cat])
        p1, o1, w1 = engine.select(sub, key32=akey, ctrs=torch.from_numpy(cat[6][sel]))
        st = torch.from_numpy(sel).to(engine.device)
        assert torch.equal(payload[st], p1) and torch.equal(ok[st], o1) and torch.equal(which[st], w1), k
        seen |= set(o1.cpu().numpy().tolist())
        ok1, pl1 = engine.aead_check(akey, blobs[st], torch.from_numpy(cat[6][sel]), want_plain=True)
        assert torch.equal(cok[st], ok1) and torch.equal(cplain[st], pl1), k
        assert int(ok1.sum()) > 0
    assert seen == {-2, -1, 0, 1}
    # a key index the host cannot see and that is outside the ring: a validator that accepts nothing
    out = torch.full((len(kidx),), N_KEYS, dtype=torch.int32, device=engine.device)
    _p, o2, _w = engine.select(res, ring=ring, key_idx=out, ctrs=torch.from_numpy(cat[6]))
    assert set(o2.cpu().numpy().tolist()) == {-2, -1, 0}
    ok2, pl2 = engine.aead_check_keyed(ring, out, blobs, torch.from_numpy(cat[6]), want_plain=True)
    assert not ok2.any() and not pl2.any()
    with pytest.raises(ValueError):
        engine.select(res, ring=ring, key_idx=np.full(len(kidx), -1), ctrs=torch.from_numpy(cat[6]))


# ------------------------------------------------------------------------------------------------------------------- plan kernel
def _check_plan(res, N, rows, peaks, npeaks, M, rowband, base, hok, hlo, hop):
    slot = res.slot.cpu().numpy(); ctr = res.ctr.cpu().numpy(); count = res.count.cpu().numpy(); looked = res.looked.cpu().numpy()
    stats = {"cut": 0, "wide": 0, "nonempty": 0}
    for k in range(N):
        for r in range(rows):
            want, want_looked = plan_reference(peaks[r], npeaks[r], M, int(rowband[r]), hok[k, base[r]:], hlo[k, base[r]:], hop[k])
            p = k * rows + r
            got = list(zip(slot[p, :count[p]].tolist(), ctr[p, :count[p]].tolist()))
            assert got == want and looked[p] == want_looked, (k, r, count[p], len(want), got[:4], want[:4])
            stats["cut"] += len(want) == 400
            stats["nonempty"] += bool(want)
            stats["wide"] += any(sum(1 for s, _ in want if s == sl) > 7 for sl in {s for s, _ in want})
    return stats


@pytest.mark.parametrize("M", [1215, 1300, 48_000, 240_000, 3_000_000])
def test_plan_kernel_equals_reference_on_random_scans(engine, M):
    rows, N = 24, N_KEYS
    peaks, npeaks, rowband, base, hok, hlo, hop = plan_inputs(np.random.default_rng(M), M, rows, N)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)
    res = engine.plan(d(peaks), d(npeaks), rowband, base, M, d(hok), d(hlo), d(hop))
    stats = _check_plan(res, N, rows, peaks, npeaks, M, rowband, base, hok, hlo, hop)
    assert stats["nonempty"] > 0 or M < 2430, stats
    if M >= 48_000:
        assert stats["cut"] > 0 and stats["wide"] > 0, stats


@pytest.mark.parametrize("clip", ["verify_trace", "verify3s"])
def test_plan_kernel_equals_reference_on_golden_clips(engine, clip):
    """The planner's real inputs: every plan call of an identify() over the golden clip is replayed on the host."""
    g = np.load(os.path.join(GOLD, f"{clip}.npz"))
    ident = WatermarkIdentifier(_keys(), list_size=LIST, engine=engine)
    calls = []
    real = engine.plan

    def plan(peaks, npeaks, rowband, base, M, hok, hlo, hop):
        res = real(peaks, npeaks, rowband, base, M, hok, hlo, hop)
        h = lambda t: t.cpu().numpy()
        calls.append(_check_plan(res, hop.shape[0], peaks.shape[0], h(peaks), h(npeaks), M, rowband, base, h(hok), h(hlo), h(hop)))
        return res
    engine.plan = plan
    try:
        ident.identify(g["clip"], 48_000)
    finally:
        del engine.plan
    assert len(calls) == 1 and calls[0]["nonempty"] >= N_KEYS


# ------------------------------------------------------------------------------------------------------------------- end to end
def _clips():
    g3 = np.load(os.path.join(GOLD, "verify3s.npz")); g1 = np.load(os.path.join(GOLD, "verify_trace.npz"))
    rng = np.random.default_rng(3)
    return [g1["clip"], g3["clip"][:48000], rng.normal(0, 0.1, 12000).astype(np.float32), np.zeros(12000, np.float32),
            np.zeros(10, np.float32), g1["clip"][::-1].copy(), g3["clip"][:48000] * 0.5]


@pytest.fixture(scope="module")
def per_key_loop(engine):
    """The yardstick: a fresh WatermarkDetector per key and clip."""
    keys, clips = _keys(), _clips()
    out = []
    for clip in clips:
        row = []
        for key in keys:
            det = WatermarkDetector(key, list_size=LIST, engine=engine); det._trace = []; det._hdr_trace = []
            row.append((det.verify(clip, 48_000), det._trace, det._hdr_trace))
        out.append(row)
    return keys, clips, out


@pytest.mark.parametrize("cap", [None, 2, 7, 50])
def test_identify_batch_equals_fresh_detector_per_key(engine, per_key_loop, cap):
    keys, clips, want = per_key_loop
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine)
    ident.trace = True
    if cap is not None:
        ident._pair_cap = lambda: cap
    matches, traces = ident.identify_batch(clips, 48_000)
    assert len(matches) == len(clips)
    tries = 0
    for c in range(len(clips)):
        assert len(matches[c]) == N_KEYS
        for k in range(N_KEYS):
            ok, tr, ht = want[c][k]
            assert (matches[c][k] is not None) == ok, (c, k)
            assert traces[c][k][0] == tr, (c, k, len(traces[c][k][0]), len(tr))
            assert traces[c][k][1] == ht, (c, k, len(traces[c][k][1]), len(ht))
            tries += len(tr)
    assert tries > 20 * N_KEYS
    ident.trace = False
    assert [[m is not None for m in row] for row in ident.identify_batch(clips[:2], 48_000)] == [[w[0] for w in want[c]] for c in range(2)]
    assert ident.identify(clips[4], 48_000) == [None] * N_KEYS


def test_identify_true_positive(engine):
    """The reference's DSP cannot produce a decodable frame: as test_try_decode_frame_true_positive does, patch
    the demodulator stage only -- every candidate then carries the clean LLRs of a blob sealed under key j for a counter of key
    j's plan -- and keep schedule, list decoder and keyed validator real.  Exactly key j matches, at that counter's first try."""
    from echoseal_amd.crypto import SecureChannel
    from echoseal_amd.polar_fast import encode
    from echoseal_amd.utils import BAND_PLAN
    keys = _keys()
    clip = np.load(os.path.join(GOLD, "verify3s.npz"))["clip"][:48000]
    ident = WatermarkIdentifier(keys, list_size=LIST, engine=engine)
    ident.trace = True
    none, traces = ident.identify(clip, 48_000)
    assert none == [None] * N_KEYS
    j = 17
    tr = traces[j][0]
    assert len(tr) > 10
    band_lo, start, ctr = tr[len(tr) // 2]                                   # somewhere inside key j's walk
    first = next(i for i, t in enumerate(tr) if t[2] == ctr)                 # the walk reaches that counter here first
    plain = b"ESAL" + ctr.to_bytes(4, "big") + b"\x07" * 8 + bytes(11)
    blob = SecureChannel(keys[j]).seal(plain)
    clean = torch.from_numpy((2.0 * encode(blob).astype(np.float32) - 1.0) * 6.0).to(engine.device).reshape(1, 1024)
    real_llr = engine.llr
    try:
        engine.llr = lambda *a, **k: clean.expand((k["rows"] if k.get("rows") is not None else a[0]).shape[0], 1024).contiguous()
        got, traces2 = ident.identify(clip, 48_000)
    finally:
        engine.llr = real_llr
    assert [m is not None for m in got] == [k == j for k in range(N_KEYS)]
    m = got[j]
    assert (m.key, m.ctr, m.variant, m.blob, m.plain) == (j, ctr, 0, blob, plain)
    assert (BAND_PLAN[m.band][0], m.start) == tr[first][:2]
    assert traces2[j][0] == tr[:first + 1]
    for k in range(N_KEYS):
        if k != j:
            assert traces2[k] == traces[k], k
    # the detector itself, under the same patch, accepts the same try
    det = WatermarkDetector(keys[j], list_size=LIST, engine=engine); det._trace = []; det._hdr_trace = []
    try:
        engine.llr = lambda *a, **k: clean.expand((k["rows"] if k.get("rows") is not None else a[0]).shape[0], 1024).contiguous()
        assert det.verify(clip, 48_000) is True
    finally:
        engine.llr = real_llr
    assert det._trace == traces2[j][0] and det._hdr_trace == traces2[j][1]
