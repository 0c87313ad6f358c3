"""Edge vectors of the payload AEAD (ChaCha20-Poly1305 over 55-byte blobs: nonce 12 | ciphertext 27 | tag 16), built on the
host without a GPU or the C oracle.

The Poly1305 code of es_aead.hip and of oracle/c/eso_aead.c is the same 26-bit limb code, so comparing the two cannot find a
bug in it.  The vectors here are crafted so that the MAC accumulator, before `+ s`, lands on chosen residues mod p = 2^130 - 5:
0..4, where the limbs hold t + p and `finish` must take its conditional subtraction, and p - 1, p - 2, p - 6, just below p.
Their tags come from echoseal_amd.primitives, plain big-integer arithmetic; `poly1305_limbs` restates the kernel's limb code
only to prove which vectors reach the subtraction."""
import numpy as np

from echoseal_amd.primitives import _aead_tag, _chacha_blocks, chacha20_xor, chacha20poly1305_encrypt, poly1305_tag

P1305 = (1 << 130) - 5
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

KEY = b"\xAA" * 32
KEYS = {"aa": KEY, "zero": b"\x00" * 32, "ff": b"\xFF" * 32,
        "random": bytes(np.random.default_rng(20261016).integers(0, 256, 32, dtype=np.uint8))}
BRANCH_RESIDUES = (0, 1, 2, 3, 4)                       # limb form t + p: the final subtraction runs
BELOW_P_RESIDUES = (P1305 - 1, P1305 - 2, P1305 - 6)    # limb form t itself: it does not
RESIDUES = BRANCH_RESIDUES + BELOW_P_RESIDUES


def _le32(b: bytes, o: int) -> int:
    return int.from_bytes(b[o:o + 4], "little")


def poly1305_limbs(otk: bytes, msg: bytes, *, final_subtract: bool = True):
    """Poly::init / block / finish of es_aead.hip, line for line, every intermediate masked to its C width (a short last
    block is padded as eso_poly1305 pads it).  -> (tag, took_final_subtract).  final_subtract=False drops the conditional
    h - p, so that a test can show its vectors would catch that."""
    k = [_le32(otk, 4 * i) for i in range(8)]
    r0 = k[0] & 0x3ffffff
    r1 = ((k[0] >> 26) | (k[1] << 6)) & 0x3ffff03
    r2 = ((k[1] >> 20) | (k[2] << 12)) & 0x3ffc0ff
    r3 = ((k[2] >> 14) | (k[3] << 18)) & 0x3f03fff
    r4 = (k[3] >> 8) & 0x00fffff
    s1, s2, s3, s4 = (r1 * 5) & M32, (r2 * 5) & M32, (r3 * 5) & M32, (r4 * 5) & M32
    h0 = h1 = h2 = h3 = h4 = 0
    for o in range(0, len(msg), 16):
        blk = msg[o:o + 16]
        blk = (blk + b"\x01" + b"\x00" * 16)[:17] if len(blk) < 16 else blk + b"\x01"
        m = [_le32(blk, 4 * i) for i in range(4)]
        h0 = (h0 + (m[0] & 0x3ffffff)) & M32
        h1 = (h1 + (((m[0] >> 26) | (m[1] << 6)) & 0x3ffffff)) & M32
        h2 = (h2 + (((m[1] >> 20) | (m[2] << 12)) & 0x3ffffff)) & M32
        h3 = (h3 + (((m[2] >> 14) | (m[3] << 18)) & 0x3ffffff)) & M32
        h4 = (h4 + ((m[3] >> 8) | (blk[16] << 24))) & M32
        d0 = (h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1) & M64
        d1 = (h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2) & M64
        d2 = (h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3) & M64
        d3 = (h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4) & M64
        d4 = (h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0) & M64
        c = (d0 >> 26) & M32; h0 = d0 & 0x3ffffff
        d1 = (d1 + c) & M64; c = (d1 >> 26) & M32; h1 = d1 & 0x3ffffff
        d2 = (d2 + c) & M64; c = (d2 >> 26) & M32; h2 = d2 & 0x3ffffff
        d3 = (d3 + c) & M64; c = (d3 >> 26) & M32; h3 = d3 & 0x3ffffff
        d4 = (d4 + c) & M64; c = (d4 >> 26) & M32; h4 = d4 & 0x3ffffff
        h0 = (h0 + c * 5) & M32; c = h0 >> 26; h0 &= 0x3ffffff; h1 = (h1 + c) & M32
    c = h1 >> 26; h1 &= 0x3ffffff
    h2 = (h2 + c) & M32; c = h2 >> 26; h2 &= 0x3ffffff
    h3 = (h3 + c) & M32; c = h3 >> 26; h3 &= 0x3ffffff
    h4 = (h4 + c) & M32; c = h4 >> 26; h4 &= 0x3ffffff
    h0 = (h0 + c * 5) & M32; c = h0 >> 26; h0 &= 0x3ffffff; h1 = (h1 + c) & M32
    g0 = (h0 + 5) & M32; c = g0 >> 26; g0 &= 0x3ffffff
    g1 = (h1 + c) & M32; c = g1 >> 26; g1 &= 0x3ffffff
    g2 = (h2 + c) & M32; c = g2 >> 26; g2 &= 0x3ffffff
    g3 = (h3 + c) & M32; c = g3 >> 26; g3 &= 0x3ffffff
    g4 = (h4 + c - (1 << 26)) & M32
    mask = ((g4 >> 31) - 1) & M32                       # all ones if h >= p
    took = mask == M32
    if final_subtract:
        nm = ~mask & M32
        h0 = (h0 & nm) | (g0 & mask); h1 = (h1 & nm) | (g1 & mask); h2 = (h2 & nm) | (g2 & mask)
        h3 = (h3 & nm) | (g3 & mask); h4 = (h4 & nm) | (g4 & mask)
    w0 = (h0 | (h1 << 26)) & M32
    w1 = ((h1 >> 6) | (h2 << 20)) & M32
    w2 = ((h2 >> 12) | (h3 << 14)) & M32
    w3 = ((h3 >> 18) | (h4 << 8)) & M32
    f = w0 + k[4]; t0 = f & M32
    f = w1 + k[5] + (f >> 32); t1 = f & M32
    f = w2 + k[6] + (f >> 32); t2 = f & M32
    f = w3 + k[7] + (f >> 32); t3 = f & M32
    return b"".join(t.to_bytes(4, "little") for t in (t0, t1, t2, t3)), took


def keystream(key: bytes, nonce: bytes, counter: int) -> bytes:
    """One 64-byte ChaCha20 block (RFC 8439 2.3)."""
    return _chacha_blocks(np.frombuffer(key, "<u4").reshape(1, 8), np.array([counter], np.uint32),
                          np.frombuffer(nonce, "<u4").reshape(1, 3))[0].tobytes()


def mac_input(ct: bytes) -> bytes:
    """What Poly1305 runs over for a 27-byte ciphertext and no AAD: ct, zero pad to 32, le64(0) | le64(27)."""
    return ct + b"\x00" * (-len(ct) % 16) + (0).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def accumulator(otk: bytes, msg: bytes) -> int:
    """The Poly1305 accumulator mod p before `+ s` (big integers)."""
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    acc = 0
    for i in range(0, len(msg), 16):
        blk = msg[i:i + 16]
        acc = ((acc + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r) % P1305
    return acc


def _round_div(a: int, b: int) -> int:
    return (2 * a + b) // (2 * b)


def _solve(a: int, w: int):
    """0 <= x < 2^96, 0 <= y < 2^88 with a*x + y == w (mod p), or None.  Lattice {(x, z): z == a*x mod p} with z weighted
    by 2^8, Lagrange-Gauss reduced, Babai rounding towards (x, z) = (2^95, w - 2^87); then y = w - z."""
    W = 1 << 8
    u, v = (1, a * W), (0, P1305 * W)

    def n2(q):
        return q[0] * q[0] + q[1] * q[1]

    if n2(u) > n2(v):
        u, v = v, u
    while True:                                         # Lagrange-Gauss: u shortest, v next
        m = _round_div(u[0] * v[0] + u[1] * v[1], n2(u))
        v = (v[0] - m * u[0], v[1] - m * u[1])
        if n2(v) >= n2(u):
            break
        u, v = v, u
    tx, tz = 1 << 95, (w - (1 << 87)) * W
    det = u[0] * v[1] - u[1] * v[0]                     # coordinates of the target in the basis (u, v), rounded
    cu = _round_div(tx * v[1] - tz * v[0], det) if det > 0 else _round_div(-(tx * v[1] - tz * v[0]), -det)
    cv = _round_div(u[0] * tz - u[1] * tx, det) if det > 0 else _round_div(-(u[0] * tz - u[1] * tx), -det)
    for du in (0, -1, 1):
        for dv in (0, -1, 1):
            x = (cu + du) * u[0] + (cv + dv) * v[0]
            z = ((cu + du) * u[1] + (cv + dv) * v[1]) // W
            y = w - z
            if 0 <= x < 1 << 96 and 0 <= y < 1 << 88 and (a * x + y - w) % P1305 == 0:
                return x, y
    return None


def craft_blob(key: bytes, nonce: bytes, residue: int):
    """A 55-byte blob nonce | ct | tag whose Poly1305 accumulator before `+ s` is == residue (mod p) and whose plaintext
    starts with "ESAL".  -> (blob, plaintext), or None when the solver finds no short enough solution.
    The MAC runs over c1 = ct[0:16] + 2^128, c2 = ct[16:27] zero-padded + 2^128 and the length block c3, so
    h = c1 r^3 + c2 r^2 + c3 r (mod p).  ct[0:4] is fixed by the magic; x = ct[4:16], y = ct[16:27] leave
    2^32 r x + y == (residue - h(x = y = 0)) / r^2 (mod p)."""
    otk = keystream(key, nonce, 0)[:32]
    ks1 = keystream(key, nonce, 1)
    r = int.from_bytes(otk[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    if r == 0:
        return None
    e = bytes(m ^ k for m, k in zip(b"ESAL", ks1[:4]))
    base = accumulator(otk, mac_input(e + b"\x00" * 23))
    r2inv = pow(r * r % P1305, -1, P1305)
    sol = _solve((r << 32) % P1305, (residue - base) * r2inv % P1305)
    if sol is None:
        return None
    x, y = sol
    ct = e + x.to_bytes(12, "little") + y.to_bytes(11, "little")
    assert accumulator(otk, mac_input(ct)) == residue % P1305
    plain = bytes(c ^ k for c, k in zip(ct, ks1[:27]))
    sealed = chacha20poly1305_encrypt(key, nonce, plain)
    assert sealed[:27] == ct and sealed[27:] == _aead_tag(key, nonce, b"", ct)
    return nonce + sealed, plain


class Vector:
    """One crafted blob: key, residue, blob, plaintext, expected counter (plaintext bytes 4..7, big endian), whether the
    final subtraction runs, whether (h mod p) + s carries past 2^128."""

    def __init__(self, key: bytes, residue: int, blob: bytes, plain: bytes):
        self.key, self.residue, self.blob, self.plain = key, residue, blob, plain
        self.nonce, self.ct, self.tag = blob[:12], blob[12:39], blob[39:]
        self.ctr = int.from_bytes(plain[4:8], "big")
        self.otk = keystream(key, self.nonce, 0)[:32]
        self.branch = residue in BRANCH_RESIDUES
        s = int.from_bytes(self.otk[16:], "little")
        self.wraps = (residue % (1 << 128)) + s >= 1 << 128


def crafted_vectors(key: bytes, *, per_residue: int = 2, seed: int = 0):
    """`per_residue` vectors for every residue of RESIDUES under `key`, nonces drawn from a seeded generator (a nonce whose
    solve fails is skipped)."""
    rng = np.random.default_rng([seed, *key[:8]])
    out = []
    for t in RESIDUES:
        got = 0
        while got < per_residue:
            c = craft_blob(key, rng.bytes(12), t)
            if c is not None:
                out.append(Vector(key, t, *c)); got += 1
    return out


def seal_rows(key: bytes, nonces: np.ndarray, plain: np.ndarray) -> np.ndarray:
    """SecureChannel.seal of many 27-byte plaintexts on the host: uint8 [n,12], [n,27] -> blobs uint8 [n,55].  The keystream
    is vectorised; each tag is primitives.poly1305_tag (big integers)."""
    n = len(nonces)
    ct = chacha20_xor(key, nonces, plain, 1)
    otk = _chacha_blocks(np.broadcast_to(np.frombuffer(key, "<u4"), (n, 8)), np.zeros(n, np.uint32),
                         np.ascontiguousarray(nonces).view("<u4").reshape(n, 3))[:, :32]
    out = np.empty((n, 55), np.uint8)
    out[:, :12] = nonces; out[:, 12:39] = ct
    for i in range(n):
        out[i, 39:] = np.frombuffer(poly1305_tag(otk[i].tobytes(), mac_input(ct[i].tobytes())), np.uint8)
    return out
