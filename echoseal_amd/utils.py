"""Host-side helpers with the reference's names (mirror of rtwm/utils.py).

Band plan and keyed hop (rtwm/utils.py:19-36), dB helpers (:40-48), Butterworth design and
resampling wrappers (:52-66), the AES-based PN stream (:83-132) and the 63-chip MLS (:135-145).
None of this is hot-path arithmetic; it produces the tables and the key/PN schedule the HIP
kernels consume.  The AES / HMAC code is our own (echoseal_amd.primitives) because neither
`cryptography` nor PyCryptodome is available where this runs.
"""
from __future__ import annotations

import hashlib
import hmac
import math
from dataclasses import dataclass
from typing import Tuple

import numpy as np
from scipy.signal import butter, resample_poly

from ._native import ES_RESAMPLE_RATE_MAX, ES_RESAMPLE_TABLE_MAX, ES_RSTREAM_TAIL
from .primitives import aes128_encrypt_blocks

BAND_PLAN: list[Tuple[int, int]] = [
    (4_000, 6_000),
    (8_000, 10_000),
    (16_000, 18_000),
    (18_000, 22_000),
]


def band_index(key: bytes, frame_ctr: int) -> int:
    """Index into BAND_PLAN for a frame counter: HMAC-SHA256(key, ctr_be32)[0] mod 4 (rtwm/utils.py:27-36).  Not memoised here: a
    process-wide cache would keep the secret hop key alive after its detector is gone (see BandHop)."""
    tag = hmac.new(bytes(key), int(frame_ctr).to_bytes(4, "big"), hashlib.sha256).digest()
    return tag[0] % len(BAND_PLAN)


class BandHop:
    """The hop schedule of ONE key, memoised per owner: the counter search of one verify() asks for several hundred counters, the same
    ones clip after clip (2 ms of HMACs per call on the host otherwise).  Lives and dies with the object that owns it (a
    WatermarkDetector), holds at most `limit` counters, and never leaves key material in module state."""

    def __init__(self, key: bytes, limit: int = 1 << 16) -> None:
        self._key, self._limit, self._memo = bytes(key), int(limit), {}

    def index(self, frame_ctr: int) -> int:
        c = int(frame_ctr)
        v = self._memo.get(c)
        if v is None:
            if len(self._memo) >= self._limit:
                self._memo.clear()
            v = self._memo[c] = band_index(self._key, c)
        return v

    def band(self, frame_ctr: int) -> tuple[int, int]:
        return BAND_PLAN[self.index(frame_ctr)]


def choose_band(key: bytes, frame_ctr: int) -> tuple[int, int]:
    return BAND_PLAN[band_index(key, frame_ctr)]


def db_to_lin(db: float) -> float:
    return 10.0 ** (db / 20.0)


def lin_to_db(lin: float) -> float:
    return 20.0 * np.log10(lin + 1e-12)


def butter_bandpass(lo: float, hi: float, fs: int, *, order: int = 4):
    nyq = 0.5 * fs
    return butter(order, [lo / nyq, hi / nyq], "band")


def resample_to(fs_target: int, audio: np.ndarray, fs_orig: int) -> tuple[np.ndarray, int]:
    if fs_orig == fs_target:
        return audio, fs_orig
    g = math.gcd(fs_orig, fs_target)
    return resample_poly(audio, fs_target // g, fs_orig // g), fs_target


def resampled_length(n_in: int, fs_orig: int, fs_target: int) -> int:
    """Samples resample_to returns for n_in samples: ceil(n_in * up / down) (scipy.signal.resample_poly)."""
    g = math.gcd(int(fs_orig), int(fs_target))
    return -(-int(n_in) * (int(fs_target) // g) // (int(fs_orig) // g))


def resample_plan(n_in: int, up: int, down: int, dtype):
    """Everything scipy.signal.resample_poly(x, up, down) does in Python before its compiled loop (SciPy 1.15: Kaiser-5.0
    `firwin` design of 20*max(up,down)+1 taps scaled by `up`, zero padding that centres the output, the kept output
    range) plus upfirdn's transposed / flipped polyphase layout.  -> (h_tf, taps per phase, up, down, first kept output,
    number of outputs, compute dtype), or None when the rates are equal.  The loop itself is es_resample_batch."""
    from scipy.signal import firwin
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    if up == down == 1:
        return None
    n_out = n_in * up
    n_out = n_out // down + bool(n_out % down)
    max_rate = max(up, down)
    half_len = 10 * max_rate
    h = firwin(2 * half_len + 1, 1.0 / max_rate, window=("kaiser", 5.0))
    if np.issubdtype(np.dtype(dtype), np.floating):
        h = h.astype(dtype)
    h *= up
    n_pre_pad = down - half_len % down
    n_post_pad = 0
    n_pre_remove = (half_len + n_pre_pad) // down

    def _output_len(len_h: int) -> int:
        nt = (n_in + (len_h + (-len_h % up)) // up - 1) * up
        return nt // down + (1 if nt % down > 0 else 0)

    while _output_len(len(h) + n_pre_pad + n_post_pad) < n_out + n_pre_remove:
        n_post_pad += 1
    h = np.concatenate((np.zeros(n_pre_pad, h.dtype), h, np.zeros(n_post_pad, h.dtype)))
    ctype = np.result_type(h.dtype, np.dtype(dtype), np.float32)
    padlen = len(h) + (-len(h) % up)
    hf = np.zeros(padlen, ctype)
    hf[: len(h)] = h
    h_tf = np.ascontiguousarray(hf.reshape(-1, up).T[:, ::-1].ravel())
    return h_tf, padlen // up, up, down, n_pre_remove, n_out, np.dtype(ctype)


def resample_geometry(n_in: int, up: int, down: int):
    """The integers of resample_plan without its filter: -> (up, down, taps per phase, first kept output, number of outputs) of the
    reduced pair, or None when the rates are equal.  Closed form of resample_plan's padding loop (the zeros appended until upfirdn's
    output is long enough), so that a rate pair can be judged before a filter of 20 * max(up, down) + 1 taps is designed."""
    g = math.gcd(int(up), int(down))
    up, down = int(up) // g, int(down) // g
    if up == down == 1:
        return None
    n_out = -(-int(n_in) * up // down)
    half_len = 10 * max(up, down)
    n_pre_pad = down - half_len % down
    y0 = (half_len + n_pre_pad) // down
    len_h = 2 * half_len + 1 + n_pre_pad
    # upfirdn returns ceil((n_in + c - 1) * up / down) outputs for c taps per phase: the smallest c that gives n_out + y0 of them
    need = n_out + y0
    c_min = -(-((need - 1) * down + 1) // up) - int(n_in) + 1
    return up, down, max(-(-len_h // up), c_min), y0, n_out


def resample_limits(n_in: int, fs_orig: int, fs_target: int) -> str | None:
    """What keeps es_resample_ragged_batch from conditioning a clip of n_in samples at fs_orig to fs_target, in words, or None when
    it can: the kernel steps through a tile in 32 bits and writes nothing for a record whose reduced up, down or taps per phase are
    above ES_RESAMPLE_RATE_MAX or whose polyphase table has more than ES_RESAMPLE_TABLE_MAX values (include/echoseal_hip.h)."""
    g = math.gcd(int(fs_orig), int(fs_target))
    up, down = int(fs_target) // g, int(fs_orig) // g
    if max(up, down) > ES_RESAMPLE_RATE_MAX:                                # (before the geometry: its integers are then of no use)
        return f"up = {up}, down = {down}: above {ES_RESAMPLE_RATE_MAX}"
    geo = resample_geometry(n_in, up, down)
    if geo is None:
        return None
    hpp = geo[2]
    if hpp > ES_RESAMPLE_RATE_MAX:
        return f"{hpp} taps per phase: above {ES_RESAMPLE_RATE_MAX}"
    if up * hpp > ES_RESAMPLE_TABLE_MAX:
        return f"a polyphase table of {up} x {hpp} values: above {ES_RESAMPLE_TABLE_MAX}"
    return None


@dataclass
class StreamResamplePlan:
    """What a live stream at another rate is conditioned with (stream_resample_plan): the reduced pair, resample_geometry's first kept
    output y0 (a property of the pair alone), the canonical taps per phase hpp = ceil((2 half_len + 1 + n_pre_pad) / up) -- no post padding,
    which only appends zero taps -- and the float32 polyphase table in resample_plan's transposed, flipped layout [up * hpp].  Equal
    rates: up = down = 1, y0 = hpp = 0 and an empty table (the stream is copied)."""
    up: int
    down: int
    y0: int
    hpp: int
    h_tf: np.ndarray


STREAM_TAPS_MAX = ES_RSTREAM_TAIL                                           # 256: a stream's tail row holds the 255 samples before its chunk


def stream_geometry(fs_in: int, fs_target: int):
    """The integers of stream_resample_plan without its filter: -> (up, down, y0, hpp, n_pre_pad) of the reduced pair; equal rates:
    (1, 1, 0, 0, 0).  Refused with a ValueError that names the rate: what resample_limits refuses, and a pair that needs more than 256
    taps per phase (the tail row serves 255 samples before the chunk; 384 kHz -> 48 kHz needs 169)."""
    fs_in, fs_target = int(fs_in), int(fs_target)
    if fs_in < 1 or fs_target < 1:
        raise ValueError(f"a stream at {fs_in} Hz -> {fs_target} Hz: rates are positive")
    why = resample_limits(0, fs_in, fs_target)
    if why is not None:
        raise ValueError(f"a stream at {fs_in} Hz -> {fs_target} Hz is outside what the device conditions: {why}")
    g = math.gcd(fs_in, fs_target)
    up, down = fs_target // g, fs_in // g
    if up == down:
        return 1, 1, 0, 0, 0
    half_len = 10 * max(up, down)
    n_pre_pad = down - half_len % down
    hpp = -(-(2 * half_len + 1 + n_pre_pad) // up)
    if hpp > STREAM_TAPS_MAX:
        raise ValueError(f"a stream at {fs_in} Hz -> {fs_target} Hz needs {hpp} taps per phase: more than the {STREAM_TAPS_MAX} a live "
                         "stream's tail serves (condition such a feed before it is pushed)")
    return up, down, (half_len + n_pre_pad) // down, hpp, n_pre_pad


def stream_resample_plan(fs_in: int, fs_target: int) -> StreamResamplePlan:
    """The plan that conditions a live stream at fs_in to fs_target chunk by chunk; refusals are stream_geometry's."""
    from scipy.signal import firwin
    up, down, y0, hpp, n_pre_pad = stream_geometry(fs_in, fs_target)
    if up == down:
        return StreamResamplePlan(1, 1, 0, 0, np.zeros(0, np.float32))
    half_len = 10 * max(up, down)
    h = firwin(2 * half_len + 1, 1.0 / max(up, down), window=("kaiser", 5.0)).astype(np.float32)        # as resample_plan for float32
    h *= up
    hf = np.zeros(up * hpp, np.float32)
    hf[n_pre_pad: n_pre_pad + h.size] = h
    return StreamResamplePlan(up, down, y0, hpp, np.ascontiguousarray(hf.reshape(-1, up).T[:, ::-1].ravel()))


def finalized(n, up: int, down: int, y0: int):
    """F(n) = max(0, (n up - 1) // down - y0 + 1): how many leading outputs of resample_poly(X[:n], up, down) no later sample changes --
    output k is final once its newest input sample, ((y0 + k) down) // up, has arrived.  n: a scalar (-> int) or an array (-> int64;
    n * up must stay below 2^63)."""
    up, down, y0 = int(up), int(down), int(y0)
    if np.ndim(n) == 0:
        return max(0, (int(n) * up - 1) // down - y0 + 1)
    return np.maximum((np.asarray(n, dtype=np.int64) * up - 1) // down - y0 + 1, 0)


def stream_position_limit(up: int) -> int:
    """The most samples a stream with this `up` may have received: n * up stays below 2^62 (the kernels' 64-bit arithmetic)."""
    return ((1 << 62) - 1) // int(up)


@dataclass
class ConditionPlan:
    """Host side of es_resample_ragged_batch for clips of one sample type: desc int64 [R, 8] = (offset of the clip in the flat sample
    pool, n_in, up, down, offset of its filter in `filters`, taps per phase, first kept output, n_out) -- words 2, 3 and 5..7 and the
    filter are resample_plan's; an identity record (equal rates) has up = down = 1 and no filter; `filters`: one copy per distinct
    filter, in the compute type (float64 for float64 samples, else float32); n_out int64 [R] = the resampled lengths."""
    desc: np.ndarray
    filters: np.ndarray
    n_out: np.ndarray


def condition_plan(lengths, fs_list, fs_target: int, dtype) -> ConditionPlan:
    """The descriptors that condition clips of `lengths` samples at rates `fs_list` (one rate, or one per clip) to fs_target in one launch.
    Clips lie back to back in the sample pool, in input order.  int16 samples are resampled as float32 (x / 32768, resample_to's input
    after soundfile.read); filters are compared by their bytes, not by the rate pair, so two rate pairs with one table share it.
    A clip whose reduced rate pair is outside the kernel's limits (resample_limits) is refused with a ValueError that names it, before
    any filter is designed: the kernel would write nothing for it."""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.int16), np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("condition_plan: samples must be int16, float32 or float64")
    ctype = np.dtype(np.float64) if dtype == np.float64 else np.dtype(np.float32)
    n = [int(v) for v in lengths]
    fs = [int(f) for f in fs_list] if isinstance(fs_list, (list, tuple, np.ndarray)) else [int(fs_list)] * len(n)
    if len(fs) != len(n) or any(v < 0 for v in n) or any(f < 1 for f in fs) or int(fs_target) < 1:
        raise ValueError("condition_plan: one positive rate per clip, no negative length")
    for r, (n_in, f) in enumerate(zip(n, fs)):
        why = resample_limits(n_in, f, int(fs_target))
        if why is not None:
            raise ValueError(f"condition_plan: clip {r} ({f} Hz -> {int(fs_target)} Hz) is outside what the device conditions: {why}")
    desc = np.zeros((len(n), 8), np.int64)
    pool: list[np.ndarray] = []
    seen: dict[bytes, int] = {}
    at = off = 0
    for r, (n_in, f) in enumerate(zip(n, fs)):
        plan = resample_plan(n_in, int(fs_target), f, ctype)
        if plan is None:
            desc[r] = (off, n_in, 1, 1, 0, 0, 0, n_in)
        else:
            h_tf, hpp, up, down, y0, n_out, ct = plan
            assert ct == ctype
            key = h_tf.tobytes()
            if key not in seen:
                seen[key] = at
                pool.append(h_tf)
                at += h_tf.size
            desc[r] = (off, n_in, up, down, seen[key], hpp, y0, n_out)
        off += n_in
    filters = np.concatenate(pool) if pool else np.zeros(0, ctype)
    return ConditionPlan(desc, filters, desc[:, 7].copy())


class StreamPRNG:
    """AES-128 block stream: block j of frame c is AES(sub_key, (c << 64 | j) big-endian)."""

    def __init__(self, master_key: bytes):
        self._sub_key = hashlib.blake2s(master_key, digest_size=16, person=b"EchoSeal").digest()

    @property
    def sub_key(self) -> bytes:
        return self._sub_key

    def blocks(self, frame_ctrs, n_blocks: int) -> np.ndarray:
        """Keystream for many counters at once -> uint8 [len(frame_ctrs), 16 * n_blocks]."""
        ctrs = np.asarray(frame_ctrs, dtype=np.uint64).reshape(-1)
        inp = np.zeros((ctrs.size, n_blocks, 16), dtype=np.uint8)
        inp[:, :, 0:8] = ctrs.astype(">u8").view(np.uint8).reshape(-1, 1, 8)
        inp[:, :, 8:16] = np.arange(n_blocks, dtype=">u8").view(np.uint8).reshape(1, n_blocks, 8)
        return aes128_encrypt_blocks(self._sub_key, inp).reshape(ctrs.size, 16 * n_blocks)

    def bytes(self, frame_ctr: int, n: int = 64) -> bytes:
        return self.blocks([frame_ctr], (n + 15) // 16)[0, :n].tobytes()


def pn_bits(prng: StreamPRNG, frame_ctr: int, n_bits: int) -> np.ndarray:
    data = prng.bytes(frame_ctr, (n_bits + 7) // 8)
    return np.unpackbits(np.frombuffer(data, dtype="u1"))[:n_bits]


def mseq_63() -> np.ndarray:
    """63-chip maximal-length sequence: 6-stage LFSR, feedback bit5 ^ bit4, seed 0b111111."""
    state = 0b111111
    out = np.empty(63, dtype=np.uint8)
    for i in range(63):
        out[i] = state & 1
        fb = ((state >> 5) ^ (state >> 4)) & 1
        state = ((state << 1) & 0b111111) | fb
    return out
