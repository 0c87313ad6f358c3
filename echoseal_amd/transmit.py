"""TxChain: the batched EchoSeal transmit chain, the half of RxEngine that makes watermarked audio.  Host code over the C ABI, as
engine.py is; each method mirrors one stage of the reference embedder:

    aead_seal / seal_keyed              rtwm/crypto.py:33-37     (SecureChannel.seal)
    make_frames / make_frames_keyed     rtwm/embedder.py:78-141  (payload -> polar code -> header, PN spread, band-pass)
    mix / mix_ragged                    rtwm/embedder.py:44-75   (process: the level mix of every block)
    plaintexts of fresh payloads        rtwm/embedder.py:153-168 (_build_payload)

`embed` (recordings of one key and one length), `embed_batch` (clips of any lengths, each under its own key) and `embed_step` (one tick of live
streams, rtwm/embedder.py:34-36,44-75) string them together; they share the private helpers below and the host layouts embed_layout / stream_layout.
"""
from __future__ import annotations

import secrets
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as nat
from .scan import ragged_buckets
from .utils import db_to_lin, mseq_63


@dataclass
class EmbedResult:
    audio: torch.Tensor        # [R,n] float32 watermarked recordings ([n] for 1-D input)
    ctr: np.ndarray            # [R] int64: counter of the next frame to generate (WatermarkEmbedder.frame_ctr after the same process() calls)
    off: np.ndarray            # [R] int64: chips of the current frame already used (0 = nothing pending)
    tail: torch.Tensor         # [R,1215] float32: the current frame; its chips from `off` on are what process() keeps in its buffer
    scale: torch.Tensor | None = None   # [R, ceil(n / block)] float64 gain of every block (want_scale)


@dataclass
class EmbedClip:
    """One clip of RxEngine.embed_batch."""
    audio: torch.Tensor        # [len] float32, the watermarked clip (a view into its launch's padded tensor)
    ctr: int                   # counter of the next frame to generate (WatermarkEmbedder.frame_ctr after process() over the clip)
    off: int                   # chips of the current frame already used (0 = nothing pending)
    scale: torch.Tensor | None = None   # [ceil(len / block)] float64 gain of every block (want_scale)


# Padded samples (clips x longest clip of the launch) one embed_batch launch may hold.  Bytes per padded sample: the float32 row that
# is mixed in place, 4, and its staging copy on the host, not on the device; per REAL sample, roughly one chip each: the frames
# float32, 4, the band-pass workspace float64, 8, code bits 1024 / 1215 and PN rows 152 / 1215, 1 -- so at most 17 bytes per padded
# sample and 2^26 samples stay under 1.2 GB.  A memory bound, not a tuned value.
EMBED_ROW_SAMPLES = 1 << 26
_PRE8 = np.packbits(np.concatenate((mseq_63().astype(np.uint8), np.zeros(1, np.uint8)))).tobytes()      # the frame generators' preamble


@dataclass
class EmbedLayout:
    """Where the frames of a batch of clips lie (embed_layout)."""
    nf: np.ndarray             # [R] int64 frames clip r generates: ceil(len_r / 1215)
    clip: np.ndarray           # [F] int64 clip of each frame of the flat frame list (clip by clip, counters ascending)
    ctr: np.ndarray            # [F] int64 counter of each frame: (ctr0[clip] + k) mod 2^32
    chip_base: np.ndarray      # [R] int64 = 1215 * index of clip r's first frame in the flat list
    chip_cnt: np.ndarray       # [R] int64 = 1215 * nf[r]
    ctr_next: np.ndarray       # [R] int64 counter after the clip: (ctr0 + nf) mod 2^32
    off: np.ndarray            # [R] int64 chips of the last frame already used: len mod 1215


def _rows_ctr0(ctr0, n: int, what: str = "clip") -> np.ndarray:
    """Start counters, a scalar for all rows or one value per row -> int64 [n], not yet reduced mod 2^32."""
    c0 = np.array(ctr0, dtype=np.int64).reshape(-1) if np.ndim(ctr0) else np.full(n, int(ctr0), np.int64)
    if c0.size != n:
        raise ValueError(f"ctr0: a scalar or one value per {what}")
    return c0


def embed_layout(lengths, ctr0) -> EmbedLayout:
    """The frames a batch of clips generates, as WatermarkEmbedder.process does whatever the block size (rtwm/embedder.py:44-62: a
    frame is made whenever the chip buffer runs short): clip r of lengths[r] samples starting at counter ctr0[r] (a scalar serves
    every clip) makes ceil(lengths[r] / 1215) frames of consecutive counters mod 2^32.  A pure host function."""
    FL = nat.ES_FRAME_LEN
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if n.size and n.min() < 0:
        raise ValueError("negative clip length")
    c0 = _rows_ctr0(ctr0, n.size) & 0xFFFFFFFF
    nf = (n + FL - 1) // FL
    first = np.cumsum(nf) - nf
    clip = np.repeat(np.arange(n.size, dtype=np.int64), nf)
    k = np.arange(int(nf.sum()), dtype=np.int64) - first[clip]
    return EmbedLayout(nf, clip, (c0[clip] + k) & 0xFFFFFFFF, first * FL, nf * FL, (c0 + nf) & 0xFFFFFFFF, n % FL)


def embed_launches(lengths, ctr0, budget: int | None = None) -> list:
    """How embed_batch cuts a batch into launches: scan.ragged_buckets(lengths, 1, EMBED_ROW_SAMPLES) (clips sorted by length, taken
    while clips x longest clip stays within the budget), each launch with the frame layout of its own clips.  -> [(indices into the
    batch, EmbedLayout of those clips in that order)]; results go back to the indices, so the caller sees input order."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    c0 = _rows_ctr0(ctr0, n.size)
    return [(idx, embed_layout(n[idx], c0[idx])) for idx in ragged_buckets(n, 1, EMBED_ROW_SAMPLES if budget is None else budget)]


@dataclass
class StreamLayout:
    """Where the frames of one tick of live streams lie (stream_layout)."""
    start: np.ndarray          # [R] int64 position of the chunk's first chip in the row [pending frame | new frames]: off, or 1215 where off == 0
    nf: np.ndarray             # [R] int64 new frames chunk r generates: ceil((start + len) / 1215) - 1
    rec: np.ndarray            # [F] int64 chunk of each frame of the flat frame list (chunk by chunk, counters ascending)
    ctr: np.ndarray            # [F] int64 counter of each frame: (ctr[rec] + k) mod 2^32
    chip_base: np.ndarray      # [R] int64 = 1215 * index of chunk r's first new frame in the flat list
    chip_cnt: np.ndarray       # [R] int64 = 1215 * nf[r]
    ctr_next: np.ndarray       # [R] int64 the stream's counter after the chunk: (ctr + nf) mod 2^32
    off_next: np.ndarray       # [R] int64 chips of the frame the stream then stands in already used: (start + len) mod 1215


def stream_layout(off, ctr, lengths) -> StreamLayout:
    """The frames one tick generates, as successive WatermarkEmbedder.process calls do (rtwm/embedder.py:44-62: a frame is made whenever
    the chip buffer runs short): chunk r of lengths[r] samples continues a stream that has used off[r] chips of the frame it stands in
    (0 = nothing pending) and makes its next frame under counter ctr[r].  It first uses up the 1215 - off[r] pending chips, then
    ceil((start + len) / 1215) - 1 new frames of consecutive counters mod 2^32 -- what `embed` computes as `new` with carry=.  A pure
    host function."""
    FL = nat.ES_FRAME_LEN
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    off = np.asarray(off, dtype=np.int64).reshape(-1)
    if off.shape != n.shape:
        raise ValueError("off, ctr, lengths: one entry per chunk")
    c0 = _rows_ctr0(ctr, n.size, "chunk") & 0xFFFFFFFF
    if n.size and n.min() < 0:
        raise ValueError("negative chunk length")
    if off.size and (off.min() < 0 or off.max() >= FL):
        raise ValueError(f"off outside [0, {FL})")
    start = np.where(off > 0, off, FL)
    end = start + n
    nf = (end + FL - 1) // FL - 1
    first = np.cumsum(nf) - nf
    rec = np.repeat(np.arange(n.size, dtype=np.int64), nf)
    k = np.arange(int(nf.sum()), dtype=np.int64) - first[rec]
    return StreamLayout(start, nf, rec, (c0[rec] + k) & 0xFFFFFFFF, first * FL, nf * FL, (c0 + nf) & 0xFFFFFFFF, end % FL)


@dataclass
class StreamTable:
    """The state of S live streams on the device (RxEngine.open_streams); RxEngine.embed_step marks chunks of any of them and moves
    them on.  Row s is what EmbedResult.ctr / off / tail are for one stream."""
    ring: "KeyRing"            # (engine.KeyRing)
    key: torch.Tensor          # [S] int32 ring row of each stream
    ctr: torch.Tensor          # [S] int64 counter of the next frame to generate, 0 .. 2^32 - 1
    off: torch.Tensor          # [S] int64 chips of the current frame already used (0 = nothing pending)
    tail: torch.Tensor         # [S, 1215] float32 the frame the stream stands in
    nonce8: torch.Tensor       # [S, 8] uint8 session nonce, fixed when the stream is opened
    key_host: np.ndarray       # [S] int64 host copy of `key`
    ctr_host: np.ndarray       # [S] int64 host mirror of `ctr`: a tick lays out its frames without a copy from the device
    off_host: np.ndarray       # [S] int64 host mirror of `off`
    live: np.ndarray           # [S] bool; False: a closed row, free for add_streams

    @property
    def n(self) -> int:
        return int(self.live.size)


# ---------------------------------------------------------------------- host steps the embeds share (no engine needed)
def _clips_1d(seq, what: str) -> list:
    """Clips or chunks, host arrays or tensors -> a list of 1-D float32 tensors."""
    ts = [c if torch.is_tensor(c) else torch.from_numpy(np.ascontiguousarray(c)) for c in seq]
    if any(t.dim() != 1 or t.dtype != torch.float32 for t in ts):
        raise ValueError(f"{what} must be 1-D float32 arrays or tensors")
    return ts


def _clip_payloads(payloads, nf: np.ndarray, refusal: str) -> list:
    """The caller's sealed payloads, one uint8 [>= nf[r], 55] per clip (None serves a clip of no frames) -> host arrays."""
    payloads = [np.zeros((0, 55), np.uint8) if p is None else np.asarray(p.cpu().numpy() if torch.is_tensor(p) else p) for p in payloads]
    if len(payloads) != nf.size or any(p.dtype != np.uint8 or p.ndim != 2 or p.shape[1] != 55 or p.shape[0] < f for p, f in zip(payloads, nf)):
        raise ValueError(refusal)
    return payloads


def _session_nonces(session_nonces, n: int, refusal: str) -> np.ndarray:
    """n session nonces of 8 bytes, the caller's or fresh ones -> uint8 [n, 8]."""
    sns = [secrets.token_bytes(8) for _ in range(n)] if session_nonces is None else [bytes(sn) for sn in session_nonces]
    if len(sns) != n or any(len(sn) != 8 for sn in sns):
        raise ValueError(refusal)
    return np.frombuffer(b"".join(sns), np.uint8).reshape(n, 8).copy()


def _fresh_plain(ctr_host: np.ndarray, nonce8_rows=None):
    """What a fresh payload seals (rtwm/embedder.py:153-168): plaintext b"ESAL" | ctr_be32 | nonce8 | pad11 per counter of ctr_host
    (int64 [F], already mod 2^32), pad bytes and the 12-byte AEAD nonces from `secrets`.  nonce8_rows uint8 [F, 8] (or one row for
    all); None leaves bytes 8:16 zero for the caller to fill.  -> (nonces uint8 [F,12], plain uint8 [F,27]), host arrays."""
    F = ctr_host.size
    plain = np.empty((F, 27), np.uint8)
    plain[:, :4] = np.frombuffer(b"ESAL", np.uint8)
    plain[:, 4:8] = ctr_host.astype(">u4").view(np.uint8).reshape(-1, 4)
    plain[:, 8:16] = 0 if nonce8_rows is None else nonce8_rows
    plain[:, 16:27] = np.frombuffer(secrets.token_bytes(11 * F), np.uint8).reshape(-1, 11)
    return np.frombuffer(secrets.token_bytes(12 * F), np.uint8).reshape(-1, 12).copy(), plain


def _clip_results(rows: torch.Tensor, scale, idx, lengths: np.ndarray, block: int, ctr_next: np.ndarray, off_next: np.ndarray, out: list) -> None:
    """out[idx[j]] = the EmbedClip of row j of a launch: its first lengths[idx[j]] samples and the gains of their blocks."""
    for j, i in enumerate(idx):
        n_i = int(lengths[i])
        out[i] = EmbedClip(rows[j, :n_i], int(ctr_next[j]), int(off_next[j]), None if scale is None else scale[j, :(n_i + block - 1) // block])


class TxChain:
    """The transmit methods of RxEngine (a mixin: it has no state of its own).  From the engine it uses _call, device, _dev, _ctr_dev,
    _key_dev, _key_host, keyring, polar_encode, schedule and schedule_keyed."""

    # ------------------------------------------------------------------ device steps the entry points share
    def _seal_args(self, nonces, plain):
        """AEAD nonces and plaintexts on the device, checked -> (nonces, plain, n, blobs uint8 [n,55] to be written)."""
        nonces = self._dev(nonces, torch.uint8); plain = self._dev(plain, torch.uint8)
        if nonces.dim() != 2 or nonces.shape[1] != 12 or plain.shape != (nonces.shape[0], 27):
            raise ValueError("nonces must be [n,12] and plain [n,27]")
        return nonces, plain, nonces.shape[0], torch.empty((nonces.shape[0], 55), dtype=torch.uint8, device=self.device)

    def _frame_args(self, ctrs, payloads):
        """What a frame generator takes: its inputs, checked -> (counters int32 [B], B, payloads uint8 [B,55] on the device), and its
        buffers -> (packed preamble, band-pass workspace float64 [B,1215], frames float32 [B,1215] to be written)."""
        cd = self._ctr_dev(ctrs).reshape(-1)
        B = cd.numel()
        payloads = self._dev(payloads, torch.uint8)
        if payloads.shape != (B, 55):
            raise ValueError("payloads must be uint8 [B,55], one per counter")
        return (cd, B, payloads), (_PRE8, torch.empty((B, 1215), dtype=torch.float64, device=self.device),
                                   torch.empty((B, 1215), dtype=torch.float32, device=self.device))

    def _mix_out(self, x: torch.Tensor, out, block, want_scale: bool):
        """What a mix of the rows x [R, n] writes -> (out: the caller's, checked, or new; block as int; scale float64 [R, ceil(n / block)] or None)."""
        if out is not None and (out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float32 tensor of x's shape")
        block = int(block)
        blocks = (x.shape[1] + block - 1) // block if block >= 1 else 0
        scale = torch.empty((x.shape[0], blocks), dtype=torch.float64, device=self.device) if want_scale else None
        return torch.empty_like(x) if out is None else out, block, scale

    def _pad_rows(self, clips: list, idx, lengths: np.ndarray):
        """The zero-padded rows of one launch -> (x float32 [len(idx), stride] on the device, stride = the longest clip rounded up to 4).
        Host clips: one staging array, one copy; with clips on the device the rows are filled there."""
        stride = (int(lengths[idx].max()) + 3) // 4 * 4
        host = all(not c.is_cuda for c in clips)
        x = np.zeros((len(idx), stride), np.float32) if host else torch.zeros((len(idx), stride), dtype=torch.float32, device=self.device)
        for j, i in enumerate(idx):
            x[j, :lengths[i]] = clips[i].numpy() if host else clips[i].to(self.device)
        return (torch.from_numpy(x).to(self.device) if host else x), stride

    def _launches(self, clips: list, lengths: np.ndarray, ctr: np.ndarray, off: np.ndarray, want_scale: bool, out: list):
        """The cut into launches, scan.ragged_buckets(lengths, 1, EMBED_ROW_SAMPLES): yields (idx, x, stride), the clips of a launch and their
        padded rows.  Clips of no samples launch nothing and are settled here: out[i] = no audio, no gains, ctr[i] and off[i] as they stand."""
        for idx in ragged_buckets(lengths, 1, EMBED_ROW_SAMPLES):
            if int(lengths[idx].max()):
                yield (idx,) + self._pad_rows(clips, idx, lengths)
                continue
            for i in idx:
                out[i] = EmbedClip(torch.empty(0, dtype=torch.float32, device=self.device), int(ctr[i]), int(off[i]),
                                   torch.empty(0, dtype=torch.float64, device=self.device) if want_scale else None)

    def _launch_blobs(self, ring, kf_d: torch.Tensor, ctr_d: torch.Tensor, ctr_host: np.ndarray, payloads, idx, nf, seed, nonce8) -> torch.Tensor:
        """The sealed blobs uint8 [F,55] of one launch's frames (keys kf_d, counters ctr_d = ctr_host): the first nf[j] of the caller's payloads[idx[j]],
        or with seed= the bytes of `synthetic_frames`, or fresh plaintexts, sealed under each frame's key.  nonce8: the session nonce of every
        frame, host uint8 [F, 8], or (device table [S, 8], device rows [F]): gathered on the device, nothing comes to the host."""
        if payloads is not None:
            return torch.from_numpy(np.concatenate([payloads[i][:f] for i, f in zip(idx, nf)])).to(self.device)
        if seed is not None:
            nonces, plain = self._synthetic_plain(ctr_d, seed)
        else:
            on_device = isinstance(nonce8, tuple)
            nonces, plain = (torch.from_numpy(a) for a in _fresh_plain(ctr_host, None if on_device else nonce8))
            if on_device:
                plain = plain.to(self.device)
                plain[:, 8:16] = nonce8[0][nonce8[1]]
        return self.seal_keyed(ring, kf_d, nonces, plain)

    # ------------------------------------------------------------------ seal, frames
    def aead_seal(self, key32: bytes, nonces: torch.Tensor, plain: torch.Tensor) -> torch.Tensor:
        """SecureChannel.seal for a batch of 27-byte plaintexts (rtwm/crypto.py:33-37): nonces uint8 [n,12],
        plain uint8 [n,27] -> blobs uint8 [n,55] on the device."""
        if len(key32) != 32:
            raise ValueError("AEAD key must be 32 bytes")
        nonces, plain, n, blobs = self._seal_args(nonces, plain)
        self._call("es_aead_seal_batch", bytes(key32), nonces, plain, n, blobs)
        return blobs

    def seal_keyed(self, ring, key_idx, nonces: torch.Tensor, plain: torch.Tensor) -> torch.Tensor:
        """`aead_seal` with the AEAD key of ring row key_idx[i] per blob (es_aead_seal_keyed_batch): nonces uint8 [n,12],
        plain uint8 [n,27] -> blobs uint8 [n,55].  A device key index outside the ring gives a zero blob."""
        nonces, plain, n, blobs = self._seal_args(nonces, plain)
        kd = self._key_dev(ring, key_idx, n)
        if n and ring.n == 0:
            raise ValueError("records but an empty key ring")
        self._call("es_aead_seal_keyed_batch", ring.ring, ring.n, kd, nonces, plain, n, blobs)
        return blobs

    def make_frames(self, sec, band_key32: bytes, ctrs, payloads: torch.Tensor) -> torch.Tensor:
        """Batch of transmitted frames on the device (WatermarkEmbedder.make_frames, rtwm/embedder.py:78-141):
        payloads uint8 [B,55] (already sealed) under frame counters `ctrs` -> float32 [B,1215].  `sec` is the
        SecureChannel (PN sub-key, header PN), band_key32 the hop key."""
        (cd, B, payloads), (pre8, y_ws, frames) = self._frame_args(ctrs, payloads)
        code = self.polar_encode(payloads)
        pn, band = self.schedule(sec._prng.sub_key, band_key32, cd.to(torch.int64) & 0xFFFFFFFF)
        hdr16 = np.packbits(sec.pn_bits(0, 128)).tobytes()
        self._call("es_tx_frames_batch", code, pn, band, cd, pre8, hdr16, B, y_ws, frames)
        return frames

    def make_frames_keyed(self, ring, key_idx, ctrs, payloads: torch.Tensor) -> torch.Tensor:
        """`make_frames` for frames of several keys: frame i carries payloads[i] (uint8 [B,55], already sealed) under counter ctrs[i]
        and the key of ring row key_idx[i] -> float32 [B,1215] (es_polar_encode_batch, es_schedule_keyed_batch,
        es_tx_frames_keyed_batch: nothing is derived or copied from the host)."""
        (cd, B, payloads), (pre8, y_ws, frames) = self._frame_args(ctrs, payloads)
        kd = self._key_dev(ring, key_idx, B)
        if B and ring.n == 0:
            raise ValueError("records but an empty key ring")
        code = self.polar_encode(payloads)
        pn, band = self.schedule_keyed(ring, kd, cd.to(torch.int64) & 0xFFFFFFFF)
        self._call("es_tx_frames_keyed_batch", code, pn, band, cd, pre8, ring.ring, ring.n, kd, B, y_ws, frames)
        return frames

    def synthetic_frames(self, key32: bytes, ctr0: int, n: int, *, seed: int = 20260101):
        """The benchmark workloads' frames for counters ctr0 .. ctr0+n-1, made wholly on the device (SURVEY 8d:
        plaintext b"ESAL" | ctr_be32 | nonce8 | pad11 sealed with a 12-byte nonce, random bytes from a seeded torch
        generator, then `make_frames`).  -> (frames float32 [n,1215], payloads uint8 [n,55]).  Input synthesis for
        configs 3 and 4, where 65 536 .. 2^20 frames would take the host embedder minutes."""
        from .crypto import SecureChannel
        sec = SecureChannel(key32)
        ctr = torch.arange(ctr0, ctr0 + n, dtype=torch.int64, device=self.device)
        payloads = self._synthetic_payloads(sec, ctr, seed)
        return self.make_frames(sec, key32, ctr, payloads), payloads

    def _synthetic_payloads(self, sec, ctr: torch.Tensor, seed: int) -> torch.Tensor:
        """Sealed payloads uint8 [len(ctr),55] of `synthetic_frames` for the int64 device counters `ctr`."""
        nonces, plain = self._synthetic_plain(ctr, seed)
        return self.aead_seal(sec._aead._key, nonces, plain)

    def _synthetic_plain(self, ctr: torch.Tensor, seed: int):
        """What `_synthetic_payloads` seals: -> (nonces uint8 [n,12], plaintexts uint8 [n,27]) of the int64 device counters `ctr`."""
        n = ctr.numel()
        # 31 random bytes per frame from a counter-based hash of (seed, ctr, byte index), so that a frame does not
        # depend on how the counter range is cut into batches or shards (32-bit multiply-xorshift rounds in int64)
        h = (ctr[:, None] * 31 + torch.arange(31, dtype=torch.int64, device=self.device)[None, :] + (int(seed) & 0xFFFFFF) * 1_000_003) & 0xFFFFFFFF
        for _ in range(3):
            h = (h * 0x45D9F3B) & 0xFFFFFFFF
            h = h ^ (h >> 16)
        rnd = (h & 0xFF).to(torch.uint8)
        plain = torch.empty((n, 27), dtype=torch.uint8, device=self.device)
        plain[:, :4] = torch.tensor(list(b"ESAL"), dtype=torch.uint8, device=self.device)
        for k in range(4):
            plain[:, 4 + k] = ((ctr >> (8 * (3 - k))) & 0xFF).to(torch.uint8)
        plain[:, 8:27] = rnd[:, :19]
        return rnd[:, 19:31].contiguous(), plain

    # ------------------------------------------------------------------ level mix: frames -> watermarked recordings
    def mix(self, x: torch.Tensor, chips: torch.Tensor, *, block: int = 1024, chip_off=None, target_rel_db: float = -10.0,
            floor_rel_dbfs: float = -35.0, want_scale: bool = False, out: torch.Tensor | None = None):
        """WatermarkEmbedder.process (rtwm/embedder.py:44-75) for every `block`-sized slice of every recording, bit for bit
        (es_mix_batch): x float32 [R, n]; chips float32 [R, stride], row r the chip stream of recording r (frames of consecutive
        counters back to back); sample t takes chips[r, chip_off[r] + t] (chip_off: int64 [R], None = 0).  out=x mixes in place.
        -> marked audio [R, n]; want_scale: (audio, scale float64 [R, ceil(n / block)])."""
        if x.dim() != 2 or chips.dim() != 2 or x.dtype != torch.float32 or chips.dtype != torch.float32 or chips.shape[0] != x.shape[0]:
            raise ValueError("x must be float32 [R, n] and chips float32 [R, stride]")
        x = x.contiguous(); chips = chips.contiguous()
        R, n = x.shape
        if chip_off is not None:
            chip_off = self._dev(chip_off, torch.int64).reshape(-1)
            if chip_off.numel() != R:
                raise ValueError("chip_off: one offset per recording")
        out, block, scale = self._mix_out(x, out, block, want_scale)
        self._call("es_mix_batch", x, R, n, block, chips, chips.shape[1], chip_off, db_to_lin(target_rel_db), db_to_lin(floor_rel_dbfs), out, scale)
        return (out, scale) if want_scale else out

    def mix_ragged(self, x: torch.Tensor, lens, chips: torch.Tensor, chip_base, chip_cnt, *, block: int = 1024, target_rel_db: float = -10.0,
                   floor_rel_dbfs: float = -35.0, want_scale: bool = False, out: torch.Tensor | None = None):
        """`mix` for recordings of unequal length (es_mix_ragged_batch): x float32 [R, stride], record r = x[r, :lens[r]]; chips ONE flat
        float32 pool, sample t of record r takes chips[chip_base[r] + t], reads clamped to the record's chip_cnt[r] chips (lens,
        chip_base, chip_cnt: int64 [R]).  Every block of a record is mixed as `mix` mixes the record alone.  out[r, lens[r]:] and the
        scales of block slots past a record's end are NOT written: give `out` (out=x mixes in place) to decide what they hold.
        -> marked audio [R, stride]; want_scale: (audio, scale float64 [R, ceil(stride / block)])."""
        if x.dim() != 2 or x.dtype != torch.float32 or chips.dtype != torch.float32:
            raise ValueError("x must be float32 [R, stride] and chips a float32 pool")
        x = x.contiguous(); chips = chips.contiguous().reshape(-1)
        R, n = x.shape
        lens, chip_base, chip_cnt = (self._dev(v, torch.int64).reshape(-1) for v in (lens, chip_base, chip_cnt))
        if lens.numel() != R or chip_base.numel() != R or chip_cnt.numel() != R:
            raise ValueError("lens, chip_base, chip_cnt: one entry per recording")
        out, block, scale = self._mix_out(x, out, block, want_scale)
        self._call("es_mix_ragged_batch", x, R, n, lens, block, chips, chips.numel(), chip_base, chip_cnt, db_to_lin(target_rel_db), db_to_lin(floor_rel_dbfs),
                   out, scale)
        return (out, scale) if want_scale else out

    # ------------------------------------------------------------------ the entry points: recordings of one key, clips of many, live streams
    def embed(self, key32: bytes, audio, *, ctr0=0, block: int = 1024, payloads=None, carry=None, seed: int | None = None,
              session_nonce: bytes | None = None, target_rel_db: float = -10.0, floor_rel_dbfs: float = -35.0, want_scale: bool = False):
        """Whole watermarked recordings: the reference's transmit chain (seal -> polar encode -> header -> PN spread -> band-pass ->
        level mix, rtwm/embedder.py) for a batch, one frame-generator call and one mix launch.  audio float32 [R, n] (or [n]);
        recording r is what a WatermarkEmbedder with frame_ctr = ctr0[r] returns from process() over successive `block`-sized slices.
        payloads: sealed uint8 [R, nf, 55] for the new frames of counters ctr0[r] + k (mod 2^32); None: plaintext b"ESAL" | ctr | nonce8 |
        pad11 sealed under a 12-byte nonce, with random bytes from `secrets` as the reference (session_nonce: the 8 bytes a session keeps),
        or, with seed=, the deterministic bytes of `synthetic_frames`.  carry: the EmbedResult of the call this one continues (its pending
        chips are used first, as process() keeps them in its buffer).  -> EmbedResult."""
        from .crypto import SecureChannel
        FL = nat.ES_FRAME_LEN
        x = audio if torch.is_tensor(audio) else torch.as_tensor(np.asarray(audio))
        one_d = x.dim() == 1
        x = x.reshape(1, -1) if one_d else x
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("audio must be float32 [R, n] or [n]")
        x = self._dev(x, torch.float32)
        R, n = x.shape
        sec = SecureChannel(key32)
        c0 = _rows_ctr0(ctr0, R, "recording")
        if carry is not None and carry.tail.shape != (R, FL):
            raise ValueError("carry: the EmbedResult of a call over the same recordings")
        lay = embed_layout([n] * R, c0) if carry is None else stream_layout(carry.off, c0, [n] * R)
        start, off = (np.zeros(R, np.int64), lay.off) if carry is None else (lay.start, lay.off_next)      # a row of chips = [pending frame | new frames]
        nf = int(lay.nf.max()) if R else 0                      # the frame grid is rectangular: every recording gets the longest's count
        if payloads is not None:
            payloads = self._dev(payloads, torch.uint8)
            if payloads.dim() != 3 or payloads.shape[0] != R or payloads.shape[2] != 55 or payloads.shape[1] < nf:
                raise ValueError(f"payloads must be uint8 [R, nf >= {nf}, 55]")
            nf = payloads.shape[1] if nf else 0
            payloads = payloads[:, :nf]
        ctr_host = (c0[:, None] + np.arange(nf, dtype=np.int64)[None, :]) & 0xFFFFFFFF
        ctr = torch.from_numpy(ctr_host).to(self.device)
        if nf and R:
            if payloads is None and seed is not None:
                payloads = self._synthetic_payloads(sec, ctr.reshape(-1), seed)
            elif payloads is None:
                sn = _session_nonces(None if session_nonce is None else [session_nonce], 1, "session_nonce must be 8 bytes")
                nonces, plain = _fresh_plain(ctr_host.reshape(-1), sn)
                payloads = self.aead_seal(sec._aead._key, torch.from_numpy(nonces), torch.from_numpy(plain))
            frames = self.make_frames(sec, getattr(sec, "band_key", key32), ctr.reshape(-1), payloads.reshape(R * nf, 55)).reshape(R, nf * FL)
        else:
            frames = torch.empty((R, 0), dtype=torch.float32, device=self.device)
        chips = torch.cat((carry.tail.to(self.device), frames), dim=1) if carry is not None else frames
        res = self.mix(x, chips, block=block, chip_off=torch.from_numpy(start) if carry is not None else None, target_rel_db=target_rel_db,
                       floor_rel_dbfs=floor_rel_dbfs, want_scale=want_scale) if n else (x.clone(), None)
        out, scale = res if (want_scale or not n) else (res, None)
        end = start + n                                         # chips of the row consumed after this call
        slot = np.where(off > 0, end // FL, np.maximum(end // FL - 1, 0))      # the frame the stream stands in (pending chips from `off` on)
        if chips.shape[1]:
            idx = torch.from_numpy(slot).to(self.device)[:, None] * FL + torch.arange(FL, dtype=torch.int64, device=self.device)[None, :]
            tail = torch.gather(chips, 1, idx)
        else:
            tail = torch.zeros((R, FL), dtype=torch.float32, device=self.device)
        return EmbedResult(out[0] if one_d else out, lay.ctr_next, off, tail, scale)

    def embed_batch(self, keys, key_idx, clips, *, ctr0=0, block: int = 1024, payloads=None, seed: int | None = None, session_nonces=None,
                    target_rel_db: float = -10.0, floor_rel_dbfs: float = -35.0, want_scale: bool = False) -> list:
        """`embed` for clips of unequal length, each under its own key and start counter: entry i is, bit for bit, what
        embed(keys[key_idx[i]], clips[i], ctr0=ctr0[i], block=block, payloads=payloads[i]) returns -- the loop this call replaces is its
        definition (and through it the host WatermarkEmbedder.process, rtwm/embedder.py:44-168).
        keys: a KeyRing or a sequence of 32-byte keys; clips: 1-D float32 arrays / tensors of any lengths, 0 included; ctr0: a scalar or
        one value per clip (wraps at 2^32).  Clip i generates ceil(len_i / 1215) frames of counters ctr0_i + k whatever the block.
        payloads: per clip sealed uint8 [nf_i, 55]; seed=: the bytes embed(seed=) draws for each counter, sealed under the clip's key;
        neither: plaintext b"ESAL" | ctr | nonce8 | pad11 with `secrets` randomness sealed on the device, nonce8 one per clip
        (session_nonces: 8 bytes per clip, default fresh).
        The clips are cut into launches by scan.ragged_buckets(lengths, 1, EMBED_ROW_SAMPLES); each launch pads its clips into one
        [clips, longest rounded up to 4] tensor and runs ONE sequence whatever the number of keys and lengths: keyed seal (if needed) ->
        polar encode -> keyed schedule -> keyed frame generator -> ragged mix, over a flat frame list (embed_layout).
        Every clip starts a stream of its own; streams that continue across calls are `embed_step`'s (many streams, each under its
        key, one sequence per tick) or, one key at a time, `embed(carry=)`'s.  -> [EmbedClip], one per clip in input order."""
        ring = self.keyring(keys)
        clips = _clips_1d(clips, "clips")
        kidx = self._key_host(ring, key_idx)
        if kidx.size != len(clips):
            raise ValueError("one key index per clip is required")
        lengths = np.array([c.numel() for c in clips], np.int64)
        lay = embed_layout(lengths, ctr0)
        if payloads is not None:
            payloads = _clip_payloads(payloads, lay.nf, "payloads: per clip uint8 [nf >= ceil(len / 1215), 55]")
        n8 = _session_nonces(session_nonces, len(clips), "session_nonces: 8 bytes per clip") if payloads is None and seed is None else None
        out: list = [None] * len(clips)
        c0 = (lay.ctr_next - lay.nf) & 0xFFFFFFFF
        for idx, x, _ in self._launches(clips, lengths, c0, lay.off, want_scale, out):
            sub = embed_layout(lengths[idx], c0[idx])                   # the launch's own flat frame list
            ctr_d = torch.from_numpy(sub.ctr).to(self.device)
            kf_d = torch.from_numpy(kidx[idx][sub.clip].astype(np.int32)).to(self.device)      # key of every frame of the launch
            blobs = self._launch_blobs(ring, kf_d, ctr_d, sub.ctr, payloads, idx, sub.nf, seed, None if n8 is None else n8[idx][sub.clip])
            frames = self.make_frames_keyed(ring, kf_d, ctr_d, blobs)
            res = self.mix_ragged(x, torch.from_numpy(lengths[idx]), frames, torch.from_numpy(sub.chip_base), torch.from_numpy(sub.chip_cnt),
                                  block=block, target_rel_db=target_rel_db, floor_rel_dbfs=floor_rel_dbfs, want_scale=want_scale, out=x)
            _clip_results(x, res[1] if want_scale else None, idx, lengths, block, sub.ctr_next, sub.off, out)
        return out

    def _stream_rows(self, ring, key_idx, ctr0, session_nonces):
        """Checked host rows of new streams -> (key int64 [n], ctr int64 [n], nonce8 uint8 [n, 8])."""
        kidx = self._key_host(ring, key_idx)
        return kidx, _rows_ctr0(ctr0, kidx.size, "stream") & 0xFFFFFFFF, _session_nonces(session_nonces, kidx.size, "session_nonces: 8 bytes per stream")

    def open_streams(self, keys_or_ring, key_idx, *, ctr0=0, session_nonces=None) -> StreamTable:
        """A table of len(key_idx) live streams: stream s is marked under keys[key_idx[s]], makes its first frame under counter ctr0[s]
        (a scalar serves all, wraps at 2^32) and has nothing pending -- an embedder that has processed nothing.  session_nonces: the 8
        bytes stream s puts into every plaintext it seals (default fresh per stream).  keys_or_ring: a KeyRing or 32-byte keys."""
        ring = self.keyring(keys_or_ring)
        kidx, c0, n8 = self._stream_rows(ring, key_idx, ctr0, session_nonces)
        S = kidx.size
        return StreamTable(ring, torch.from_numpy(kidx.astype(np.int32)).to(self.device), torch.from_numpy(c0).to(self.device),
                           torch.zeros(S, dtype=torch.int64, device=self.device), torch.zeros((S, nat.ES_FRAME_LEN), dtype=torch.float32, device=self.device),
                           torch.from_numpy(n8).to(self.device), kidx.copy(), c0.copy(), np.zeros(S, np.int64), np.ones(S, bool))

    def add_streams(self, table: StreamTable, key_idx, *, ctr0=0, session_nonces=None) -> np.ndarray:
        """More streams for `table` (arguments of open_streams): closed rows are used first, lowest first, then the table grows.
        -> their stream ids, int64."""
        kidx, c0, n8 = self._stream_rows(table.ring, key_idx, ctr0, session_nonces)
        n, S = kidx.size, table.n
        ids = np.concatenate((np.flatnonzero(~table.live)[:n], np.arange(S, S + n, dtype=np.int64)))[:n]
        grow = int(np.count_nonzero(ids >= S))
        if grow:
            ext = lambda t, *shape: torch.cat((t, torch.zeros((grow,) + shape, dtype=t.dtype, device=t.device)))
            table.key, table.ctr, table.off = ext(table.key), ext(table.ctr), ext(table.off)
            table.tail, table.nonce8 = ext(table.tail, nat.ES_FRAME_LEN), ext(table.nonce8, 8)
            table.key_host, table.ctr_host, table.off_host = (np.concatenate((a, np.zeros(grow, np.int64)))
                                                              for a in (table.key_host, table.ctr_host, table.off_host))
            table.live = np.concatenate((table.live, np.zeros(grow, bool)))
        if n:
            rows = torch.from_numpy(ids).to(self.device)
            table.key[rows] = torch.from_numpy(kidx.astype(np.int32)).to(self.device)
            table.ctr[rows] = torch.from_numpy(c0).to(self.device)
            table.off[rows] = 0
            table.tail[rows] = 0.0
            table.nonce8[rows] = torch.from_numpy(n8).to(self.device)
            table.key_host[ids], table.ctr_host[ids], table.off_host[ids], table.live[ids] = kidx, c0, 0, True
        return ids

    def close_streams(self, table: StreamTable, sid) -> None:
        """Free the rows of streams `sid`: embed_step refuses them until add_streams hands the rows out again."""
        table.live[self._stream_ids(table, sid)] = False

    @staticmethod
    def _stream_ids(table: StreamTable, sid) -> np.ndarray:
        """Stream ids as int64, each inside the table, open and named once."""
        ids = np.asarray(sid.cpu().numpy() if torch.is_tensor(sid) else sid, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= table.n):
            raise ValueError(f"stream id outside [0, {table.n})")
        if np.unique(ids).size != ids.size:
            raise ValueError("a stream id appears twice in one call")
        if not table.live[ids].all():
            raise ValueError("a closed stream")
        return ids

    def embed_step(self, table: StreamTable, sid, chunks, *, block: int = 1024, payloads=None, seed: int | None = None,
                   target_rel_db: float = -10.0, floor_rel_dbfs: float = -35.0, want_scale: bool = False) -> list:
        """One tick of live streams: chunks[i] continues stream sid[i] of `table`, and the table moves on.  Entry i is, bit for bit, what
        embed(keys[key[s]], chunks[i], ctr0=prev.ctr, carry=prev, block=block, ...) returns for s = sid[i], `prev` the EmbedResult of
        that stream's previous chunk (none, and ctr0 = the stream's opening counter, for its first), and table.ctr / off / tail [s]
        are then that call's EmbedResult.ctr / off / tail -- the per-stream loop this call replaces is its definition (and through it
        WatermarkEmbedder.process over successive `block`-sized slices of every chunk, rtwm/embedder.py:44-75; the block grid starts
        again at every chunk).  chunks: 1-D float32 arrays / tensors of any lengths, 0 included; sid: stream ids, each at most once;
        streams not named are not touched.  payloads: per chunk sealed uint8 [>= new frames of the chunk, 55] (stream_layout says how
        many); seed=: the bytes embed(seed=) draws for each counter, sealed under the stream's key; neither: plaintext b"ESAL" | ctr |
        nonce8 | pad11 with `secrets` randomness sealed on the device, nonce8 the stream's own.
        The chunks are cut into launches by scan.ragged_buckets(lengths, 1, EMBED_ROW_SAMPLES); each launch pads its chunks into one
        [chunks, longest rounded up to 4] tensor and runs ONE sequence whatever the number of streams and keys: keyed seal (if needed)
        -> polar encode -> keyed schedule -> keyed frame generator -> stream mix (pending frame and new frames read where they lie) ->
        commit, over the flat frame list stream_layout computes from the table's host mirror.  A call whose chunks are all empty
        launches nothing.  -> [EmbedClip], one per chunk in input order."""
        ids = self._stream_ids(table, sid)
        chunks = _clips_1d(chunks, "chunks")
        if ids.size != len(chunks):
            raise ValueError("one stream id per chunk is required")
        block = int(block)
        if block < 1:
            raise ValueError("block must be >= 1")
        lengths = np.array([c.numel() for c in chunks], np.int64)
        if payloads is not None:
            payloads = _clip_payloads(payloads, stream_layout(table.off_host[ids], table.ctr_host[ids], lengths).nf,
                                      "payloads: per chunk uint8 [nf >= the chunk's new frames, 55]")
        out: list = [None] * len(chunks)
        for idx, x, stride in self._launches(chunks, lengths, table.ctr_host[ids], table.off_host[ids], want_scale, out):
            rows = ids[idx]
            lay = stream_layout(table.off_host[rows], table.ctr_host[rows], lengths[idx])
            F, n = lay.rec.size, len(idx)
            rec = np.ascontiguousarray(np.stack((rows, table.off_host[rows], lengths[idx], lay.chip_base, lay.chip_cnt), axis=1))   # [n, 5]
            rec_d = torch.from_numpy(np.ascontiguousarray(rec.T)).to(self.device)                                                    # [5, n]
            frames = None                                               # no new frame: every chunk lives on its stream's pending frame
            if F:
                fr = torch.from_numpy(np.stack((lay.ctr, table.key_host[rows][lay.rec], rows[lay.rec]))).to(self.device)            # [3, F]
                ctr_d, kf_d = fr[0], fr[1].to(torch.int32)
                blobs = self._launch_blobs(table.ring, kf_d, ctr_d, lay.ctr, payloads, idx, lay.nf, seed, (table.nonce8, fr[2]))      # (the stream's own nonce)
                frames = self.make_frames_keyed(table.ring, kf_d, ctr_d, blobs)
            scale = self._mix_out(x, x, block, want_scale)[2]
            tick = (n, stride, rec_d[2])
            pool = (frames, F * nat.ES_FRAME_LEN, rec_d[3], rec_d[4], rec.ctypes.data)
            self._call("es_mix_stream_batch", x, *tick, block, rec_d[0], table.n, table.tail, table.off, *pool, db_to_lin(target_rel_db),
                       db_to_lin(floor_rel_dbfs), x, scale)
            self._call("es_stream_commit_batch", *tick, rec_d[0], table.n, table.tail, table.ctr, table.off, *pool)
            table.ctr_host[rows], table.off_host[rows] = lay.ctr_next, lay.off_next
            _clip_results(x, scale, idx, lengths, block, lay.ctr_next, lay.off_next, out)
        return out
