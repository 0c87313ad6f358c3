"""WatermarkIssuer: mark many clips, each under its owner's key -- the transmit-side twin of WatermarkIdentifier.

For keys k_0 .. k_{N-1}, mark_batch(clips, key_idx)[i] is exactly what a freshly built WatermarkEmbedder(k_{key_idx[i]}, params) with
frame_ctr = ctr0[i] returns from process() over successive `block`-sized slices of clips[i] (rtwm/embedder.py:44-168) -- that
single-key host path, pinned to the reference by tests/golden/embed_mix.npz, is the definition.  What differs is the work: the clips
of a call, whatever their lengths and keys, share one launch sequence per memory-bounded group (RxEngine.embed_batch, in transmit.py):

    keys -> es_keyring_derive_batch, once                     (rtwm/crypto.py:19-30, rtwm/utils.py:86-88)
    payloads -> es_aead_seal_keyed_batch                      (rtwm/embedder.py:153-168, rtwm/crypto.py:33-37)
    frames -> es_polar_encode_batch, es_schedule_keyed_batch, es_tx_frames_keyed_batch    (rtwm/embedder.py:78-141)
    level mix -> es_mix_ragged_batch                          (rtwm/embedder.py:44-75)

Every clip of mark_batch starts a stream of its own (an embedder that has processed nothing).  Streams that go on from call to call are
open_streams' job: a LiveStreams keeps, per stream, the counter, the frame it stands in and its session nonce on the device, and
push() marks one chunk of any length for any subset of them in one launch sequence (RxEngine.embed_step: the chain above with
es_mix_stream_batch for the mix and es_stream_commit_batch behind it) -- each stream exactly what its own WatermarkEmbedder returns from
process() over successive `block`-sized slices of each chunk.  Declared limit: the code, frame layout and sample rate are the engine's (N = 1024, K = 448, 48 kHz
unless the engine says otherwise, the 63-chip preamble); params that ask for others are refused before any GPU work.
"""
from __future__ import annotations

import numpy as np

from .embedder import TxParams
from .polar_fast import K_DEFAULT, N_DEFAULT
from .utils import mseq_63


class WatermarkIssuer:
    def __init__(self, keys, params: TxParams | None = None, *, engine=None) -> None:
        self.keys = [bytes(k) for k in keys]
        if any(len(k) != 32 for k in self.keys):
            raise ValueError("master_key must be 32 bytes (256 bit)")
        self.p = params or TxParams()
        self._engine = engine
        self._ring = None
        self._check_params()

    def _check_params(self) -> None:
        """The declared limit: N, K and fs of the engine (the defaults an engine is built with while none is given), its preamble."""
        eng = self._engine
        want = {"N": N_DEFAULT, "K": getattr(eng, "code_k", K_DEFAULT), "fs": getattr(eng, "fs", 48_000)}
        for name, v in want.items():
            if int(getattr(self.p, name)) != int(v):
                raise ValueError(f"WatermarkIssuer: params.{name} = {getattr(self.p, name)} but the engine's is {v}: the batched transmit "
                                 "chain runs the engine's code and sample rate only")
        if not np.array_equal(np.asarray(self.p.preamble), mseq_63()):
            raise ValueError("WatermarkIssuer: params.preamble must be the 63-chip m-sequence of the frame generator")

    @property
    def engine(self):
        if self._engine is None:
            from .engine import RxEngine
            self._engine = RxEngine(0, list_size_max=0)             # a front-end engine: the transmit chain needs no list decoder
            self._check_params()
        return self._engine

    def _keyring(self):
        eng = self.engine
        if self._ring is None or self._ring.ring.device != eng.device:
            self._ring = eng.keyring(self.keys)                      # derived on first use
        return self._ring

    def mark_batch(self, clips, key_idx, *, ctr0=0, block: int = 1024, payloads=None, seed: int | None = None) -> list:
        """Clip i marked under keys[key_idx[i]] from frame counter ctr0[i] (a scalar serves all) -> list of float32 arrays, in input
        order.  payloads: per clip sealed uint8 [ceil(len / 1215), 55]; seed=: deterministic payloads (RxEngine.embed_batch); neither:
        fresh randomness per call, as the reference."""
        clips = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in clips]
        kidx = self._key_indices(key_idx)
        if kidx.size != len(clips):
            raise ValueError("one key index per clip is required")
        if not clips:
            return []
        res = self.engine.embed_batch(self._keyring(), kidx, clips, ctr0=ctr0, block=block, payloads=payloads, seed=seed,
                                      target_rel_db=self.p.target_rel_db, floor_rel_dbfs=self.p.floor_rel_dbfs)
        return [r.audio.cpu().numpy() for r in res]

    def open_streams(self, key_idx, *, ctr0=0, session_nonces=None) -> "LiveStreams":
        """Live streams, stream s under keys[key_idx[s]] from frame counter ctr0[s] (a scalar serves all); session_nonces: the 8 bytes
        each stream puts into every plaintext it seals (default fresh per stream)."""
        return LiveStreams(self, self.engine.open_streams(self._keyring(), self._key_indices(key_idx), ctr0=ctr0, session_nonces=session_nonces))

    def _key_indices(self, key_idx) -> np.ndarray:
        kidx = np.asarray(key_idx, dtype=np.int64).reshape(-1)
        if kidx.size and (kidx.min() < 0 or kidx.max() >= len(self.keys)):
            raise ValueError(f"key index outside [0, {len(self.keys)})")
        return kidx

    def mark(self, clip, key_index: int, *, ctr0: int = 0, block: int = 1024, payloads=None, seed: int | None = None) -> np.ndarray:
        return self.mark_batch([clip], [key_index], ctr0=ctr0, block=block, payloads=None if payloads is None else [payloads], seed=seed)[0]


class LiveStreams:
    """The open streams of a WatermarkIssuer (WatermarkIssuer.open_streams); stream ids are the rows of `table`."""

    def __init__(self, issuer: WatermarkIssuer, table) -> None:
        self._issuer, self.table = issuer, table

    def __len__(self) -> int:
        return int(np.count_nonzero(self.table.live))

    def push(self, chunks, streams=None, *, block: int = 1024, payloads=None, seed: int | None = None) -> list:
        """chunks[i], float32 of any length, continues stream streams[i] (None: one chunk per open stream, in order) -> the
        marked chunks as float32 arrays, in input order; the streams move on, the others are not touched.  payloads: per chunk sealed
        uint8 [>= its new frames, 55]; seed=: deterministic payloads; neither: fresh randomness under the stream's session nonce.  A
        stream named twice, outside the table or closed is a ValueError before any GPU work."""
        chunks = [np.ascontiguousarray(c, dtype=np.float32) for c in chunks]
        if streams is None:
            streams = np.flatnonzero(self.table.live)
        p = self._issuer.p
        res = self._issuer.engine.embed_step(self.table, streams, chunks, block=block, payloads=payloads, seed=seed,
                                             target_rel_db=p.target_rel_db, floor_rel_dbfs=p.floor_rel_dbfs)
        return [r.audio.cpu().numpy() for r in res]

    def state(self):
        """-> (ctr, off) int64 [streams]: the counter of each stream's next frame and the chips of its current frame already used
        (host copies; rows of closed streams keep what they last held)."""
        return self.table.ctr_host.copy(), self.table.off_host.copy()

    def add(self, key_idx, *, ctr0=0, session_nonces=None) -> np.ndarray:
        """More streams (arguments of WatermarkIssuer.open_streams) -> their ids; rows of closed streams are used first."""
        return self._issuer.engine.add_streams(self.table, self._issuer._key_indices(key_idx), ctr0=ctr0, session_nonces=session_nonces)

    def close(self, streams) -> None:
        """Free the rows of `streams`; a push to a closed stream raises ValueError."""
        self._issuer.engine.close_streams(self.table, streams)


__all__ = ["WatermarkIssuer", "LiveStreams"]
