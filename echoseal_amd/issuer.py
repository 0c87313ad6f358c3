"""WatermarkIssuer: mark many clips, each under its owner's key -- the transmit-side twin of WatermarkIdentifier.

For keys k_0 .. k_{N-1}, mark_batch(clips, key_idx)[i] is exactly what a freshly built WatermarkEmbedder(k_{key_idx[i]}, params) with
frame_ctr = ctr0[i] returns from process() over successive `block`-sized slices of clips[i] (rtwm/embedder.py:44-168) -- that
single-key host path, pinned to the reference by tests/golden/embed_mix.npz, is the definition.  What differs is the work: the clips
of a call, whatever their lengths and keys, share one launch sequence per memory-bounded group (RxEngine.embed_batch):

    keys -> es_keyring_derive_batch, once                     (rtwm/crypto.py:19-30, rtwm/utils.py:86-88)
    payloads -> es_aead_seal_keyed_batch                      (rtwm/embedder.py:153-168, rtwm/crypto.py:33-37)
    frames -> es_polar_encode_batch, es_schedule_keyed_batch, es_tx_frames_keyed_batch    (rtwm/embedder.py:78-141)
    level mix -> es_mix_ragged_batch                          (rtwm/embedder.py:44-75)

Every clip starts a stream of its own (an embedder that has processed nothing); continuing a stream across calls is
WatermarkEmbedder.embed's job.  Declared limit: the code, frame layout and sample rate are the engine's (N = 1024, K = 448, 48 kHz
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
        kidx = np.asarray(key_idx, dtype=np.int64).reshape(-1)
        if kidx.size != len(clips):
            raise ValueError("one key index per clip is required")
        if kidx.size and (kidx.min() < 0 or kidx.max() >= len(self.keys)):
            raise ValueError(f"key index outside [0, {len(self.keys)})")
        if not clips:
            return []
        res = self.engine.embed_batch(self._keyring(), kidx, clips, ctr0=ctr0, block=block, payloads=payloads, seed=seed,
                                      target_rel_db=self.p.target_rel_db, floor_rel_dbfs=self.p.floor_rel_dbfs)
        return [r.audio.cpu().numpy() for r in res]

    def mark(self, clip, key_index: int, *, ctr0: int = 0, block: int = 1024, payloads=None, seed: int | None = None) -> np.ndarray:
        return self.mark_batch([clip], [key_index], ctr0=ctr0, block=block, payloads=None if payloads is None else [payloads], seed=seed)[0]


__all__ = ["WatermarkIssuer"]
