"""Presence on the host: does a clip carry preamble peaks on one 1215-sample grid that follow a key's band-hop sequence from
some counter?  A NumPy twin that the kernels behind es_phase_fold_batch / es_hop_score_batch (csrc/es_keyring.hip) are held to bit for
bit, the public decoy keys the verdict is ranked against, and the argument checks of WatermarkDetector.presence.  No engine is needed for
anything here.

The rows: clip b owns rows 4 b .. 4 b + 3 of `corr`, row 4 b + band the float64 correlation row (es_xcorr_batch) of BAND_PLAN band `band`,
lags [0, nlag[b]); J = nlag // 1215 whole slots.  Every sum is float64, added term by term in ascending slot order from 0.0 -- the loops
below add one slot at a time to every independent sum at once, which is that order for each of them; np.sum is never used.
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

from .acquire import check_span, origin_of
from .scan import CTR_END, FRAME_LEN, PRE_L
from .utils import band_index

NBANDS = 4
DECOY_LABEL = b"EchoSeal:decoy:v1:"
NO_BAND = 0xFF                   # es_hop_window_batch's byte for a counter past 2^32 - 1


@dataclass
class Presence:
    """The verdict of a presence test.  score: the best mean of the correlation rows the detector's key hops through, over the span's
    origins and the phase list; null: the same under each public decoy key, in decoy order; detected: score > max(null), strictly, with
    at least one decoy -- under exchangeability of the keys a false alarm has probability at most 1 / (len(null) + 1).  ctr: the counter
    of the first whole frame of the best origin, phase its first sample, ctr0 = acquire.origin_of(ctr, phase) the counter origin to verify
    or acquire with; all three -1 where nothing was scored (an empty span).  frames: whole 1215-sample slots of the clip (J); phases:
    the phase list that was searched, best keyless fold first."""
    detected: bool
    score: float
    null: np.ndarray
    ctr: int
    phase: int
    ctr0: int
    frames: int
    phases: list


def decoy_keys(n: int) -> list[bytes]:
    """The first n public decoy master keys: SHA-256(b"EchoSeal:decoy:v1:" + i as four big-endian bytes), i from 0."""
    n = check_decoys(n)
    return [hashlib.sha256(DECOY_LABEL + i.to_bytes(4, "big")).digest() for i in range(n)]


def _int(v, what: str) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what} = {v!r}: an integer")
    return int(v)


def check_phases(phases) -> int:
    p = _int(phases, "phases")
    if not 1 <= p <= FRAME_LEN:
        raise ValueError(f"phases = {p}: between 1 and {FRAME_LEN} phases of the frame grid are searched")
    return p


def check_decoys(decoys) -> int:
    r = _int(decoys, "decoys")
    if r < 0:
        raise ValueError(f"decoys = {r}: a count of decoy keys, 0 or more (0 never detects)")
    return r


def slots(samples: int) -> int:
    """J: the whole 1215-sample slots among the lags of a clip of `samples` samples at fs_target."""
    return max(0, int(samples) - (PRE_L - 1)) // FRAME_LEN


def check_reach(span, samples: int) -> tuple[int, int]:
    """The span (acquire.check_span) of a clip of `samples` samples: the window of the last origin, hi - 1 + J - 1, must be a counter."""
    lo, hi = check_span(span)
    J = slots(samples)
    if hi > lo and hi + J - 1 > CTR_END:
        raise ValueError(f"span = ({lo}, {hi}): a clip of {int(samples)} samples has {J} frames, and hi + {J} - 1 > 2^32 "
                         "(spans that wrap past 2^32 are out of scope)")
    return lo, hi


def clip_spans(ctr0, span, n: int) -> list:
    """The span of each of n clips: `span` where ctr0 is None, else (c, c + 2) for the clip's origin c (one origin, or one per clip with
    None entries allowed: scan.counter_origins)."""
    from .scan import counter_origins
    span = check_span(span)
    return [span if c is None else check_span((c, c + 2)) for c in counter_origins(ctr0, n)]


def _rows(corr, nlag):
    corr = np.asarray(corr, np.float64)
    nlag = np.clip(np.asarray(nlag, np.int64).reshape(-1), 0, corr.shape[1])
    if corr.ndim != 2 or corr.shape[0] < NBANDS * nlag.size:
        raise ValueError("corr: float64 [rows, stride] with four rows per clip")
    return corr, nlag


def fold_model(corr, nlag) -> np.ndarray:
    """es_phase_fold_batch in NumPy -> fold float64 [B, 1215]."""
    corr, nlag = _rows(corr, nlag)
    fold = np.zeros((nlag.size, FRAME_LEN), np.float64)
    for b, n in enumerate(nlag.tolist()):
        acc = np.zeros(FRAME_LEN, np.float64)
        for j in range(n // FRAME_LEN):
            v = corr[NBANDS * b:NBANDS * b + NBANDS, FRAME_LEN * j:FRAME_LEN * (j + 1)]
            m = v[0].copy()
            for band in range(1, NBANDS):                                   # a later band only where strictly larger
                np.copyto(m, v[band], where=v[band] > m)
            acc = acc + m
        fold[b] = acc
    return fold


def pick_phases(fold_row, phases: int) -> list[int]:
    """The min(phases, 1215) phases of largest fold, largest first; of equal values the lower phase first."""
    f = np.asarray(fold_row, np.float64).reshape(-1)
    if f.size != FRAME_LEN:
        raise ValueError(f"a fold row has {FRAME_LEN} values")
    order = sorted(range(FRAME_LEN), key=lambda phi: (-f[phi], phi))
    return order[:check_phases(phases)]


def hop_model(keys, lo: int, cols: int) -> np.ndarray:
    """es_hop_window_batch with one hop row in NumPy: uint8 [K, cols], column i = utils.band_index(key, lo + i), 0xFF past 2^32 - 1."""
    hop = np.full((len(keys), int(cols)), NO_BAND, np.uint8)
    for k, key in enumerate(keys):
        for i in range(min(int(cols), CTR_END - int(lo))):
            hop[k, i] = band_index(key, int(lo) + i)
    return hop


def score_model(corr, nlag, phases, hop, n_origins: int):
    """es_hop_score_batch in NumPy -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K])."""
    corr, nlag = _rows(corr, nlag)
    phases = np.asarray(phases, np.int64).reshape(nlag.size, -1)
    hop = np.asarray(hop, np.uint8)
    K, n_origins = hop.shape[0], int(n_origins)
    score = np.full((nlag.size, K), -np.inf, np.float64)
    origin = np.full((nlag.size, K), -1, np.int64)
    rank = np.full((nlag.size, K), -1, np.int32)
    for b, n in enumerate(nlag.tolist()):
        J = n // FRAME_LEN
        if J == 0 or n_origins == 0:
            continue
        if hop.shape[1] < n_origins + J - 1:
            raise ValueError("hop: fewer than n_origins + J - 1 columns")
        rows = corr[NBANDS * b:NBANDS * b + NBANDS]
        for k in range(K):
            win = np.stack([hop[k, j:j + n_origins] for j in range(J)])                  # [J, n_origins]: slot j of every origin's window
            scored = np.flatnonzero((win < NBANDS).all(axis=0))
            if not scored.size:
                continue
            win = (win & 3).astype(np.int64)
            for p, phi in enumerate(phases[b].tolist()):
                if not 0 <= phi < FRAME_LEN:
                    continue
                acc = np.zeros(n_origins, np.float64)
                for j in range(J):
                    acc = acc + rows[win[j], phi + FRAME_LEN * j]
                s = (acc / np.float64(J))[scored]
                i = int(np.argmax(s))                                                    # the first of equal values: the lowest origin
                if origin[b, k] < 0 or s[i] > score[b, k] or (s[i] == score[b, k] and scored[i] < origin[b, k]):
                    score[b, k], origin[b, k], rank[b, k] = s[i], scored[i], p
    return score, origin, rank


def verdict(score_row, origin_row, rank_row, lo: int, phases: list, frames: int) -> Presence:
    """The Presence of one clip from its row of the score call: key row 0 is the detector's key, rows 1 .. R the decoys."""
    own, null = float(score_row[0]), np.array(score_row[1:], np.float64)
    found = int(origin_row[0]) >= 0
    ctr = int(lo) + int(origin_row[0]) if found else -1
    phase = int(phases[int(rank_row[0])]) if found else -1
    return Presence(bool(null.size and own > null.max()), own, null, ctr, phase, origin_of(ctr, phase) if found else -1, int(frames), list(phases))


def presence_model(corr4, nlag: int, key: bytes, *, span=(0, 4096), phases: int = 8, decoys: int = 32) -> Presence | None:
    """WatermarkDetector.presence from one clip's four correlation rows (BAND_PLAN order), on the host: the fold, the phase list, the hop
    rows of `key` and the decoys, the score and the verdict.  None where the clip has no whole slot."""
    corr4 = np.asarray(corr4, np.float64)
    nlag = min(max(int(nlag), 0), corr4.shape[1])
    lo, hi = check_reach(span, nlag + PRE_L - 1)
    J = nlag // FRAME_LEN
    if J == 0:
        return None
    plist = pick_phases(fold_model(corr4, [nlag])[0], phases)
    hop = hop_model([bytes(key)] + decoy_keys(decoys), lo, max(hi - lo + J - 1, 0))
    score, origin, rank = score_model(corr4, [nlag], [plist], hop, hi - lo)
    return verdict(score[0], origin[0], rank[0], lo, plist, J)


__all__ = ["DECOY_LABEL", "Presence", "check_decoys", "check_phases", "check_reach", "clip_spans", "decoy_keys", "fold_model", "hop_model",
           "pick_phases", "presence_model", "score_model", "slots", "verdict"]
