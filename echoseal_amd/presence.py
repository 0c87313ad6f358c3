"""Presence on the host: does a clip carry preamble peaks on one 1215-sample grid that follow a key's band-hop sequence from
some counter?  A NumPy twin that the kernels behind es_phase_fold_batch / es_hop_score_batch (csrc/es_keyring.hip) are held to bit for
bit, the public decoy keys the verdict is ranked against, and the argument checks of WatermarkDetector.presence.  No engine is needed for
anything here: the dataclasses, the checks, the geometry of spans and windows, and every *_model twin.  What is handed an engine -- the
launches and the verdict fan-out of every public presence call -- is presence_search.py.

The rows: clip b owns rows 4 b .. 4 b + 3 of `corr`, row 4 b + band the float64 correlation row (es_xcorr_batch) of BAND_PLAN band `band`,
lags [0, nlag[b]); J = nlag // 1215 whole slots.  Every sum is float64, added term by term in ascending slot order from 0.0 -- the loops
below add one slot at a time to every independent sum at once, which is that order for each of them; np.sum is never used.

Drift: a recording played by one device and captured by another has no rigid grid.  skew_table lists, for a largest clock
offset of drift_ppm, every total skew e of -E .. E samples across the clip as a row of per-slot offsets; warp_fold_model /
pick_hypotheses / warp_score_model are the fold, the pick and the score along those rows (es_warp_fold_batch, es_warp_score_batch;
include/echoseal_warp.h), and presence_model(..., drift_ppm=...) the whole search.

Live windows: a record may lie anywhere in a table of rows, such as a stream's window in a monitor table's correlation
history.  window_rows cuts the block es_warp_fold_at_batch / es_warp_score_at_batch may read (include/echoseal_live_presence.h), so the
models above are their twins too; live_span is the counter span of a stream with an origin, live_model the whole call for one stream.

The timeline: which parts of a clip carry the mark, and where it was cut.  pick_model is the twin of the device's pick
(es_fold_pick_batch; include/echoseal_pick.h); map_windows cuts a clip into overlapping windows, each a record of the _at calls with its own
span; stretches joins the detected windows that lie on one frame grid and names the splices between confirmed stretches; map_model is the
whole call on the host (presence_search.search_map: its launches).

The coherent test: the preamble and the keyed header of every frame start on matched-filter rows, over every phase.
mf_rows_model / coherent_score_model are the twins of es_mf_rows_batch / es_coherent_score_batch (include/echoseal_coherent.h),
coherent_model the whole of WatermarkDetector.presence_coherent for one clip on the host.

The coherent timeline: the coherent test on the windows of the timeline, for loud hosts.  coherent_score_at_model is the twin
of es_coherent_score_at_batch (include/echoseal_coherent_at.h), coherent_windows cuts a clip by its coherent slots, coherent_map_model is
the whole of WatermarkDetector.presence_coherent_map on the host (presence_search.search_coherent_map: its launches).
"""
from __future__ import annotations

import hashlib
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

from .acquire import check_span, origin_of
from .scan import CTR_END, FRAME_LEN, PRE_L
from .utils import band_index

NBANDS = 4
DECOY_LABEL = b"EchoSeal:decoy:v1:"
NO_BAND = 0xFF                   # es_hop_window_batch's byte for a counter past 2^32 - 1
PICK_MAX_H = 64                  # ES_PICK_MAX_H of include/echoseal_pick.h: the longest list es_fold_pick_batch picks


@dataclass
class Presence:
    """The verdict of a presence test.  score: the best mean of the correlation rows the detector's key hops through, over the span's
    origins and the phase list; null: the same under each public decoy key, in decoy order; detected: score > max(null), strictly, with
    at least one decoy -- under exchangeability of the keys a false alarm has probability at most 1 / (len(null) + 1).  ctr: the counter
    of the first whole frame of the best origin, phase its first sample, ctr0 = acquire.origin_of(ctr, phase) the counter origin to verify
    or acquire with; all three -1 where nothing was scored (an empty span).  frames: the 1215-sample slots that were summed (J); phases:
    the phase list that was searched, best keyless fold first.
    With a drift search (drift_ppm > 0 asked for): skew, the total offset in samples across the clip of the grid the best score was found
    on (the last slot starts `skew` samples later than on the rigid grid; 0 where nothing was scored); drift_ppm, the clock offset that
    corresponds to, 10^6 skew / (1215 frames); hypotheses, the (skew, phase) pairs that were searched, best keyless fold first (phases
    is their second column).  Without one: 0, 0.0 and None."""
    detected: bool
    score: float
    null: np.ndarray
    ctr: int
    phase: int
    ctr0: int
    frames: int
    phases: list
    skew: int = 0
    drift_ppm: float = 0.0
    hypotheses: list | None = None


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


def _reach(span, J: int, samples: int) -> tuple[int, int]:
    """The span (acquire.check_span) of a clip of `samples` samples and J slots: the window of the last origin, hi - 1 + J - 1, must be a
    counter."""
    lo, hi = check_span(span)
    if hi > lo and hi + J - 1 > CTR_END:
        raise ValueError(f"span = ({lo}, {hi}): a clip of {int(samples)} samples has {J} frames, and hi + {J} - 1 > 2^32 "
                         "(spans that wrap past 2^32 are out of scope)")
    return lo, hi


def check_reach(span, samples: int) -> tuple[int, int]:
    """The span of a clip of `samples` samples, checked (_reach) with J = slots(samples)."""
    return _reach(span, slots(samples), samples)


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


def _rigid(corr, nlag):
    """The rigid grid as a warp table: one row of zeros per clip, every whole slot of it -> (warp, nwarp, nslot) of the warp models."""
    corr, nlag = _rows(corr, nlag)
    return np.zeros((nlag.size, 1, corr.shape[1] // FRAME_LEN), np.int64), np.ones(nlag.size, np.int64), nlag // FRAME_LEN


def fold_model(corr, nlag) -> np.ndarray:
    """es_phase_fold_batch in NumPy -> fold float64 [B, 1215]: warp_fold_model on the rigid grid, as the kernels share one body."""
    return warp_fold_model(corr, nlag, *_rigid(corr, nlag))[:, 0]


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
    """es_hop_score_batch in NumPy -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K]): warp_score_model on the rigid grid,
    list entry p = (row 0, phases[b][p])."""
    warp, nwarp, nslot = _rigid(corr, nlag)
    phases = np.asarray(phases, np.int64).reshape(nslot.size, -1)
    return warp_score_model(corr, nlag, warp, nwarp, nslot, np.stack([np.zeros_like(phases), phases], axis=2), hop, n_origins)


def check_drift(drift_ppm) -> float:
    """drift_ppm of a presence call: a finite number, 0 or more (0: the rigid grid)."""
    if isinstance(drift_ppm, (bool, np.bool_)) or not isinstance(drift_ppm, (int, float, np.integer, np.floating)):
        raise ValueError(f"drift_ppm = {drift_ppm!r}: a number of parts per million")
    if not math.isfinite(drift_ppm) or drift_ppm < 0:
        raise ValueError(f"drift_ppm = {drift_ppm!r}: the largest clock offset searched in either direction, finite and 0 or more")
    return float(drift_ppm)


def skew_table(nlag: int, drift_ppm) -> tuple[list[int], int, np.ndarray]:
    """The grids a drift search tries on a clip of nlag lags -> (skews, J, warp).  E = ceil(drift_ppm nlag / 10^6) exactly;
    J = (nlag - E) // 1215 slots; skews = [0, -1, 1, -2, 2 .. -E, E], row 0 the rigid grid; warp int32 [2 E + 1, J],
    warp[d][j] = floor((2 j e + J) / (2 J)) for e = skews[d]: j e / J rounded half up, so e is the total skew across the clip.  Every
    column phi + 1215 j + warp[d][j], phi <= 1214, lies in [0, nlag).  Integers only.  ValueError: a bad drift_ppm (check_drift),
    E > 1214, or no slot left (J == 0) where the rigid grid had one."""
    drift, nlag = check_drift(drift_ppm), max(int(nlag), 0)
    E = math.ceil(Fraction(drift) * nlag / 10 ** 6)
    if E > FRAME_LEN - 1:
        raise ValueError(f"drift_ppm = {drift_ppm!r}: {E} samples of skew across {nlag} lags, more than {FRAME_LEN - 1} (a whole frame)")
    J = (nlag - E) // FRAME_LEN
    if J == 0 and nlag // FRAME_LEN:
        raise ValueError(f"drift_ppm = {drift_ppm!r}: {E} samples of skew leave no whole slot in {nlag} lags")
    skews = [0] + [s * e for e in range(1, E + 1) for s in (-1, 1)]
    j = np.arange(J, dtype=np.int64)
    warp = np.stack([(2 * j * e + J) // (2 * J) if J else j for e in skews]).astype(np.int32)       # // floors, for negative e too
    return skews, J, warp


def _table(warp, nwarp, nslot, nlag):
    """The table of a warp call as the kernels see it: -> (warp int64 [B, D, Jw], nwarp [B], J [B] clamped to [0, min(Jw, nlag // 1215)])."""
    warp = np.asarray(warp, np.int64)
    if warp.ndim != 3 or warp.shape[0] != nlag.size:
        raise ValueError("warp: int [B, D, Jw], a table per clip")
    nwarp, nslot = (np.asarray(a, np.int64).reshape(-1) for a in (nwarp, nslot))
    if nwarp.size != nlag.size or nslot.size != nlag.size:
        raise ValueError("nwarp, nslot: one value per clip")
    return warp, nwarp, np.clip(nslot, 0, np.minimum(warp.shape[2], nlag // FRAME_LEN))


def _usable(w, d: int, nw: int, J: int, n: int) -> bool:
    """Row d of a clip's table w [D, Jw]: d < nwarp, and each of its J slots whole inside [0, n)."""
    if not 0 <= d < min(nw, w.shape[0]):
        return False
    first = FRAME_LEN * np.arange(J, dtype=np.int64) + w[d, :J]
    return bool((first >= 0).all() and (first + (FRAME_LEN - 1) < n).all())


def warp_fold_model(corr, nlag, warp, nwarp, nslot) -> np.ndarray:
    """es_warp_fold_batch in NumPy -> fold float64 [B, D, 1215]; an unusable row is -inf."""
    corr, nlag = _rows(corr, nlag)
    warp, nwarp, nslot = _table(warp, nwarp, nslot, nlag)
    fold = np.full((nlag.size, warp.shape[1], FRAME_LEN), -np.inf, np.float64)
    phi = np.arange(FRAME_LEN)
    for b, (n, J) in enumerate(zip(nlag.tolist(), nslot.tolist())):
        for d in range(warp.shape[1]):
            if not _usable(warp[b], d, int(nwarp[b]), J, n):
                continue
            acc = np.zeros(FRAME_LEN, np.float64)
            for j in range(J):
                v = corr[NBANDS * b:NBANDS * b + NBANDS][:, FRAME_LEN * j + int(warp[b, d, j]) + phi]
                m = v[0].copy()
                for band in range(1, NBANDS):                               # a later band only where strictly larger
                    np.copyto(m, v[band], where=v[band] > m)
                acc = acc + m
            fold[b, d] = acc
    return fold


def _score_frame(hop, nslot, n_origins: int, record):
    """What the score twins share around their inner sums -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K]).  Record b
    has nslot[b] slots J; hop uint8 [K, Ccols] holds, per key, the window of every origin: slot j of origin o is hop[k][o + j].  Scored
    are the origins whose J bytes are all bands (none above 3).  record(b, J) -> term, and term(k, win, scored) yields (entry, s) in list
    order: s float64 [scored.size], the score of list entry `entry` at each scored origin under key k, win int64 [J, n_origins] the bands.
    Kept per (record, key) is the largest s, of equal values the lowest origin, then the earliest entry; (-inf, -1, -1) where nothing is
    scored (J == 0, no origin, no scored origin, no entry)."""
    K, B = hop.shape[0], len(nslot)
    score = np.full((B, K), -np.inf, np.float64)
    origin = np.full((B, K), -1, np.int64)
    rank = np.full((B, K), -1, np.int32)
    for b, J in enumerate(nslot):
        if J == 0 or n_origins == 0:
            continue
        if hop.shape[1] < n_origins + J - 1:
            raise ValueError("hop: fewer than n_origins + J - 1 columns")
        term = record(b, J)
        for k in range(K):
            win = np.stack([hop[k, j:j + n_origins] for j in range(J)])                  # [J, n_origins]: slot j of every origin's window
            scored = np.flatnonzero((win < NBANDS).all(axis=0))
            if not scored.size:
                continue
            for entry, s in term(k, (win & 3).astype(np.int64), scored):
                i = int(np.argmax(s))                                                    # the first of equal values: the lowest origin
                if origin[b, k] < 0 or s[i] > score[b, k] or (s[i] == score[b, k] and scored[i] < origin[b, k]):
                    score[b, k], origin[b, k], rank[b, k] = s[i], scored[i], entry
    return score, origin, rank


def pick_hypotheses(fold_rows, phases: int) -> list[tuple[int, int]]:
    """The min(phases, D 1215) pairs (row d, phase phi) of largest fold over the usable rows of one clip's fold [D, 1215] (an unusable
    row is all -inf), largest first; of equal values the lower row first, then the lower phase."""
    f = np.asarray(fold_rows, np.float64)
    if f.ndim != 2 or f.shape[1] != FRAME_LEN:
        raise ValueError(f"a clip's fold is [D, {FRAME_LEN}]")
    pairs = [(d, phi) for d in range(f.shape[0]) if not np.isneginf(f[d]).all() for phi in range(FRAME_LEN)]
    pairs.sort(key=lambda p: (-f[p], p))
    return pairs[:min(check_phases(phases), f.shape[0] * FRAME_LEN)]


def warp_score_model(corr, nlag, warp, nwarp, nslot, hyp, hop, n_origins: int):
    """es_warp_score_batch in NumPy: hyp int [B, H, 2], entry h of clip b = (d, phi)
    -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K])."""
    corr, nlag = _rows(corr, nlag)
    warp, nwarp, nslot = _table(warp, nwarp, nslot, nlag)
    hyp = np.asarray(hyp, np.int64).reshape(nlag.size, -1, 2)
    n_origins = int(n_origins)

    def record(b, J):
        rows = corr[NBANDS * b:NBANDS * b + NBANDS]
        good = [(h, d, phi) for h, (d, phi) in enumerate(hyp[b].tolist())
                if 0 <= phi < FRAME_LEN and _usable(warp[b], d, int(nwarp[b]), J, int(nlag[b]))]

        def term(k, win, scored):
            for h, d, phi in good:
                acc = np.zeros(n_origins, np.float64)
                for j in range(J):
                    acc = acc + rows[win[j], phi + FRAME_LEN * j + int(warp[b, d, j])]
                yield h, (acc / np.float64(J))[scored]
        return term

    return _score_frame(np.asarray(hop, np.uint8), nslot.tolist(), n_origins, record)


def verdict(score_row, origin_row, rank_row, lo: int, phases: list, frames: int, pos0: int = 0) -> Presence:
    """The Presence of one record from its row of the score call: key row 0 is the detector's key, rows 1 .. R the decoys.  pos0: the
    absolute first sample of the record (a clip: 0; a live window: w0; a window of a timeline: its column), for ctr0."""
    own, null = float(score_row[0]), np.array(score_row[1:], np.float64)
    found = int(origin_row[0]) >= 0
    ctr = int(lo) + int(origin_row[0]) if found else -1
    phase = int(phases[int(rank_row[0])]) if found else -1
    return Presence(bool(null.size and own > null.max()), own, null, ctr, phase, origin_of(ctr, phase, int(pos0)) if found else -1, int(frames),
                    list(phases))


def drift_verdict(score_row, origin_row, rank_row, lo: int, hyps: list, skews: list, frames: int, pos0: int = 0) -> Presence:
    """The Presence of one record from its row of the warp score call: hyps its (row, phase) list, skews the skew of each table row."""
    p = verdict(score_row, origin_row, rank_row, lo, [phi for _, phi in hyps], frames, pos0)
    p.skew = int(skews[hyps[int(rank_row[0])][0]]) if p.ctr >= 0 else 0
    p.drift_ppm = 1e6 * p.skew / (FRAME_LEN * int(frames))
    p.hypotheses = [(int(skews[d]), int(phi)) for d, phi in hyps]
    return p


def presence_model(corr4, nlag: int, key: bytes, *, span=(0, 4096), phases: int = 8, decoys: int = 32, drift_ppm=0.0, pos0: int = 0) -> Presence | None:
    """WatermarkDetector.presence from one clip's four correlation rows (BAND_PLAN order), on the host: the fold, the phase list, the hop
    rows of `key` and the decoys, the score and the verdict.  None where the clip has no whole slot.  drift_ppm > 0: the same along every
    row of skew_table(nlag, drift_ppm), the list being the (row, phase) pairs of largest fold.  pos0: the absolute first sample of the
    rows, where they are a window of something longer (verdict)."""
    corr4 = np.asarray(corr4, np.float64)
    nlag = min(max(int(nlag), 0), corr4.shape[1])
    lo, hi = check_reach(span, nlag + PRE_L - 1)
    if check_drift(drift_ppm) > 0:
        skews, J, warp = skew_table(nlag, drift_ppm)
        if J == 0:
            return None
        tab = (warp[None], [len(skews)], [J])
        hyps = pick_hypotheses(warp_fold_model(corr4, [nlag], *tab)[0], phases)
        hop = hop_model([bytes(key)] + decoy_keys(decoys), lo, max(hi - lo + J - 1, 0))
        score, origin, rank = warp_score_model(corr4, [nlag], *tab, [hyps], hop, hi - lo)
        return drift_verdict(score[0], origin[0], rank[0], lo, hyps, skews, J, pos0)
    J = nlag // FRAME_LEN
    if J == 0:
        return None
    plist = pick_phases(fold_model(corr4, [nlag])[0], phases)
    hop = hop_model([bytes(key)] + decoy_keys(decoys), lo, max(hi - lo + J - 1, 0))
    score, origin, rank = score_model(corr4, [nlag], [plist], hop, hi - lo)
    return verdict(score[0], origin[0], rank[0], lo, plist, J, pos0)


# ---- records anywhere in a table of rows: the windows of live streams (include/echoseal_live_presence.h) ----
def window_rows(corr, rows4, col, nlag) -> np.ndarray:
    """The record of an _at call as a clip: float64 [4, n], row `band` = corr[rows4[band], col : col + n], n = nlag clamped to
    [0, stride - col] -- and n = 0 where the record is not addressable (a row outside [0, rows) or col outside [0, stride]).  The
    models above run on it unchanged: es_warp_fold_at_batch / es_warp_score_at_batch read exactly this block."""
    corr = np.asarray(corr, np.float64)
    if corr.ndim != 2:
        raise ValueError("corr: float64 [rows, stride]")
    rows4 = [int(r) for r in np.asarray(rows4, np.int64).reshape(-1)]
    if len(rows4) != NBANDS:
        raise ValueError("rows4: the row of each of the four bands")
    col, stride = int(col), corr.shape[1]
    ok = 0 <= col <= stride and all(0 <= r < corr.shape[0] for r in rows4)
    n = min(max(int(nlag), 0), stride - col) if ok else 0
    return np.stack([corr[r, col:col + n] for r in rows4]) if n else np.zeros((NBANDS, 0), np.float64)


def live_span(origin: int, w0: int, J: int) -> tuple[int, int]:
    """The counters the first whole frame of a window may carry, for a stream whose frame k carries counter origin + k and whose window
    starts at absolute sample w0: slot 0 at phase phi <= 1214 carries origin + round((w0 + phi) / 1215) (the rounding of es_plan_at_batch
    and acquire.origin_of), which is e or e + 1 for e = origin + (2 w0 + 1215) // 2430 -> (e, e + 2), hi lowered so that the window of
    the last origin, hi - 1 + J - 1, is a counter (hi + J - 1 <= 2^32; never below lo)."""
    e = min(int(origin) + (2 * int(w0) + FRAME_LEN) // (2 * FRAME_LEN), CTR_END)
    return e, max(e, min(e + 2, CTR_END - max(int(J), 1) + 1))


def table_rows(bands, stream: int) -> list[int]:
    """rows4 of stream `stream` of a monitor table whose row 4 s + j holds band bands[j]: entry `band` = 4 s + j with bands[j] == band."""
    place = {int(b): j for j, b in enumerate(np.asarray(bands).reshape(-1).tolist())}
    if sorted(place) != list(range(NBANDS)):
        raise ValueError("bands: the four band indices, each once")
    return [NBANDS * int(stream) + place[band] for band in range(NBANDS)]


def live_model(hist, stream: int, bands, base: int, w0: int, n: int, key: bytes, *, origin: int | None = None, span=(0, 4096), phases: int = 8,
               decoys: int = 32, drift_ppm=0.0) -> Presence | None:
    """LiveMonitor.presence for one stream, on the host, from the monitor table's correlation history `hist` [4 S, H] (column 0 = absolute
    lag `base`): the window [w0, n) has lags [0, n - 62 - w0) from column w0 - base of the stream's four rows; the span is live_span
    for a stream with a counter origin, else `span` read as absolute counters of the window's first frame; then presence_model.  The
    result's ctr0 is acquire.origin_of(ctr, phase, w0): ctr is the counter of the window's first whole frame, phase is relative to the
    window.  None where the window has no whole slot."""
    nlag = int(n) - (PRE_L - 1) - int(w0)
    J = max(nlag, 0) // FRAME_LEN
    if J == 0:
        return None
    block = window_rows(hist, table_rows(bands, stream), int(w0) - int(base), nlag)
    sp = check_reach(span, nlag + PRE_L - 1) if origin is None or int(origin) < 0 else live_span(origin, w0, J)
    return presence_model(block, nlag, key, span=sp, phases=phases, decoys=decoys, drift_ppm=drift_ppm, pos0=w0)


# ---- the hypothesis list as the device picks it (include/echoseal_pick.h) ----
def pick_model(fold, nwarp=None, H: int = 8):
    """es_fold_pick_batch in NumPy: fold float64 [B, D, 1215], nwarp [B] (None: D; clamped to [0, D]) -> (hyp int32 [B, H, 2], val
    float64 [B, H]).  The candidates of record b are the values of its first nwarp[b] rows that are neither -inf nor NaN; entry h is
    the (row, phase) of the h-th largest, equal values (-0.0 == +0.0) by the lower row, then the lower phase; val the value as the fold
    holds it; (-1, -1) and -inf past the last candidate."""
    fold = np.asarray(fold, np.float64)
    if fold.ndim != 3 or fold.shape[2] != FRAME_LEN:
        raise ValueError(f"fold: float64 [B, D, {FRAME_LEN}]")
    B, D, H = fold.shape[0], fold.shape[1], _int(H, "H")
    if not 1 <= H <= PICK_MAX_H:
        raise ValueError(f"H = {H}: a list of 1 .. {PICK_MAX_H} entries")
    nwarp = np.full(B, D, np.int64) if nwarp is None else np.clip(np.asarray(nwarp, np.int64).reshape(-1), 0, D)
    if nwarp.size != B:
        raise ValueError("nwarp: one row count per record")
    hyp = np.full((B, H, 2), -1, np.int32)
    val = np.full((B, H), -np.inf, np.float64)
    for b in range(B):
        v = fold[b, :nwarp[b]].reshape(-1)
        idx = np.flatnonzero(~np.isnan(v) & ~np.isneginf(v))
        rank = np.where(v[idx] == 0.0, 0.0, v[idx])                         # one zero
        top = idx[np.lexsort((idx, -rank))][:H]                             # by the value, largest first; then by the index
        hyp[b, :top.size, 0], hyp[b, :top.size, 1] = top // FRAME_LEN, top % FRAME_LEN
        val[b, :top.size] = v[top]
    return hyp, val


# ---- the presence timeline of a clip: windows, marked stretches and splices ----
@dataclass
class Stretch:
    """A maximal run of adjacent windows first .. last, each detected and each consistent with the one before it.  start, end: the
    samples [start, end) at fs_target from the first window's first to the last window's last slot; t: the grid anchor of the first
    window, the clip sample at which frame 0 would start (col + phase - 1215 ctr); ctr0: the counter origin of the first window
    (acquire.origin_of at its column); score: the smallest own score in the run; confirmed: the run has at least `confirm` windows."""
    first: int
    last: int
    start: int
    end: int
    t: int
    ctr0: int
    score: float
    confirmed: bool


@dataclass
class Splice:
    """A change of grid between two successive confirmed stretches A and B, whatever lies between them: somewhere in samples [lo, hi)
    -- from the column of A's last window to the end of B's first -- `removed` samples are missing (negative: were inserted):
    the anchor of A's last window minus the anchor of B's first."""
    lo: int
    hi: int
    removed: int


@dataclass
class PresenceMap:
    """The presence timeline of a clip.  windows: the Presence of each window (its ctr0 taken at the window's column); starts: the slot
    each window starts at; stretches, splices: as above; marked: the samples at fs_target covered by confirmed stretches (the union of
    their [start, end))."""
    windows: list
    starts: list
    stretches: list
    splices: list
    marked: int


def check_map(window, step, confirm, phases) -> tuple[int, int, int, int]:
    """The arguments of a presence map: integers, 1 <= step <= window slots, confirm >= 1 windows, 1 <= phases <= 64 (the device picks
    the lists: ES_PICK_MAX_H)."""
    W, S, C, P = _int(window, "window"), _int(step, "step"), _int(confirm, "confirm"), check_phases(phases)
    if S < 1 or S > W:
        raise ValueError(f"step = {S}, window = {W}: windows of `window` 1215-sample slots every `step` slots, 1 <= step <= window")
    if C < 1:
        raise ValueError(f"confirm = {C}: the windows that confirm a stretch, 1 or more")
    if P > PICK_MAX_H:
        raise ValueError(f"phases = {P}: a presence map searches at most {PICK_MAX_H} phases per window")
    return W, S, C, P


def map_windows(nlag: int, window: int = 40, step: int = 20) -> list[tuple[int, int, int]]:
    """The windows of a clip of nlag lags -> [(first slot s, column 1215 s, lags)], J = nlag // 1215: none for J == 0; the whole clip,
    (0, 0, nlag), for J <= window; else windows of `window` slots at s = 0, step, 2 step .. <= J - window, and one at J - window
    where the steps do not end there."""
    nlag = max(int(nlag), 0)
    J = nlag // FRAME_LEN
    return [(s, FRAME_LEN * s, FRAME_LEN * n if n < J else nlag) for s, n in _cut(J, window, step)]


def _cut(J: int, window: int, step: int) -> list[tuple[int, int]]:
    """The windows of J slots -> [(first slot s, slots)]: none for J == 0; all of them, (0, J), for J <= window; else windows of `window`
    slots at s = 0, step, 2 step .. <= J - window, and one at J - window where the steps do not end there."""
    W, S, _, _ = check_map(window, step, 1, 1)
    if J <= W:
        return [(0, J)] if J else []
    starts = list(range(0, J - W + 1, S))
    if (J - W) % S:
        starts.append(J - W)
    return [(s, W) for s in starts]


def window_span(span, s: int, J: int) -> tuple[int, int]:
    """The span of the window that starts s slots into a clip whose slot 0 may carry the counters of `span`: (lo + s, hi + s), lowered
    at 2^32 as live_span lowers it (hi + J - 1 <= 2^32 for the window's J slots; never below lo; possibly empty)."""
    lo, hi = check_span(span)
    lo = min(lo + int(s), CTR_END)
    return lo, max(lo, min(hi + int(s), CTR_END - max(int(J), 1) + 1))


def anchor(p: Presence, col: int) -> int:
    """t of a window whose own key was found: the clip sample at which frame 0 would start."""
    return int(col) + p.phase - FRAME_LEN * p.ctr


def consistent(t_a: int, col_a: int, t_b: int, col_b: int, drift_ppm=0.0) -> bool:
    """Do two windows lie on one frame grid?  |t_a - t_b| <= 1 + ceil(drift_ppm |col_b - col_a| / 10^6), the ceiling exact."""
    return abs(int(t_a) - int(t_b)) <= 1 + math.ceil(Fraction(check_drift(drift_ppm)) * abs(int(col_b) - int(col_a)) / 10 ** 6)


def stretches(windows, cols, nlags, drift_ppm=0.0, confirm: int = 2):
    """The stretches, the splices and the marked samples of a list of windows -> (list of Stretch, list of Splice, marked).  windows[w]:
    the Presence of window w or None; cols[w], nlags[w]: its first column and its lags."""
    C = _int(confirm, "confirm")
    out, run = [], []

    def close():
        if run:
            a, b = run[0], run[-1]
            out.append(Stretch(a, b, int(cols[a]), int(cols[b]) + FRAME_LEN * (int(nlags[b]) // FRAME_LEN), anchor(windows[a], cols[a]),
                               origin_of(windows[a].ctr, windows[a].phase, int(cols[a])), min(float(windows[w].score) for w in run), len(run) >= C))
            run.clear()

    for w, p in enumerate(windows):
        if p is None or not p.detected or p.ctr < 0:
            close()
            continue
        if run and not consistent(anchor(windows[run[-1]], cols[run[-1]]), cols[run[-1]], anchor(p, cols[w]), cols[w], drift_ppm):
            close()
        run.append(w)
    close()
    sure = [s for s in out if s.confirmed]
    splices = [Splice(int(cols[a.last]), int(cols[b.first]) + FRAME_LEN * (int(nlags[b.first]) // FRAME_LEN),
                      anchor(windows[a.last], cols[a.last]) - anchor(windows[b.first], cols[b.first])) for a, b in zip(sure[:-1], sure[1:])]
    marked, reach = 0, 0
    for s in sure:                                                          # ascending starts: the union of [start, end)
        marked += max(s.end - max(s.start, reach), 0)
        reach = max(reach, s.end)
    return out, splices, marked


def make_map(windows, wins, drift_ppm, confirm) -> PresenceMap:
    """The PresenceMap of a clip from its windows' verdicts and map_windows' list."""
    st, sp, marked = stretches(windows, [c for _, c, _ in wins], [n for _, _, n in wins], drift_ppm, confirm)
    return PresenceMap(list(windows), [s for s, _, _ in wins], st, sp, marked)


def map_model(corr4, nlag: int, key: bytes, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2, phases: int = 8,
              decoys: int = 32, drift_ppm=0.0) -> PresenceMap | None:
    """WatermarkDetector.presence_map from one clip's four correlation rows, on the host: presence_model on the window_rows block of each
    window of map_windows, under the window's own span, then stretches.  None where the clip has no whole slot."""
    corr4 = np.asarray(corr4, np.float64)
    W, S, C, P = check_map(window, step, confirm, phases)
    nlag = min(max(int(nlag), 0), corr4.shape[1])
    wins = map_windows(nlag, W, S)
    if not wins:
        return None
    verdicts = [presence_model(window_rows(corr4, range(NBANDS), col, n), n, key, span=window_span(span, s, n // FRAME_LEN), phases=P, decoys=decoys,
                               drift_ppm=drift_ppm, pos0=col) for s, col, n in wins]
    return make_map(verdicts, wins, drift_ppm, C)


# ---- the coherent presence test: preamble and keyed header on matched-filter rows, every phase (include/echoseal_coherent.h) ----
HDR_L, HDR_REPEAT = 128, 8       # the header: the counter's low 16 bits, each over 8 chips, times the key's header PN
COH_SPAN = PRE_L + HDR_L - 1     # 190: the last chip of a frame start that the receiver can know, from its first


def mf_tables(fs: int = 48_000, tables=None):
    """What the coherent rows need of an engine's tables (tables.pack_tables(fs), or `tables` = its tuple) -> (g, c): g[b] float64 [L_b],
    g[b][i] = taps[b][L_b - 1 - i], the matched filter in forward order; c float64 [4], c[b] = sqrt(191 * sum_i g[b][i]^2), the sum taken
    term by term from +0.0 in ascending i."""
    if tables is None:
        from .tables import pack_tables
        tables = pack_tables(fs)
    taps, ntaps = tables[2], tables[3]
    g = [np.asarray(taps[b][:int(ntaps[b])], np.float32)[::-1].astype(np.float64) for b in range(NBANDS)]
    c = np.zeros(NBANDS, np.float64)
    for b in range(NBANDS):
        s = np.float64(0.0)
        for v in g[b]:
            s = s + v * v
        c[b] = np.sqrt(np.float64(COH_SPAN + 1) * s)
    return g, c


def coherent_slots(samples: int, g) -> int:
    """J of a clip of `samples` samples: max(0, n - 189 - L_max) // 1215 -- every start phi + 1215 j, phi <= 1214, j < J, is then
    defined in every band."""
    return max(0, int(samples) - (COH_SPAN - 1) - max(len(t) for t in g)) // FRAME_LEN


def check_coherent_reach(span, samples: int, g) -> tuple[int, int]:
    """check_reach with the coherent J."""
    return _reach(span, coherent_slots(samples, g), samples)


def mf_rows_model(y, lens, bands, g, c):
    """es_mf_rows_batch in NumPy: y float64 [rows, T], lens [rows] (clamped to [0, T]), bands [rows] -> (M, A, D) float64 [rows, T], NaN
    where a value is not defined.  With L = len(g[band]), W = 190 + L and n the row's length:
        M[t] = sum_{i < L} y[t + i] g[i]                   t + L <= n
        A[s] = sum_{q < 63} p_q M[s + q]                   s + W <= n        p = the preamble symbols, +-1
        D[s] = sqrt(sum_{m < W} y[s + m]^2) c[band]        s + W <= n
    every sum term by term from +0.0 in ascending index, a product formed and then added.  Nothing at or past n is read."""
    from .utils import mseq_63
    y = np.asarray(y, np.float64)
    if y.ndim != 2:
        raise ValueError("y: float64 [rows, T]")
    rows, T = y.shape
    lens = np.clip(np.asarray(lens, np.int64).reshape(-1), 0, T)
    bands = np.asarray(bands, np.int64).reshape(-1)
    if lens.size != rows or bands.size != rows or (rows and (bands.min() < 0 or bands.max() >= NBANDS)):
        raise ValueError("lens, bands: one length and one band index 0 .. 3 per row")
    pre = 2.0 * mseq_63().astype(np.float64) - 1.0
    M, A, D = (np.full((rows, T), np.nan, np.float64) for _ in range(3))
    for r in range(rows):
        n, gb = int(lens[r]), g[int(bands[r])]
        L = len(gb)
        nm, ns = n - L + 1, n - (COH_SPAN + L) + 1
        if nm <= 0:
            continue
        m = np.zeros(nm, np.float64)
        for i in range(L):
            m = m + y[r, i:i + nm] * gb[i]
        M[r, :nm] = m
        if ns <= 0:
            continue
        a, q = np.zeros(ns, np.float64), np.zeros(ns, np.float64)
        for k in range(PRE_L):
            a = a + pre[k] * m[k:k + ns]
        for k in range(COH_SPAN + L):
            q = q + y[r, k:k + ns] * y[r, k:k + ns]
        A[r, :ns], D[r, :ns] = a, np.sqrt(q) * c[int(bands[r])]
    return M, A, D


def header_signs(keys) -> np.ndarray:
    """u float64 [K, 128], +-1: the header PN of each master key, as ring bytes 272 .. 287 hold it (MSB first)."""
    from .crypto import SecureChannel
    return np.stack([2.0 * np.asarray(SecureChannel(bytes(k)).pn_bits(0, HDR_L), np.float64) - 1.0 for k in keys]) if len(keys) else np.zeros((0, HDR_L))


def ring_signs(hdr_pn) -> np.ndarray:
    """The same from packed rows: hdr_pn uint8 [K, 16] (KeyRing.hdr_pn)."""
    return 2.0 * np.unpackbits(np.asarray(hdr_pn, np.uint8).reshape(-1, HDR_L // 8), axis=1).astype(np.float64) - 1.0


def coherent_score_model(M, A, D, nslot, phases, u, hop, lo: int, n_origins: int):
    """es_coherent_score_batch in NumPy.  Clip b owns rows 4 b .. 4 b + 3 of M, A, D [rows, T]; nslot [B] its slots J (clamped to
    [0, max(0, T - 190) // 1215]: no index can pass a row); phases int [B, P]; u [K, 128] +-1 (header_signs); hop uint8 [K, Ccols], column i
    the band of counter lo + i; origins 0 .. n_origins - 1.  For key k, origin o, entry p with phi = phases[b][p], and per slot j:
        c = lo + o + j, band = hop[k][o + j], s = phi + 1215 j, v = c & 0xFFFF, sigma_i = 2 ((v >> (15 - i)) & 1) - 1
        Z_i = sum_{m < 8} u[k][8 i + m] M[band][s + 63 + 8 i + m]
        N = (A[band][s] + sum_{i < 8} sigma_i Z_i) + sum_{i = 8 .. 15} sigma_i Z_i,     R = N / D[band][s], +0.0 where D == 0
        S(k, o, p) = (sum_{j < J} R) / J
    -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K]): the largest S, ties to the lowest origin, then the earliest entry;
    (-inf, -1, -1) where nothing is scored (J == 0, no origin whose window is free of bytes above 3, no entry in 0 .. 1214).  Vectorised
    over the phase list; the two header sums are tabulated per (band, byte) present, each entry summed in the order above."""
    M, A, D = (np.asarray(a, np.float64) for a in (M, A, D))
    if M.ndim != 2 or A.shape != M.shape or D.shape != M.shape:
        raise ValueError("M, A, D: float64 [rows, T], the three of one shape")
    T = M.shape[1]
    nslot = np.clip(np.asarray(nslot, np.int64).reshape(-1), 0, max(0, T - COH_SPAN) // FRAME_LEN)
    B = nslot.size
    if M.shape[0] < NBANDS * B:
        raise ValueError("M, A, D: four rows per clip")
    phases = np.asarray(phases, np.int64).reshape(B, -1)
    u, hop = np.asarray(u, np.float64).reshape(-1, HDR_L), np.asarray(hop, np.uint8)
    K, n_origins, lo = hop.shape[0], int(n_origins), int(lo)
    if u.shape[0] != K:
        raise ValueError("u: one row of 128 signs per hop row")
    bit = lambda v, i: 2.0 * ((v >> (7 - i)) & 1) - 1.0                     # sign i of a byte, MSB first

    def record(b, J):
        good = np.flatnonzero((phases[b] >= 0) & (phases[b] < FRAME_LEN))
        phi = phases[b][good]
        Mb, Ab, Db = (a[NBANDS * b:NBANDS * b + NBANDS] for a in (M, A, D))

        def term(k, win, scored):
            if not good.size:
                return
            acc = np.zeros((scored.size, good.size), np.float64)
            for j in range(J):
                s = phi + FRAME_LEN * j
                band = win[j, scored]
                v = (lo + scored + j) & 0xFFFF
                hi8, lo8 = v >> 8, v & 0xFF
                Z = np.zeros((NBANDS, 16, s.size), np.float64)
                for i in range(16):
                    for m in range(HDR_REPEAT):
                        Z[:, i] = Z[:, i] + u[k, 8 * i + m] * Mb[:, s + (PRE_L + 8 * i + m)]
                tabs = []
                for byte, half in ((hi8, 0), (lo8, 8)):                      # the sum of a byte's eight terms, per value present
                    vals, inv = np.unique(byte, return_inverse=True)
                    t = np.zeros((NBANDS, vals.size, s.size), np.float64)
                    for i in range(8):
                        t = t + bit(vals, i)[None, :, None] * Z[:, half + i][:, None, :]
                    tabs.append(t[band, inv])                                # [scored, P]
                num = (Ab[:, s][band] + tabs[0]) + tabs[1]
                den = Db[:, s][band]
                acc = acc + np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
            S = acc / np.float64(J)
            for col, p in enumerate(good.tolist()):
                yield p, S[:, col]
        return term

    return _score_frame(hop, nslot.tolist(), n_origins, record)


def coherent_model(y4, n: int, key: bytes, *, span=(0, 4096), phases=FRAME_LEN, decoys: int = 32, fs: int = 48_000, tables=None,
                   pos0: int = 0) -> Presence | None:
    """WatermarkDetector.presence_coherent from one clip's four band-passed rows y4 [4, >= n] (BAND_PLAN order), on the host: the rows,
    the hop rows and header signs of `key` and the decoys, the score over every phase and the verdict.  phases: 1215, every phase in
    order, or an explicit list (what the keyless fold picked).  None where the clip has no whole slot (J == 0).  pos0: the absolute first
    sample of the rows, where they are a window of something longer (verdict)."""
    y4 = np.asarray(y4, np.float64)
    n = min(max(int(n), 0), y4.shape[1])
    g, c = mf_tables(fs, tables)
    lo, hi = check_coherent_reach(span, n, g)
    plist = list(range(FRAME_LEN)) if isinstance(phases, (int, np.integer)) and int(phases) == FRAME_LEN else [int(p) for p in phases]
    J = coherent_slots(n, g)
    if J == 0:
        return None
    keys = [bytes(key)] + decoy_keys(decoys)
    M, A, D = mf_rows_model(y4[:NBANDS, :n], [n] * NBANDS, range(NBANDS), g, c)
    hop = hop_model(keys, lo, max(hi - lo + J - 1, 0))
    score, origin, rank = coherent_score_model(M, A, D, [J], [plist], header_signs(keys), hop, lo, hi - lo)
    return verdict(score[0], origin[0], rank[0], lo, plist, J, pos0)


# ---- the coherent presence timeline: the coherent test on the windows of a clip (include/echoseal_coherent_at.h) ----
def coherent_score_at_model(M, A, D, rows4, col, nslot, Jw: int, phases, u, hop, hop_row, lo, n_origins: int):
    """es_coherent_score_at_batch in NumPy.  M, A, D float64 [rows, stride]; record b: rows4[b][band] the row of its band `band`, col[b]
    the column of its sample 0, nslot[b] its slots.  It is addressable iff its four rows lie in [0, rows) and 0 <= col <= stride; its J is
    nslot clamped to [0, min(Jw, max(0, stride - col - 190) // 1215)], 0 where it is not addressable or hop_row[b] lies outside [0, HR).
    hop uint8 [K, HR, Ccols] ([K, Ccols]: HR = 1); lo[b] the counter of column 0 of hop row hop_row[b], counters taken mod 2^32.  The
    record's block -- columns [col, col + 1215 J + 190) of its four rows, all the kernel may read -- goes through coherent_score_model
    under its own hop row and lo, as window_rows serves the folds -> (score float64 [B, K], origin int64 [B, K], rank int32 [B, K])."""
    M, A, D = (np.asarray(a, np.float64) for a in (M, A, D))
    if M.ndim != 2 or A.shape != M.shape or D.shape != M.shape:
        raise ValueError("M, A, D: float64 [rows, stride], the three of one shape")
    rows, stride = M.shape
    nslot = np.asarray(nslot, np.int64).reshape(-1)
    B, Jw = nslot.size, int(Jw)
    rows4, col = np.asarray(rows4, np.int64).reshape(B, NBANDS), np.asarray(col, np.int64).reshape(-1)
    hop_row, lo = np.asarray(hop_row, np.int64).reshape(-1), np.asarray(lo, np.int64).reshape(-1)
    if col.size != B or hop_row.size != B or lo.size != B:
        raise ValueError("col, nslot, hop_row, lo: one value per record")
    hop = np.asarray(hop, np.uint8)
    if hop.ndim == 2:
        hop = hop[:, None, :]
    K, HR = hop.shape[0], hop.shape[1]
    phases = np.asarray(phases, np.int64).reshape(B, -1)
    if Jw < 0 or hop.shape[2] < int(n_origins) + Jw - 1:
        raise ValueError("Jw >= 0 and hop with at least n_origins + Jw - 1 columns")
    score = np.full((B, K), -np.inf, np.float64)
    origin = np.full((B, K), -1, np.int64)
    rank = np.full((B, K), -1, np.int32)
    for b in range(B):
        c = int(col[b])
        if not (0 <= c <= stride and all(0 <= int(r) < rows for r in rows4[b]) and 0 <= int(hop_row[b]) < HR):
            continue
        J = min(max(int(nslot[b]), 0), Jw, max(0, stride - c - COH_SPAN) // FRAME_LEN)
        if J == 0:
            continue
        n = FRAME_LEN * J + COH_SPAN
        block = [np.stack([a[int(r), c:c + n] for r in rows4[b]]) for a in (M, A, D)]
        score[b], origin[b], rank[b] = (v[0] for v in coherent_score_model(*block, [J], [phases[b]], u, hop[:, int(hop_row[b])],
                                                                            int(lo[b]) & 0xFFFFFFFF, n_origins))
    return score, origin, rank


def coherent_windows(samples: int, g, window: int = 40, step: int = 20) -> list[tuple[int, int, int]]:
    """The windows of a clip of `samples` samples -> [(first slot s, column 1215 s, slots)], J = coherent_slots(samples, g): none for
    J == 0; the whole clip, (0, 0, J), for J <= window; else windows of `window` slots at s = 0, step, 2 step .. <= J - window, and one
    at J - window where the steps do not end there (map_windows, counted in slots: a window reads 1215 slots + 189 + L_max samples)."""
    return [(s, FRAME_LEN * s, n) for s, n in _cut(coherent_slots(samples, g), window, step)]


def coherent_map_model(y4, n: int, key: bytes, *, span=(0, 4096), window: int = 40, step: int = 20, confirm: int = 2, decoys: int = 32,
                       fs: int = 48_000, tables=None) -> PresenceMap | None:
    """WatermarkDetector.presence_coherent_map from one clip's four band-passed rows y4 [4, >= n], on the host: coherent_model on the
    samples [col, col + 1215 slots + 189 + L_max) of each window of coherent_windows, under the window's own span (window_span), every
    phase searched; then stretches on the rigid grid.  M, A and D are FIR outputs of y, so the rows of a slice are the clip's rows bit
    for bit wherever the slice defines them.  None where the clip has no whole slot."""
    y4 = np.asarray(y4, np.float64)
    W, S, C, _ = check_map(window, step, confirm, 1)
    n = min(max(int(n), 0), y4.shape[1])
    g, _ = mf_tables(fs, tables)
    wins = coherent_windows(n, g, W, S)
    if not wins:
        return None
    tail = COH_SPAN - 1 + max(len(t) for t in g)
    verdicts = [coherent_model(y4[:NBANDS, col:col + FRAME_LEN * J + tail], FRAME_LEN * J + tail, key, span=window_span(span, s, J), decoys=decoys,
                               fs=fs, tables=tables, pos0=col) for s, col, J in wins]
    return make_map(verdicts, [(s, col, FRAME_LEN * J) for s, col, J in wins], 0.0, C)


__all__ = ["COH_SPAN", "DECOY_LABEL", "PICK_MAX_H", "Presence", "PresenceMap", "Splice", "Stretch", "anchor",
           "check_coherent_reach", "check_decoys", "check_drift", "check_map", "check_phases", "check_reach", "clip_spans", "coherent_map_model",
           "coherent_model", "coherent_score_at_model", "coherent_score_model", "coherent_slots", "coherent_windows", "consistent", "decoy_keys",
           "drift_verdict", "fold_model", "header_signs", "hop_model", "live_model", "live_span", "make_map", "map_model", "map_windows",
           "mf_rows_model", "mf_tables", "pick_hypotheses", "pick_model", "pick_phases", "presence_model", "ring_signs", "score_model", "skew_table", "slots", "stretches", "table_rows", "verdict", "warp_fold_model", "warp_score_model",
           "window_rows", "window_span"]
