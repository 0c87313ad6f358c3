"""Presence on the device: the launches and the verdict fan-out behind every public presence call.  Everything here
is handed an engine; everything that can be checked without a GPU -- the checks, the geometry, the host twins of every kernel called here,
the verdicts themselves -- is presence.py.

search: the correlation test (4.23), its drift search (4.24) and records anywhere in a table of rows (4.25), on the host's pick or the
device's (4.26).  search_map: the timeline, the windows of a launch's clips through search in groups.  search_coherent: the coherent test
of a launch's clips (4.27).  search_coherent_map: its timeline (4.28).  The two timelines share one record builder and one group
generator: windows go to the device in groups of consecutive windows whose hop table stays within MAP_HOP_BYTES.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from .presence import NBANDS, PICK_MAX_H, coherent_windows, drift_verdict, make_map, map_windows, pick_hypotheses, pick_phases, skew_table, verdict, window_span
from .scan import CTR_END, FRAME_LEN, dev

MAP_HOP_BYTES = 256 << 20        # the most bytes of one group's hop table, [K][HR][Ccols] uint8: windows go to the search in groups within it


def _verdicts(n_own: int, score_row, origin_row, rank_row, make) -> list:
    """One Presence per own key from a record's row of a score call over the ring [own keys] + decoys: entry k ranks key row k against
    the decoy rows.  make(score, origin, rank) is verdict / drift_verdict with the record's own arguments bound."""
    pick = lambda a, k: np.concatenate((a[k:k + 1], a[n_own:]))
    return [make(pick(score_row, k), pick(origin_row, k), pick(rank_row, k)) for k in range(n_own)]


def _padded(lists, ids, P: int) -> np.ndarray:
    """hyp int32 [len(ids), P, 2] of the records `ids`: a list is P entries long; a shorter one ends in entries that name nothing."""
    hyp = np.full((len(ids), P, 2), -1, np.int32)
    for k, b in enumerate(ids):
        hyp[k, :len(lists[b])] = lists[b]
    return hyp


def search(eng, ring, n_own: int, corr, nlag, spans, drift: float, P: int, at=None, pos0=None, device_pick: bool = False) -> list:
    """The launches and verdicts of every presence call (WatermarkDetector.presence_batch, WatermarkIdentifier.presence_batch,
    LiveMonitor.presence, LiveIdentifier.presence) -> per record None (no whole slot) or a list of n_own Presence, one per own key.
    ring: the device key ring [the n_own own keys] + decoys.  corr, nlag: the records' rows; spans: (lo, hi) per record.
    at None: clips, record b = rows 4 b .. 4 b + 3 from column 0, all of ONE span -- the rigid grid (drift 0) through phase_fold /
    hop_score, a drift search through warp_fold / warp_score, as presence_batch always called them.
    at = (rows4 [B, 4], col [B]): records anywhere in the table `corr`, each with its own span -- ONE warp_fold_at over all of them (drift 0:
    a one-row table of zeros), ONE download and pick, ONE hop_window with a hop row per distinct span base, and ONE warp_score_at per
    group of equal span width.  pos0 [B]: the absolute first sample of each record, for the verdict's ctr0 (None: 0).
    device_pick (the at= route only, P <= ES_PICK_MAX_H): the fold stays on the device, ONE fold_pick replaces the download
    and the host's pick, its lists go into warp_score_at as they are, and only they are downloaded, for the verdicts' phase lists -- the
    same verdicts, field for field.  False: the launches and bits every call had before."""
    if device_pick and at is None:
        raise ValueError("device_pick: the route of records anywhere in a table (at=)")
    if device_pick and P > PICK_MAX_H:
        raise ValueError(f"phases = {P}: the device picks lists of at most {PICK_MAX_H} entries")
    nlag = np.asarray(nlag, np.int64).reshape(-1)
    B = nlag.size
    out: list = [None] * B
    spans = [(int(lo), int(hi)) for lo, hi in spans]
    rigid = not drift > 0
    made = {} if rigid else {n: skew_table(n, drift) for n in set(nlag.tolist())}       # records of one length share a table
    tabs = None if rigid else [made[n] for n in nlag.tolist()]
    J = np.maximum(nlag, 0) // FRAME_LEN if rigid else np.array([t[1] for t in tabs], np.int64)
    if not B or not J.max():
        return out

    # ---- stage one, the lists: per record its phases (the rigid clip route) or its (row, phase) pairs, best keyless fold first
    table = hyp_dev = None
    if rigid and at is None:
        lists = [pick_phases(f, P) for f in eng.phase_fold(corr, nlag).cpu().numpy()]
        jw = corr.shape[1] // FRAME_LEN                                     # the slots hop_score sizes the hop table for
    else:
        nwarp = np.ones(B, np.int32) if rigid else np.array([len(t[0]) for t in tabs], np.int32)
        warp = np.zeros((B, int(nwarp.max()), int(J.max())), np.int32)      # zeros past a record's own rows and slots: nwarp and nslot say where they end
        for k, t in enumerate(tabs or ()):
            warp[k, :t[2].shape[0], :t[1]] = t[2]
        table = (dev(eng, warp, np.int32), dev(eng, nwarp, np.int32), dev(eng, J, np.int32))
        fold = eng.warp_fold(corr, nlag, *table) if at is None else eng.warp_fold_at(corr, at[0], at[1], nlag, *table)
        if device_pick:
            hyp_dev = eng.fold_pick(fold, table[1], P, want_val=False)[0]
            lists = [[(d, phi) for d, phi in h if d >= 0] for h in hyp_dev.cpu().numpy().tolist()]
        else:
            lists = [pick_hypotheses(f[:d], P) for f, d in zip(fold.cpu().numpy(), nwarp)]
        jw = int(J.max())

    def make(b):
        """verdict / drift_verdict with record b's own arguments bound."""
        lo, first = spans[b][0], 0 if pos0 is None else int(pos0[b])
        if rigid:
            phis = lists[b] if at is None else [phi for _, phi in lists[b]]
            return lambda s, o, r: verdict(s, o, r, lo, phis, int(J[b]), first)
        return lambda s, o, r: drift_verdict(s, o, r, lo, lists[b], tabs[b][0], int(J[b]), first)

    # ---- stage two, the score per span width and the verdicts
    bases = sorted({min(lo, CTR_END - 1) for lo, _ in spans})               # one hop row per distinct span base
    hop = eng.hop_window(ring, bases, max(max(hi - lo for lo, hi in spans) + jw - 1, 0))
    if at is not None:
        rows4, col = dev(eng, at[0], np.int64).reshape(B, NBANDS), dev(eng, at[1], np.int64).reshape(B)
    for width in sorted({hi - lo for lo, hi in spans}):
        ids = [b for b, (lo, hi) in enumerate(spans) if hi - lo == width]
        if at is None:
            if len(ids) != B or len(bases) != 1:
                raise ValueError("clips of one launch share one span")
            res = eng.hop_score(corr, nlag, np.array(lists, np.int32), hop, width) if rigid else \
                eng.warp_score(corr, nlag, *table, _padded(lists, ids, P), hop, width)
        else:
            sel = dev(eng, ids, np.int64)
            hop_row = np.array([bases.index(min(spans[b][0], CTR_END - 1)) for b in ids], np.int32)
            res = eng.warp_score_at(corr, rows4[sel], col[sel], nlag[ids], table[0][sel], table[1][sel], table[2][sel],
                                    hyp_dev[sel] if device_pick else _padded(lists, ids, P), hop, hop_row, width)
        score, origin, rank = (t.cpu().numpy() for t in res)
        for k, b in enumerate(ids):
            if J[b]:
                out[b] = _verdicts(n_own, score[k], origin[k], rank[k], make(b))
    return out


def search_coherent(eng, ring, n_own: int, M, A, D, J, lists, lo: int, hi: int) -> list:
    """The coherent test of the clips of one launch, all of the span (lo, hi) -> per clip None (no whole slot) or a list of n_own
    Presence, one per own key.  Clip b owns rows 4 b .. 4 b + 3 of M, A, D (mf_rows' tensors) and has J[b] slots (presence.coherent_slots);
    lists[b] is its phase list.  ONE hop window over the ring and ONE coherent_score."""
    base = min(lo, CTR_END - 1)
    hop = eng.hop_window(ring, [base], max(hi - lo + max(0, M.shape[1] - 190) // FRAME_LEN - 1, 0))
    score, origin, rank = (t.cpu().numpy() for t in eng.coherent_score(M, A, D, J, np.array(lists, np.int32), ring, hop, base, hi - lo))
    return [_verdicts(n_own, score[b], origin[b], rank[b], lambda s, o, r: verdict(s, o, r, lo, lists[b], int(J[b]))) if J[b] else None
            for b in range(len(J))]


# ---- the two timelines: records, and the groups they go to the device in ----
class Record(NamedTuple):
    """A window of a clip as a record of the _at calls."""
    clip: int                   # the clip of the launch, and ...
    window: int                 # ... which of its windows
    rows4: list                 # the rows of its four bands
    col: int                    # the column of its sample 0: its absolute first sample in the clip
    size: int                   # what the window cutter gave it: lags (map_windows) or slots (coherent_windows)
    slots: int
    span: tuple                 # its own span (presence.window_span)


def _records(wins, spans, per_slot: int) -> list:
    """The windows of every clip of a launch as records, clip by clip: wins[c] the windows of clip c (first slot, column, size), of
    size // per_slot slots each; spans[c] the span of the clip's slot 0."""
    return [Record(c, w, [NBANDS * c + band for band in range(NBANDS)], col, size, size // per_slot, window_span(spans[c], s, size // per_slot))
            for c, ws in enumerate(wins) for w, (s, col, size) in enumerate(ws)]


def _groups(recs, K: int):
    """Consecutive records in groups whose hop table -- a hop row per distinct span base min(lo, 2^32 - 1), K HR Ccols bytes -- stays
    within MAP_HOP_BYTES (read at every call); a group holds at least one record -> (records, sorted bases, Ccols) per group."""
    i = 0
    while i < len(recs):
        bases, ccols, j = set(), 0, i
        while j < len(recs):                                                # grow the group while its hop table fits
            lo, hi = recs[j].span
            grown = bases | {min(lo, CTR_END - 1)}
            cols = max(ccols, hi - lo + recs[j].slots - 1)
            if j > i and K * len(grown) * cols > MAP_HOP_BYTES:
                break
            bases, ccols, j = grown, cols, j + 1
        yield recs[i:j], sorted(bases), ccols
        i = j


def _maps(wins, verdicts, n_own: int, drift: float, confirm: int) -> list:
    """Per clip None (no window) or one PresenceMap per own key from its windows (first slot, column, lags) and their verdicts."""
    return [None if not ws else [make_map([None if v is None else v[k] for v in vs], ws, drift, confirm) for k in range(n_own)]
            for ws, vs in zip(wins, verdicts)]


def search_map(eng, ring, n_own: int, corr, clip_nlag, spans, drift: float, P: int, window: int, step: int, confirm: int) -> list:
    """The windows of every clip of one launch through `search` (at=, device_pick=True) -> per clip None (no whole slot) or n_own
    PresenceMap, one per own key.  Clip c owns rows 4 c .. 4 c + 3 of corr; spans[c] is its span.  Windows go in groups (_groups): per
    group ONE fold, ONE pick, ONE hop window and ONE score per span width, never a launch per window."""
    wins = [map_windows(n, window, step) for n in np.asarray(clip_nlag, np.int64).reshape(-1).tolist()]
    verdicts = [[None] * len(ws) for ws in wins]
    for group, _, _ in _groups(_records(wins, spans, FRAME_LEN), ring.n):
        col = [r.col for r in group]
        res = search(eng, ring, n_own, corr, [r.size for r in group], [r.span for r in group], drift, P,
                     at=(np.array([r.rows4 for r in group], np.int64), np.array(col, np.int64)), pos0=col, device_pick=True)
        for r, v in zip(group, res):
            verdicts[r.clip][r.window] = v
    return _maps(wins, verdicts, n_own, drift, confirm)


def search_coherent_map(eng, ring, n_own: int, M, A, D, clip_samples, spans, g, window: int, step: int, confirm: int) -> list:
    """The coherent windows of every clip of one launch through the device -> per clip None (no whole slot) or n_own PresenceMap, one per
    own key.  Clip c owns rows 4 c .. 4 c + 3 of M, A, D (mf_rows' tensors) and has clip_samples[c] samples; spans[c] is its span; g the
    matched filters (mf_tables).  Windows go in the groups of search_map (_groups): per group ONE hop window and ONE coherent_score_at
    per distinct span width, never a launch per window.  Every record searches every phase: the identity list."""
    wins = [coherent_windows(n, g, window, step) for n in np.asarray(clip_samples, np.int64).reshape(-1).tolist()]
    verdicts = [[None] * len(ws) for ws in wins]
    plist = list(range(FRAME_LEN))
    for group, bases, ccols in _groups(_records(wins, spans, 1), ring.n):
        hop = eng.hop_window(ring, bases, max(ccols, 0))
        for width in sorted({r.span[1] - r.span[0] for r in group}):
            ids = [r for r in group if r.span[1] - r.span[0] == width]
            base = [min(r.span[0], CTR_END - 1) for r in ids]
            lists = torch.arange(FRAME_LEN, dtype=torch.int32, device=eng.device).repeat(len(ids), 1)
            res = eng.coherent_score_at(M, A, D, np.array([r.rows4 for r in ids], np.int64), np.array([r.col for r in ids], np.int64),
                                        np.array([r.slots for r in ids], np.int32), lists, ring, hop,
                                        np.array([bases.index(v) for v in base], np.int32), np.array(base, np.int64), width)
            score, origin, rank = (t.cpu().numpy() for t in res)
            for k, r in enumerate(ids):
                verdicts[r.clip][r.window] = _verdicts(n_own, score[k], origin[k], rank[k],
                                                       lambda s, o, q: verdict(s, o, q, r.span[0], plist, r.slots, r.col))
    return _maps([[(s, col, FRAME_LEN * J) for s, col, J in ws] for ws in wins], verdicts, n_own, 0.0, confirm)


__all__ = ["MAP_HOP_BYTES", "search", "search_coherent", "search_coherent_map", "search_map"]
