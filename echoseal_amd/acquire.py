"""Acquisition on the host: which counters a decoded header may belong to when nobody knows where in its stream a clip or
a window lies, in which order they are tried, and the counter origin a found frame implies -- with a NumPy model that the kernels behind
es_acquire_mask_batch / es_acquire_list_batch (csrc/es_keyring.hip) are held to word for word.  No engine is needed for anything here.

A record is one (key, fitting peak) pair with a header decode: ok, the low 16 bits of the frame's counter, and the band of the sync row the
peak was found in.  Its candidates are the counters (h << 16) | lo16 of the span that hop to that band.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .scan import CTR_END, FRAME_LEN, counter_estimate
from .utils import band_index

FULL_SPAN = (0, CTR_END)


@dataclass
class Acquired:
    """A frame found by acquisition: `ctr` is the counter its payload states, `start` its first sample in the clip or window, `band` the
    (lo, hi) band it was found in.  ctr0 = origin_of(ctr, start, pos0) is the counter origin to verify the clip or stream with.  records:
    the header records that were searched; tried: the candidates decoded up to and including the accepted one."""
    ctr0: int
    ctr: int
    start: int
    band: tuple
    blob: bytes
    plain: bytes
    records: int
    tried: int


def check_span(span) -> tuple[int, int]:
    """A counter span [lo, hi) as two ints with 0 <= lo <= hi <= 2^32; anything else is a ValueError that names it."""
    try:
        lo, hi = span
    except (TypeError, ValueError):
        raise ValueError(f"span = {span!r}: a pair (first counter, one past the last)") from None
    for v in (lo, hi):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"span = {span!r}: counters are integers")
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi > CTR_END:
        raise ValueError(f"span = ({lo}, {hi}) lies outside [0, 2^32] (spans that wrap past 2^32 are out of scope)")
    if lo > hi:
        raise ValueError(f"span = ({lo}, {hi}) is reversed: (first counter, one past the last)")
    return lo, hi


def check_max_records(max_records) -> int:
    if isinstance(max_records, (bool, np.bool_)) or not isinstance(max_records, (int, np.integer)) or int(max_records) < 1:
        raise ValueError(f"max_records = {max_records!r}: at least one header record must be searched")
    return int(max_records)


def span_words(span) -> tuple[int, int, int]:
    """-> (h0, H, W): the first high half of the span, the number of high halves it touches and the 32-bit words of a mask row."""
    lo, hi = check_span(span)
    h0 = lo >> 16
    H = ((hi + 65535) >> 16) - h0
    return h0, H, (H + 31) // 32


def candidates(hop_key: bytes, lo16: int, band: int, span) -> list[int]:
    """The ascending counters c of the span with c & 0xFFFF == lo16 that hop to band index `band` under hop_key (utils.band_index)."""
    lo, hi = check_span(span)
    lo16 = int(lo16)
    if not 0 <= lo16 <= 0xFFFF:
        return []
    h0, H, _ = span_words((lo, hi))
    out = []
    for h in range(h0, h0 + H):
        c = (h << 16) | lo16
        if lo <= c < hi and band_index(hop_key, c) == int(band):
            out.append(c)
    return out


def mask_model(keys, key_idx, ok, lo16, band, span):
    """es_acquire_mask_batch in NumPy: keys = the ring's hop keys -> (mask uint32 [P, W], count int32 [P], candidates per record)."""
    h0, _, W = span_words(span)
    P = len(key_idx)
    mask, count, cands = np.zeros((P, W), np.uint32), np.zeros(P, np.int32), []
    for p in range(P):
        live = bool(ok[p]) and 0 <= int(key_idx[p]) < len(keys)
        cs = candidates(keys[int(key_idx[p])], int(lo16[p]), int(band[p]), span) if live else []
        for c in cs:
            j = (c >> 16) - h0
            mask[p, j >> 5] |= np.uint32(1 << (j & 31))
        count[p] = len(cs)
        cands.append(cs)
    return mask, count, cands


def list_model(cands, base, rec_out: np.ndarray, ctr_out: np.ndarray) -> None:
    """es_acquire_list_batch in NumPy over mask_model's candidates, into the caller's arrays: only the named ranges are written."""
    for p, cs in enumerate(cands):
        b = int(base[p])
        if b >= 0 and cs:
            rec_out[b:b + len(cs)] = p
            ctr_out[b:b + len(cs)] = np.array(cs, np.int64).astype(ctr_out.dtype)


def origin_of(ctr: int, start: int, pos0: int = 0) -> int:
    """The counter origin that makes scan.counter_estimate(start, pos0, origin) land on ctr: ctr - round((pos0 + start) / 1215), or 0
    where that would be negative (the estimate is then above ctr, by less than the planner's window in every real case)."""
    return max(0, int(ctr) - (2 * (int(pos0) + int(start)) + FRAME_LEN) // (2 * FRAME_LEN))


def record_order(ok, lo16, band_place, starts, pos0: int = 0, max_records: int = 8) -> list[int]:
    """Which header records of one clip or window are searched, and in which order.  The arrays run over the fitting peaks in (band row,
    peak) order, band_place = the row's place in the detector's band order.  Of the records with ok: r = (lo16 - estimate) & 0xFFFF with
    estimate = round((pos0 + start) / 1215) is what the headers of one stream's consecutive frames agree on, so records are sorted by
    (-number of records sharing their r, band place, peak order) and the first max_records are kept -> indices into the arrays."""
    idx = [j for j in range(len(ok)) if ok[j] and 0 <= int(lo16[j]) <= 0xFFFF]
    res = {j: (int(lo16[j]) - counter_estimate(int(starts[j]), pos0)) & 0xFFFF for j in idx}
    share: dict[int, int] = {}
    for j in idx:
        share[res[j]] = share.get(res[j], 0) + 1
    idx.sort(key=lambda j: (-share[res[j]], int(band_place[j]), j))
    return idx[:check_max_records(max_records)]


__all__ = ["Acquired", "FULL_SPAN", "candidates", "check_max_records", "check_span", "list_model", "mask_model", "origin_of", "record_order",
           "span_words"]
