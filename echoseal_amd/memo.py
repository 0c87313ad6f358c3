"""The verdict memo of live identification on the host: how records are packed, where they live, and a NumPy model of the
table that the kernels of csrc/es_memo.hip are held to byte for byte.  No engine is needed for anything here.

A record names one candidate that is known to fail: (key index, history row 4 s + j, epoch of stream slot s, absolute start, counter).
The table is direct-mapped: a record lives at slot(k0, k1) or nowhere, an entry is the record itself, and an empty entry is all ones.
"""
from __future__ import annotations

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
KEY_BITS, ROW_BITS, EPOCH_BITS, START_BITS, CTR_BITS = 20, 24, 16, 48, 16      # k0 = key | row << 20 | epoch << 44; k1 = start | ctr << 48
MAX_KEYS = (1 << KEY_BITS) - 1              # keys a live identifier with a memo takes
MAX_COUNTERS = (1 << CTR_BITS) - 1          # ... and the width of its hop table, ceil(W / 1215) + 201
MAX_POSITION = 1 << START_BITS              # ... and the samples a stream may have received
EPOCHS = 1 << EPOCH_BITS
MAX_SLOTS = 1 << 25                         # 512 MiB of entries (+ 128 MiB of claim words): the table stays under 1 GiB
MIN_SLOTS = 1 << 10

_U = np.uint64


def pack(key_idx, row, epoch, start, ctr):
    """-> (k0, k1) uint64 arrays.  A field outside its bits is a ValueError: a truncated field would make two candidates one record."""
    f = [np.asarray(v, dtype=np.int64).reshape(-1) for v in (key_idx, row, epoch, start, ctr)]
    n = max(a.size for a in f)
    f = [np.broadcast_to(a, (n,)) if a.size == 1 else a for a in f]
    for a, bits, what in zip(f, (KEY_BITS, ROW_BITS, EPOCH_BITS, START_BITS, CTR_BITS), ("key index", "history row", "epoch", "absolute start", "counter")):
        if a.size != n:
            raise ValueError("memo records: one value per record in every field")
        if n and (a.min() < 0 or a.max() >= (1 << bits)):
            raise ValueError(f"memo record: {what} outside [0, 2^{bits})")
    k, r, e, s, c = (a.astype(_U) for a in f)
    return k | (r << _U(KEY_BITS)) | (e << _U(KEY_BITS + ROW_BITS)), s | (c << _U(START_BITS))


DELTA_MAX = 400                             # a candidate lies within +-200 counters of its peak's estimate


def pack_abs(key_idx, row, epoch, start, delta):
    """pack() for the candidates of a stream with a counter origin: the 16-bit counter field holds
    delta = ctr - ctr_est(start) + 200, with ctr_est(start) = origin + round(start / 1215) of the record's absolute start -- 0 .. 400 by
    the planner's rules.  The origin is a function of (stream slot, epoch), both in the record, so the record still names one candidate
    whatever the size of its counter.  A delta outside 0 .. 400 is a ValueError."""
    d = np.asarray(delta, dtype=np.int64).reshape(-1)
    if d.size and (d.min() < 0 or d.max() > DELTA_MAX):
        raise ValueError(f"memo record: counter delta outside [0, {DELTA_MAX}] (a candidate more than 200 counters from its peak's estimate)")
    return pack(key_idx, row, epoch, start, d)


def unpack(k0, k1):
    """-> (key index, history row, epoch, absolute start, counter) int64 arrays of packed records."""
    k0, k1 = np.asarray(k0, _U), np.asarray(k1, _U)
    m = lambda bits: _U((1 << bits) - 1)
    return tuple(a.astype(np.int64) for a in (k0 & m(KEY_BITS), (k0 >> _U(KEY_BITS)) & m(ROW_BITS), (k0 >> _U(KEY_BITS + ROW_BITS)) & m(EPOCH_BITS),
                                              k1 & m(START_BITS), k1 >> _U(START_BITS)))


def slot(k0, k1, slots: int) -> np.ndarray:
    """The entry of record (k0, k1): the splitmix64 finaliser over k0 * 0x9E3779B97F4A7C15 + k1 (mod 2^64), masked by slots - 1 -- the
    one other statement of es_memo_mix (csrc/es_internal.h, include/echoseal_hip.h)."""
    with np.errstate(over="ignore"):
        z = np.asarray(k0, _U) * _U(0x9E3779B97F4A7C15) + np.asarray(k1, _U)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        z = z ^ (z >> _U(31))
    return (z & _U(int(slots) - 1)).astype(np.int64)


def check_slots(slots: int) -> int:
    slots = int(slots)
    if slots < 1 or slots & (slots - 1):
        raise ValueError(f"memo_slots = {slots}: a power of two (or 0: no memo)")
    return slots


def default_slots(n_keys: int, n_streams: int) -> int:
    """The next power of two above 2 x keys x 4 streams x 400 -- twice the candidates of a tick in which no key matches anything --,
    at least 2^10 and at most 2^25 entries (512 MiB of entries and 128 MiB of claim words)."""
    want = 2 * max(1, int(n_keys)) * 4 * max(1, int(n_streams)) * 400
    return min(MAX_SLOTS, max(MIN_SLOTS, 1 << int(want).bit_length()))


class MemoModel:
    """The table as es_memo_probe_batch / es_memo_insert_batch leave it: `table` [slots, 2] uint64."""

    def __init__(self, slots: int) -> None:
        self.slots = check_slots(slots)
        self.table = np.full((self.slots, 2), EMPTY, _U)

    def clear(self) -> None:
        self.table[:] = EMPTY

    def probe(self, k0, k1) -> np.ndarray:
        k0, k1 = np.asarray(k0, _U).reshape(-1), np.asarray(k1, _U).reshape(-1)
        e = self.table[slot(k0, k1, self.slots)]
        return (e[:, 0] == k0) & (e[:, 1] == k1)

    def insert(self, k0, k1) -> np.ndarray:
        """One call: per slot the record of the lowest index replaces the entry, the others are dropped; k0 == EMPTY masks a record out.
        -> bool per record: it was written."""
        k0, k1 = np.asarray(k0, _U).reshape(-1), np.asarray(k1, _U).reshape(-1)
        live = np.flatnonzero(k0 != EMPTY)
        s = slot(k0[live], k1[live], self.slots)
        _, first = np.unique(s, return_index=True)                          # the first occurrence of each slot: its lowest record index
        win = live[first]
        self.table[s[first], 0], self.table[s[first], 1] = k0[win], k1[win]
        wrote = np.zeros(k0.size, bool)
        wrote[win] = True
        return wrote


def bump_epochs(epoch: np.ndarray, ids) -> bool:
    """Closing stream slots `ids`: their epochs move on, so that whoever opens the slot next never meets the old stream's records.
    -> True where an epoch wrapped to 0: records of its first life could be met again, and the caller clears the whole table."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    epoch[ids] = (epoch[ids] + 1) % EPOCHS
    return bool(ids.size and (epoch[ids] == 0).any())


__all__ = ["EMPTY", "MAX_KEYS", "MAX_COUNTERS", "MAX_POSITION", "MemoModel", "bump_epochs", "check_slots", "default_slots", "pack", "pack_abs", "slot", "unpack"]
