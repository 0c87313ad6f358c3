"""WatermarkIdentifier: which of many keys marked a recording?

For a clip and keys k_0 .. k_{N-1} the answer for key k_i is exactly what a freshly built
WatermarkDetector(k_i, fs_target=..., list_size=...).verify(clip, fs_in) gives (same boolean, same tries in the same order, and for a
match the blob it accepted) -- that single-key path, pinned to the reference by tests/golden/, is the definition.  What differs is the
work: the key-independent half of the search (conditioning, four band-passes, four correlation rows, peak picking) runs once per clip,
and everything keyed runs for all keys at once from a key ring on the device:

    keys -> es_keyring_derive_batch                      (rtwm/crypto.py:19-30, rtwm/utils.py:86-88)
    header decode per (key, peak) -> es_header_at_batch  (rtwm/detector.py:452-515)
    hop table per (key, counter) -> es_schedule_keyed_batch, bands only
    candidate planning per (key, clip, band) -> es_plan_batch                  (rtwm/detector.py:105-142)
    band rank by band rank (rank 0 = each key's band of counter 0): es_schedule_keyed_batch -> es_llr_at_batch x 2 variants ->
    es_scl_batch -> es_select_keyed_batch over the candidates of every key still unmatched

Each key starts with session_nonce = None, so a key matches iff some candidate of its walk validates (AEAD opens, "ESAL", counter
equal), and the first such candidate in the reference's walk order is the reported one.  Nonce state across calls is out of scope.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from ._native import ES_MAX_PEAKS, ES_MAX_TRIES, NativeError
from .detector import FRAME_LEN, MAX_TRIES, PEAK_LIMIT, TIGHT_DELTA, WIDE_DELTA, WatermarkDetector
from .scan import cut_launches, sync_launch
from .utils import BAND_PLAN

assert MAX_TRIES == ES_MAX_TRIES
NB = len(BAND_PLAN)
PAIR_BUDGET = 1 << 16           # (key, clip-band) pairs planned per call: the bounded candidate table is 2 000 bytes per pair


@dataclass
class KeyMatch:
    key: int            # index into the identifier's key list
    ctr: int            # frame counter of the accepted candidate
    band: int           # index into BAND_PLAN
    start: int          # peak (sample offset of the frame in the conditioned clip)
    variant: int        # 0..3: +llr0, -llr0, +llr1, -llr1 (rtwm/detector.py:161-190)
    blob: bytes         # the 55 bytes the validator accepted
    plain: bytes        # their 27-byte plaintext


def ctr_estimate(start: int) -> int:
    """round(start / 1215) in integers: 1215 is odd, so start / 1215 never lies on a tie."""
    return (2 * int(start) + FRAME_LEN) // (2 * FRAME_LEN)


def plan_reference(peaks, npeaks: int, M: int, band: int, hdr_ok, hdr_lo16, hop):
    """Host twin of es_plan_batch for one (key, row): the rules of WatermarkDetector._scan_plan (rtwm/detector.py:105-142) restated
    on the kernel's inputs.  peaks: the row's ES_MAX_PEAKS sync peaks, npeaks: its raw count word, M: samples per record, band: the
    row's band index, hdr_ok / hdr_lo16: header results of the row's fitting peaks in order, hop[ctr]: band index of the key's
    counters.  -> (plan [(peak slot, ctr)] in try order, fitting peaks looked at)."""
    plan: list[tuple[int, int]] = []
    looked = 0
    n = min(int(npeaks) & 0xFFFF, ES_MAX_PEAKS, PEAK_LIMIT)
    for slot in range(n):
        start = int(peaks[slot])
        if start < 0 or start + FRAME_LEN > M:
            continue
        if len(plan) >= MAX_TRIES:
            break
        j = looked
        looked += 1
        est = ctr_estimate(start)
        wide = range(max(0, est - WIDE_DELTA), est + WIDE_DELTA + 1)
        if hdr_ok[j]:
            cands = [c for c in wide if (c & 0xFFFF) == int(hdr_lo16[j]) and hop[c] == band]
        else:
            cands = [c for c in range(max(0, est - TIGHT_DELTA), est + TIGHT_DELTA + 1) if hop[c] == band]
            if not cands:
                cands = [c for c in wide if hop[c] == band]
        plan += [(slot, c) for c in cands[:MAX_TRIES - len(plan)]]
    return plan, looked


class WatermarkIdentifier:
    """identify(audio, fs_in) -> one entry per key: a KeyMatch, or None where WatermarkDetector(key).verify would return False.
    With `.trace = True` a call returns (matches, traces), traces[i] = (the `_trace`, the `_hdr_trace`) a fresh detector of key i
    would have recorded."""

    def __init__(self, keys, *, fs_target: int = 48_000, list_size: int = 256, engine=None) -> None:
        self.keys = [bytes(k) for k in keys]
        if any(len(k) != 32 for k in self.keys):
            raise ValueError("master_key must be 32 bytes (256 bit)")
        self.fs_target = fs_target
        self._list_size = int(list_size)
        self.trace = False
        # conditioning, sync and the engine choice are the detector's; its key plays no part in what is used of it
        self._det = WatermarkDetector(self.keys[0] if self.keys else bytes(32), fs_target=fs_target, list_size=list_size, engine=engine)
        self._ring = None

    @property
    def engine(self):
        return self._det.engine

    def _pair_cap(self) -> int:
        return self._det._pair_cap()

    def identify(self, audio, fs_in: int):
        res = self.identify_batch([audio], fs_in)
        return (res[0][0], res[1][0]) if self.trace else res[0]

    def identify_batch(self, clips, fs_in):
        """identify() for several recordings -> one list of per-key entries per clip (with .trace: (those, per clip the per-key
        traces)).  Clips of one sample type share their launches whatever their lengths (scan.cut_launches)."""
        N = len(self.keys)
        clips = list(clips)
        out = [[None] * N for _ in clips]
        traces = [[([], []) for _ in range(N)] for _ in clips]
        if N:
            fs_list = list(fs_in) if isinstance(fs_in, (list, tuple)) else [fs_in] * len(clips)
            per_call = max(1, PAIR_BUDGET // (N * NB))
            for la in cut_launches(clips, fs_list, self.fs_target, NB, self._det._conditioned):      # (clips shorter than the template are in none)
                for at in range(0, len(la.idx), per_call):
                    part = la.part(at, at + per_call)
                    self._group(part, [out[i] for i in part.idx], [traces[i] for i in part.idx])
        return (out, traces) if self.trace else out

    # ------------------------------------------------------------------ one group of clips that share their launches
    def _group(self, launch, out, traces) -> None:
        import torch
        eng = self.engine
        dev = eng.device
        N, g = len(self.keys), len(launch.idx)
        R = g * NB                                                          # sync rows: row = clip * 4 + band index
        if self._ring is None or self._ring.ring.device != dev:
            self._ring = eng.keyring(self.keys)
        ring = self._ring
        scan = sync_launch(eng, launch, range(NB))                           # conditioning + sync once, whatever the number of keys
        sy, y, rows_a, starts = scan.sy, scan.sy.y, scan.rows, scan.starts   # the P fitting peaks, in (row, peak) order
        if not rows_a.size:                                                 # no peak can hold a frame: nothing to try for any key
            return
        sizes = np.array(scan.sizes, np.int32)
        M = int(sizes.max())                                                # the longest clip: row length of the sync call
        M_rows = np.repeat(sizes, NB)                                       # samples of each sync row's own clip
        P = rows_a.size
        base = np.searchsorted(rows_a, np.arange(R)).astype(np.int32)
        # one header decode over (key, fitting peak), key-major, each key with its own header PN
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
        okh, val, score = eng.header(y, t(np.tile(rows_a % NB, N), np.uint8), ring.hdr_pn.repeat_interleave(P, dim=0),
                                     rows=t(np.tile(rows_a, N), np.int32), start=t(np.tile(starts, N), np.int32))
        # hop table: band of (key, counter) for every counter a window can reach
        C = -(-M // FRAME_LEN) + WIDE_DELTA + 1
        kk = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(C)
        cc = torch.arange(C, dtype=torch.int64, device=dev).repeat(N)
        _, hop = eng.schedule_keyed(ring, kk, cc, want_pn=False)
        rowband = np.tile(np.arange(NB, dtype=np.uint8), g)
        plan = eng.plan(sy.peaks, sy.npeaks, rowband, base, M if int(sizes.min()) == M else M_rows, okh.reshape(N, P), val.reshape(N, P),
                        hop.reshape(N, C))
        count = plan.count.cpu().numpy().astype(np.int64).reshape(N, R)
        hop0 = ring.hop0.cpu().numpy().astype(np.int64)
        order = np.array([[h] + [b for b in range(NB) if b != h] for h in range(NB)], np.int64)[hop0]      # [N, 4]: rtwm/detector.py:46-52
        pk_h = sy.peaks.cpu().numpy()
        if self.trace:
            looked = plan.looked.cpu().numpy().reshape(N, R)
            hdr_h = (okh.cpu().numpy().reshape(N, P), val.cpu().numpy().reshape(N, P), score.cpu().numpy().astype(np.float64).reshape(N, P))
            fit = (pk_h >= 0) & (pk_h + FRAME_LEN <= M_rows[:, None]) & (np.arange(ES_MAX_PEAKS)[None, :] < np.minimum(sy.npeaks.cpu().numpy() & 0xFFFF, PEAK_LIMIT)[:, None])
            fit_rank = np.cumsum(fit, axis=1) - 1                           # header-log index of a peak slot

            def hdr_log(k, r, n):
                j = k, slice(int(base[r]), int(base[r]) + n)
                return [(float(bool(a)), float(b), float(c)) for a, b, c in zip(hdr_h[0][j], hdr_h[1][j], hdr_h[2][j])]
        alive = np.ones((N, g), bool)
        found: list = []                                                    # (key, clip, ctr, band, start, variant, blob row)
        cap = max(1, int(self._pair_cap()))
        L = self._list_size
        if L > eng.list_size_max:
            raise NotImplementedError(f"list_size={L}: the HIP decoder supports list sizes up to {eng.list_size_max}")
        for rank in range(NB):
            ks, cs = np.nonzero(alive)                                      # key-major: candidates arrive sorted by key
            if not ks.size:
                break
            rs = cs * NB + order[ks, rank]
            cnt = count[ks, rs]
            total = int(cnt.sum())
            first = np.full(ks.size, -1, np.int64)                          # per pair: its first validated candidate (index into the flat list)
            if total:
                pair_of = np.repeat(np.arange(ks.size), cnt)
                pos = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                flat = t((ks[pair_of] * R + rs[pair_of]) * ES_MAX_TRIES + pos, np.int64)
                ctr_d = plan.ctr.reshape(-1)[flat]
                slot_d = plan.slot.reshape(-1)[flat].to(torch.int64)
                row_d = t(rs[pair_of], np.int64)
                start_d = sy.peaks.reshape(-1)[row_d * ES_MAX_PEAKS + slot_d]
                key_d = t(ks[pair_of], np.int32)
                row_d = row_d.to(torch.int32)
                ok_all = np.empty((total, 4), np.int8)
                blobs: dict[int, np.ndarray] = {}
                for a in range(0, total, cap):
                    b = min(total, a + cap)
                    n = b - a
                    pn, bands = eng.schedule_keyed(ring, key_d[a:b], ctr_d[a:b])
                    l0 = eng.llr(y, bands, pn, variant=0, rows=row_d[a:b], start=start_d[a:b])
                    l1 = eng.llr(y, bands, pn, variant=1, rows=row_d[a:b], start=start_d[a:b])
                    res = eng.scl(torch.cat((l0, -l0, l1, -l1), dim=0), list_size=L, skip_if_hard_ok=False)
                    payload, ok, _which = eng.select(res, ring=ring, key_idx=key_d[a:b].repeat(4), ctrs=ctr_d[a:b].repeat(4))
                    okc = ok.cpu().numpy().reshape(4, n).T
                    if (okc == -2).any():
                        raise NativeError("es_scl_batch: some candidate records were not decoded (no free scratch-slab slot)")
                    ok_all[a:b] = okc
                    hit = np.flatnonzero((okc == 1).any(axis=1))
                    if hit.size:
                        v = np.argmax(okc[hit] == 1, axis=1)                # the first of +llr0, -llr0, +llr1, -llr1 that validates
                        got = payload[t(v * n + hit, np.int64)].cpu().numpy()
                        for i, vv, row in zip(hit, v, got):
                            blobs[a + int(i)] = (int(vv), row)
                hits = np.flatnonzero((ok_all == 1).any(axis=1))
                if hits.size:
                    pairs, where = np.unique(pair_of[hits], return_index=True)      # hits ascend: the first hit of each pair
                    first[pairs] = hits[where]
                ctr_h = ctr_d.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                start_h = start_d.cpu().numpy().astype(np.int64)
                for p in np.flatnonzero(first >= 0):
                    i = int(first[p])
                    vv, blob = blobs[i]
                    found.append((int(ks[p]), int(cs[p]), int(ctr_h[i]), int(order[ks[p], rank]), int(start_h[i]), vv, blob))
            if self.trace:
                off = np.cumsum(cnt) - cnt
                slot_h = slot_d.cpu().numpy() if total else None
                for p in range(ks.size):
                    k, c, r = int(ks[p]), int(cs[p]), int(rs[p])
                    tr, ht = traces[c][k]
                    lo = int(BAND_PLAN[order[k, rank]][0])
                    end = int(first[p]) + 1 if first[p] >= 0 else int(off[p] + cnt[p])
                    tr.extend((lo, int(start_h[i]), int(ctr_h[i])) for i in range(int(off[p]), end))
                    # the reference decodes a peak's header when it reaches the peak: peaks after the accepted one were never looked at
                    ht.extend(hdr_log(k, r, int(fit_rank[r, slot_h[first[p]]]) + 1 if first[p] >= 0 else int(looked[k, r])))
            alive[ks[first >= 0], cs[first >= 0]] = False                   # keys that matched leave before the next rank
        if found:
            kd = np.array([f[0] for f in found], np.int64)
            blob_rows = np.stack([f[6] for f in found])
            ok, plain = eng.aead_check_keyed(ring, torch.from_numpy(kd).to(dev), torch.from_numpy(blob_rows).to(dev),
                                             torch.tensor([f[2] for f in found], dtype=torch.int64), want_plain=True)
            ok = ok.cpu().numpy(); plain = plain.cpu().numpy()
            for f, o, pt in zip(found, ok, plain):
                if o != 1:
                    raise NativeError("es_select_keyed_batch accepted a blob that es_aead_check_keyed_batch rejects")
                out[f[1]][f[0]] = KeyMatch(f[0], f[2], f[3], f[4], f[5], f[6].tobytes(), pt.tobytes())


__all__ = ["KeyMatch", "WatermarkIdentifier", "plan_reference", "ctr_estimate"]
