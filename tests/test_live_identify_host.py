"""Live identification without a GPU: the memo's C ABI at the boundary, its record packing, the host twin's insert rules, epochs, and
every refusal of WatermarkIdentifier.open_streams / LiveIdentifier.push -- none of which may need an engine."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "echoseal_hip.h")
KEYS = [bytes([k]) * 32 for k in (1, 2, 3)]


def test_header_declares_and_native_binds_the_memo_entry_points():
    import echoseal_amd._native as nat
    assert nat.CONSTANTS["ES_ABI_VERSION"] == nat.ES_ABI_VERSION == 2
    assert nat.CONSTANTS["ES_MEMO_EMPTY"] == nat.ES_MEMO_EMPTY == 2 ** 64 - 1
    for name, n in (("es_memo_probe_batch", 8), ("es_memo_insert_batch", 8)):
        res, args = nat.SIGNATURES[name]
        decl = nat.DECLARATIONS[name]
        assert res is ctypes.c_int and len(args) == n == len(decl), name
        for a, (ctype, _) in zip(args, decl):                               # the two int64 (slots, n) sit where the header puts them
            assert (a is ctypes.c_int64) == (ctype == "int64_t"), (name, ctype)
    lib = ctypes.CDLL(nat.LIB_PATH)                                          # loads without a GPU
    assert hasattr(lib, "es_memo_probe_batch") and hasattr(lib, "es_memo_insert_batch")
    assert lib.es_abi_version() == 2


def test_slot_function_is_stated_alike_in_header_kernel_source_and_twin():
    from echoseal_amd import memo
    consts = ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB")
    for path in (HEADER, os.path.join(ROOT, "echoseal_amd", "csrc", "es_internal.h"), memo.__file__):
        src = open(path).read()
        assert all(c in src for c in consts), path
    # the finaliser by hand in Python integers, at values that exercise every carry
    m64 = (1 << 64) - 1

    def mix(k0, k1):
        z = (k0 * 0x9E3779B97F4A7C15 + k1) & m64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m64
        return z ^ (z >> 31)
    rng = np.random.default_rng(1)
    k0 = np.concatenate((rng.integers(0, 2 ** 60, 50, dtype=np.uint64), np.array([0, 2 ** 60 - 1], np.uint64)))
    k1 = np.concatenate((rng.integers(0, 2 ** 64, 50, dtype=np.uint64), np.array([0, 2 ** 64 - 1], np.uint64)))
    for slots in (1, 64, 1 << 25):
        assert memo.slot(k0, k1, slots).tolist() == [mix(int(a), int(b)) & (slots - 1) for a, b in zip(k0, k1)]


def test_packing_round_trips_at_the_field_limits():
    from echoseal_amd import memo
    lim = [(0, 2 ** 20 - 1), (0, 2 ** 24 - 1), (0, 2 ** 16 - 1), (0, 2 ** 48 - 1), (0, 2 ** 16 - 1)]
    recs = np.array(np.meshgrid(*lim, indexing="ij")).reshape(5, -1)        # every corner of the five fields
    k0, k1 = memo.pack(*recs)
    assert k0.dtype == k1.dtype == np.uint64 and k0.size == 32
    assert all(np.array_equal(a, b) for a, b in zip(memo.unpack(k0, k1), recs))
    assert not (k0 >> np.uint64(60)).any() and (k0 != memo.EMPTY).all()     # bits 60..63 zero: no record is the empty entry
    assert len({(int(a), int(b)) for a, b in zip(k0, k1)}) == 32
    # neighbouring fields do not bleed into each other
    assert memo.pack(1, 0, 0, 0, 0)[0][0] == 1 and memo.pack(0, 1, 0, 0, 0)[0][0] == 1 << 20 and memo.pack(0, 0, 1, 0, 0)[0][0] == 1 << 44
    assert memo.pack(0, 0, 0, 1, 0)[1][0] == 1 and memo.pack(0, 0, 0, 0, 1)[1][0] == 1 << 48
    for bad in ((2 ** 20, 0, 0, 0, 0), (0, 2 ** 24, 0, 0, 0), (0, 0, 2 ** 16, 0, 0), (0, 0, 0, 2 ** 48, 0), (0, 0, 0, 0, 2 ** 16), (-1, 0, 0, 0, 0)):
        with pytest.raises(ValueError, match="outside"):
            memo.pack(*bad)


def _same_slot(memo, slots, want, start=0):
    """`want` distinct records that all map to one slot of a table of `slots` entries."""
    k0, k1 = memo.pack(7, 3, 0, np.arange(start, start + 4000), 9)
    s = memo.slot(k0, k1, slots)
    pick = np.flatnonzero(s == s[0])[:want]
    assert pick.size == want
    return k0[pick], k1[pick]


def test_twin_insert_lowest_index_wins_masked_ignored_duplicates_harmless():
    from echoseal_amd import memo
    m = memo.MemoModel(64)
    a0, a1 = _same_slot(memo, 64, 3)
    s = int(memo.slot(a0[:1], a1[:1], 64)[0])
    other0, other1 = memo.pack(1, 2, 0, 5, 6)
    # three records contest one slot: index 0 wins, 1 and 2 are dropped
    wrote = m.insert(a0, a1)
    assert wrote.tolist() == [True, False, False] and m.table[s].tolist() == [int(a0[0]), int(a1[0])]
    assert m.probe(a0, a1).tolist() == [True, False, False]
    # the winner masked out: the next lowest index wins, and replaces what the slot held
    k0 = a0.copy(); k0[0] = memo.EMPTY
    wrote = m.insert(k0, a1)
    assert wrote.tolist() == [False, True, False] and m.table[s].tolist() == [int(a0[1]), int(a1[1])]
    assert m.probe(a0, a1).tolist() == [False, True, False]
    # all masked: nothing changes
    before = m.table.copy()
    assert not m.insert(np.full(3, memo.EMPTY), a1).any() and np.array_equal(m.table, before)
    # exact duplicates: one of them is written, the table is as if it were named once
    m2, m3 = memo.MemoModel(64), memo.MemoModel(64)
    m2.insert(np.repeat(a0[2:], 4), np.repeat(a1[2:], 4))
    m3.insert(a0[2:], a1[2:])
    assert np.array_equal(m2.table, m3.table) and m2.probe(a0[2:], a1[2:]).all()
    # a table of one entry holds the lowest record of the last call
    m1 = memo.MemoModel(1)
    m1.insert(a0, a1); m1.insert(other0, other1)
    assert m1.table.tolist() == [[int(other0[0]), int(other1[0])]] and not m1.probe(a0, a1).any()
    m.clear()
    assert (m.table == memo.EMPTY).all() and not m.probe(a0, a1).any()
    for bad in (0, 3, -4, 48):
        with pytest.raises(ValueError, match="power of two"):
            memo.MemoModel(bad)


def test_epoch_bump_makes_old_entries_miss_and_a_wrap_clears():
    from echoseal_amd import memo
    from echoseal_amd.identify import LiveIdentifier, WatermarkIdentifier
    from echoseal_amd.monitor import host_table
    m = memo.MemoModel(256)
    epoch = np.zeros(3, np.int64)
    rec = lambda s: memo.pack([0, 1], [4 * s, 4 * s + 3], epoch[s], [100, 2000], [0, 5])
    m.insert(*rec(1)); m.insert(*rec(2))
    assert m.probe(*rec(1)).all() and m.probe(*rec(2)).all()
    assert memo.bump_epochs(epoch, [1]) is False and epoch.tolist() == [0, 1, 0]
    assert not m.probe(*rec(1)).any() and m.probe(*rec(2)).all()             # the slot's next stream never meets the old verdicts
    epoch[1] = memo.EPOCHS - 1
    assert memo.bump_epochs(epoch, [1, 2]) is True and epoch.tolist() == [0, 0, 1]      # back at a value it has had: the caller must clear
    # LiveIdentifier.close does so (the engine's part of closing replaced: no GPU here)
    class Eng:
        fs, list_size_max = 48_000, 32

        def close_monitor_streams(self, table, ids):
            table.live[ids] = False
    live = LiveIdentifier(WatermarkIdentifier(KEYS, list_size=8, engine=Eng()), host_table(2, 4000, 1000), memo_slots=64)
    calls = []
    live.forget = lambda: calls.append(1)
    live.close([0])
    assert live._epoch.tolist() == [1, 0] and calls == []
    live.table.live[0] = True
    live._epoch[0] = memo.EPOCHS - 1
    live.close([0])
    assert live._epoch.tolist() == [0, 0] and calls == [1]


def test_every_refusal_comes_before_an_engine_is_built(monkeypatch):
    import echoseal_amd.fastpolar as fp
    from echoseal_amd import memo
    from echoseal_amd.identify import LiveIdentifier, WatermarkIdentifier
    from echoseal_amd.monitor import MIN_WINDOW, host_table

    def no_engine(*a, **k):
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(fp, "engine_for_fs", no_engine)
    monkeypatch.setattr(fp, "engine_for_large_list", no_engine)
    ident = WatermarkIdentifier(KEYS, list_size=8)
    with pytest.raises(ValueError, match="at least 2432 samples"):          # bad geometry
        ident.open_streams(4, window_s=(MIN_WINDOW - 1) / 48_000)
    with pytest.raises(ValueError, match="chunk_max"):
        ident.open_streams(4, chunk_max=0)
    with pytest.raises(ValueError, match="2 rates for 4 streams"):          # bad rates
        ident.open_streams(4, fs=[48_000, 44_100])
    # a window whose hop table would be wider than a 16-bit counter: ceil(W / 1215) + 201 > 65535
    w_ok = (memo.MAX_COUNTERS - 201) * 1215
    LiveIdentifier.check_memo(64, 3, w_ok)
    with pytest.raises(ValueError, match="window of .* samples.*counter"):
        LiveIdentifier.check_memo(64, 3, w_ok + 1)
    with pytest.raises(ValueError, match="window of .* samples.*counter"):
        ident.open_streams(1, window_s=(w_ok + 1215) / 48_000, chunk_max=100)
    LiveIdentifier.check_memo(0, 3, w_ok + 1)                               # ... not refused with the memo off
    with pytest.raises(ValueError, match="power of two"):
        ident.open_streams(1, memo_slots=48)
    # more than 2^20 - 1 keys
    many = WatermarkIdentifier([bytes(32)] * (memo.MAX_KEYS + 1), list_size=8)
    with pytest.raises(ValueError, match="1048576 keys"):
        many.open_streams(1)
    LiveIdentifier.check_memo(64, memo.MAX_KEYS, 4000)
    # pushes: the host half of a table, no device arrays
    live = LiveIdentifier(ident, host_table(3, 48_000, 1000), memo_slots=64)
    ok = np.zeros(100, np.float32)
    with pytest.raises(ValueError, match="fs_target"):
        live.push([ok], [0], fs=44_100)
    with pytest.raises(ValueError, match="1-D"):
        live.push([np.zeros((2, 50), np.float32)], [0])
    with pytest.raises(ValueError, match="longer than chunk_max"):
        live.push([np.zeros(1001, np.float32)], [0])
    with pytest.raises(ValueError, match="named twice"):
        live.push([ok, ok], [1, 1])
    with pytest.raises(ValueError, match="one chunk per stream"):
        live.push([ok], [0, 1])
    with pytest.raises(ValueError, match="outside"):
        live.push([ok], [3])
    live.table.live[2] = False
    with pytest.raises(ValueError, match="closed"):
        live.push([ok], [2])
    # a stream at 2^48 - 50 samples: 50 more are fine for the check, 51 are refused by name
    live.table.n_host[1] = memo.MAX_POSITION - 50
    live.table.base_host[1] = (memo.MAX_POSITION - 50 - 48_000) // 1216 * 1216
    with pytest.raises(ValueError, match="stream 1 would pass 2\\^48 samples"):
        live.push([ok, np.zeros(51, np.float32)], [0, 1])
    assert live.position(1) == memo.MAX_POSITION - 50 and live.window(0) == (0, 0) and len(live) == 2 and live.rate(0) == 48_000
    assert live.push([], []) == [] and live.stats == {"planned": 0, "decoded": 0, "skipped": 0}
    assert memo.default_slots(16, 64) == 1 << 22 and memo.default_slots(1, 1) == 1 << 12 and memo.default_slots(10 ** 6, 10 ** 4) == 1 << 25
