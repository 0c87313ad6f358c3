"""oracle.map_records (the threaded map the full-size GPU tests compare with) returns exactly what serial calls return.

Workers are threads in one process; the C oracle's calls release the GIL.  Checked on the 256 config-3 windows of
tests/golden/c3_windows.npz through oracle.headline_record (sync, LLR at the first peak, hard decision, SCL-8,
selection) and on scl_list rows at several list sizes, with more threads than the machine may have CPUs."""
import os

import numpy as np
import pytest

from echoseal_amd.tables import pack_tables

KEY = b"\xAA" * 32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _flat(rec):
    """A record's oracle outputs as one comparable tuple of bytes (floats by their bits)."""
    return tuple((k, np.asarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v)) for k, v in sorted(rec.items()))


@pytest.fixture(scope="module")
def c3():
    from echoseal_amd.crypto import SecureChannel
    g = np.load(os.path.join(GOLDEN, "c3_windows.npz"))
    sec = SecureChannel(KEY)
    pn = np.stack([sec.pn_bits(int(c), 1215) for c in g["ctr"]]).astype(np.uint8)
    return g["win"], g["band"].astype(np.int64), pn


def test_threaded_map_equals_serial_on_config3_windows(oracle, c3):
    win, band, pn = c3
    ba, tpl, taps, ntaps, _ = pack_tables()
    n = win.shape[0]
    assert n == 256

    def rec(i):
        b = band[i]
        return oracle.headline_record(win[i], ba[b], tpl[b], taps[b, :ntaps[b]], pn[i], L=8)

    serial = [_flat(rec(i)) for i in range(n)]
    assert len({s for s in serial}) == n                                # distinct records
    listed = sum(not rec(i)["hard_ok"] for i in range(0, n, 8))
    assert listed > 0                                                   # the list decoder is part of what is compared
    for threads, chunk in ((8, 7), (16, 1), (3, 64)):
        got = oracle.map_records(lambda lo, hi: [(i, _flat(rec(i))) for i in range(lo, hi)], n, chunk=chunk, threads=threads)
        assert [i for i, _ in got] == list(range(n))                    # record order, every record once
        assert [s for _, s in got] == serial, (threads, chunk)
    # the way the GPU tests use it: compare inside the worker, return only mismatch descriptors
    want = [rec(i) for i in range(n)]
    bad = dict(want[17]); bad["cand_metric"] = bad["cand_metric"].copy(); bad["cand_metric"][3] = np.nextafter(bad["cand_metric"][3], np.inf)
    bad["llr"] = bad["llr"].copy(); bad["llr"][700] = -bad["llr"][700] if bad["llr"][700] else np.float32(1e-30)
    want[17] = bad

    def cmp(lo, hi):
        out = []
        for i in range(lo, hi):
            r = rec(i)
            for k in ("llr", "cand_metric", "cand_info", "peaks"):
                d = oracle.first_diff(r[k], want[i][k])
                if d is not None:
                    out.append((i, k, d))
        return out
    mism = oracle.map_records(cmp, n, chunk=16)
    assert mism == [(17, "llr", 700), (17, "cand_metric", 3)]


@pytest.mark.parametrize("L", [1, 8, 32])
def test_threaded_map_equals_serial_on_scl_rows(oracle, L):
    rng = np.random.default_rng(40 + L)
    n = 96 if L < 32 else 32
    llr = np.clip(rng.normal(0, 3, (n, 1024)), -12, 12).astype(np.float32).astype(np.float64)
    llr[1] = np.where(rng.integers(0, 2, 1024) == 1, 12.0, -12.0)
    llr[2] = rng.integers(-3, 4, 1024).astype(np.float64)                   # small integers: exact ties
    serial = []
    for i in range(n):
        nn, ci, cm, cc = oracle.scl_list(llr[i], L)
        serial.append((nn, ci.tobytes(), cm.tobytes(), cc.tobytes()))

    def rows(lo, hi):
        out = []
        for i in range(lo, hi):
            nn, ci, cm, cc = oracle.scl_list(llr[i], L)
            out.append((nn, ci.tobytes(), cm.tobytes(), cc.tobytes()))
        return out
    assert oracle.map_records(rows, n, chunk=5, threads=16) == serial
    assert oracle.map_records(rows, n, chunk=5, threads=1) == serial


def test_threaded_map_guards_the_code_size(oracle):
    """The code's K cannot change while a map runs (its tables are shared by the workers); inside code_k a map uses that K."""
    import threading
    started, release = threading.Event(), threading.Event()

    def slow(lo, hi):
        started.set(); release.wait(30); return []
    t = threading.Thread(target=oracle.map_records, args=(slow, 1), kwargs=dict(threads=1))
    t.start()
    try:
        assert started.wait(30)
        with pytest.raises(RuntimeError, match="map_records"):
            with oracle.code_k(512):
                pass
    finally:
        release.set(); t.join()
    assert oracle.polar_tables()[1].size == 448                          # the refused change left K alone
    rng = np.random.default_rng(7)
    x = rng.normal(0, 3, (8, 1024))
    with oracle.code_k(512):
        want = [oracle.polar_hard(r)[0].tobytes() for r in x]
        got = oracle.map_records(lambda lo, hi: [oracle.polar_hard(x[i])[0].tobytes() for i in range(lo, hi)], 8, chunk=1, threads=4)
        assert got == want and len(want[0]) == 504
    assert oracle.polar_tables()[1].size == 448


def test_map_threads_follows_affinity(oracle):
    assert oracle.map_threads() == max(1, min(16, len(os.sched_getaffinity(0))))
