"""The lane-per-path list decoder's per-bit path (leaf penalty on the straight-line softplus with its deferred generic form, even / odd
leaves as two pieces of code, slot-pointer bytes, the all-ascending sort with mirrored-lane stages) through es_scl_batch against oracle.scl_list, bit for bit: candidate bits, metrics,
cand_ok, ncand and the hard decision, at

  * list sizes 1, 2, 3, 4, 8, 16, 33, 64, 128, 256 (every capacity of es_scl_wide.hip, two sizes below their capacity),
  * skip_if_hard_ok 0 and 1, float32 and float64 LLRs,
  * B = 9 and B = 17 frames: at L = 8 a wave holds eight frames, so these are one full wave plus a last wave with ONE frame whose
    other seven frame groups mirror it (and the sort's mirrored lanes hold dead paths' fillers at every list size below its capacity),

on rows of N(0, 3), an all-zero row, a tie-heavy row of +-1e-3, a code word scaled until leaf LLRs pass 512 in magnitude on the CPU (the
deferred generic penalty runs; the scale is checked on the oracle's own f), a row whose second half is zero, and a clean code word
(the hard decision passes: skipped with skip_if_hard_ok).  The rows hold float32 values, so both dtypes decode the same numbers: the
oracle's lists are computed once per list size for the 17 rows and shared by every case."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 8, 16, 33, 64, 128, 256)
NROWS = 17


def _sc_leaf_llrs(oracle, x):
    """Leaf LLRs of plain successive cancellation (the list decoder's path at L = 1) with the oracle's f: -> (1024 leaf LLRs)."""
    frozen, _ = oracle.polar_tables()
    leaf = np.zeros(1024)
    pos = [0]

    def rec(llr):
        n = llr.size
        if n == 1:
            i = pos[0]; pos[0] += 1
            leaf[i] = llr[0]
            return np.array([0 if frozen[i] else int(llr[0] >= 0.0)], np.uint8)
        a, b = llr[:n // 2], llr[n // 2:]
        ul = rec(oracle.polar_f_vec(a, b))
        ur = rec(b + (1.0 - 2.0 * ul) * a)
        return np.concatenate([ul ^ ur, ur])
    rec(np.asarray(x, np.float64))
    return leaf


@pytest.fixture(scope="module")
def rows(oracle):
    rng = np.random.default_rng(2024)
    x = rng.normal(0.0, 3.0, (NROWS, 1024))
    x[1] = 0.0                                                        # all zero: every comparison a tie
    x[2] = np.where(rng.integers(0, 2, 1024) > 0, 1e-3, -1e-3)         # tie-heavy
    code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
    big = np.where(code > 0, 2.0, -2.0)
    big[rng.choice(1024, 5, replace=False)] *= -1.0                   # (so that the hard decision fails and skip_if_hard_ok keeps the row)
    x[3] = big
    x[4, 512:] = 0.0                                                  # second half zero
    x[5] = np.where(code > 0, 3.0, -3.0)                              # a clean code word: the hard decision passes (skip_if_hard_ok skips it)
    x[9] = x[3] * 1.5                                                 # rows 8.. ride in the last wave at B = 9 (row 8 alone) and B = 17 (row 16 alone)
    x[16] = x[2]
    x = x.astype(np.float32).astype(np.float64)                       # the same values in both dtypes
    for r in (3, 9):
        assert np.abs(_sc_leaf_llrs(oracle, x[r])).max() >= 512.0, r   # a leaf passes the straight-line softplus's range on the CPU
        assert oracle.polar_hard(x[r])[1] is False
    assert oracle.polar_hard(x[5])[1] is True
    return x


@pytest.fixture(scope="module")
def lists(oracle, rows):
    """(L) -> per row (hard_info bytes, hard_ok, n, packed candidate rows, metrics, cand_ok); both dtypes hold the same values"""
    hard = [oracle.polar_hard(r) for r in rows]
    cache = {}

    def get(L):
        if L not in cache:
            out = [None] * NROWS

            def work(lo, hi):
                for i in range(lo, hi):
                    n, ci, cm, cc = oracle.scl_list(rows[i], L)
                    out[i] = (np.packbits(hard[i][0]).tobytes(), hard[i][1], n, np.packbits(ci, axis=1), cm, cc)
                return []
            oracle.map_records(work, NROWS, chunk=1)
            cache[L] = out
        return cache[L]
    return get


@pytest.fixture(scope="module")
def eng():
    from echoseal_amd.engine import RxEngine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = RxEngine(0, list_size_max=256)
    e.set_option("scl_multi", 1); e.set_option("scl_lanes", 1)         # one lane per path (es_scl_wide.hip) at every list size
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.mark.parametrize("L", SIZES)
def test_lists_equal_oracle(eng, rows, lists, L):
    want = lists(L)
    for dt in (np.float32, np.float64):
        for B in (9, 17):
            xd = torch.from_numpy(rows[:B].astype(dt)).to(eng.device)
            for skip in (False, True):
                res = eng.scl(xd, list_size=L, skip_if_hard_ok=skip).check()
                ci = res.cand_info.cpu().numpy(); cm = res.cand_metric.cpu().numpy(); cc = res.cand_ok.cpu().numpy()
                nc = res.ncand.cpu().numpy(); hi = res.hard_info.cpu().numpy(); ho = res.hard_ok.cpu().numpy()
                for i in range(B):
                    what = (L, dt.__name__, B, skip, i)
                    hinfo, hok, n, wci, wcm, wcc = want[i]
                    assert hi[i].tobytes() == hinfo and bool(ho[i]) == hok, what
                    if skip and hok:
                        assert int(nc[i]) == 0 and not ci[i].any() and not cm[i].any() and not cc[i].any(), what
                        continue
                    assert int(nc[i]) == n == L, what
                    assert np.array_equal(ci[i], wci), what
                    assert np.array_equal(cm[i].view(np.uint64), wcm.view(np.uint64)), what
                    assert np.array_equal(cc[i], wcc), what

