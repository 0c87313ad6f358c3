"""The lane-per-path list decoder's shared depth-2 level at bit 512 (es_scl_wide.hip): in one-wave blocks with eight or more lanes per
frame and float32 LLRs, the frame's lanes evaluate the four possible values of each of the 256 elements once between them, and every
path then takes its own from the lane that holds it, chosen by two bits of its 512-bit partial-sum block (ds_bpermute).  Through es_scl_batch (RxEngine.scl)
against oracle.scl_list / oracle.polar_hard, bit for bit: candidate bits, metrics as uint64, cand_ok, ncand and the hard decision, at

  * list sizes 5, 8, 16, 33, 64 (the shared path; 5 and 33 sit below their capacity, so dead lanes evaluate table entries too) and
    4 and 128 (fewer than eight lanes per frame / blocks of several waves: the arms that keep the per-path evaluation), as controls,
  * skip_if_hard_ok 0 and 1, float32 and float64 LLRs holding the same float32 values (float64 launches keep depth 1 in the slab),
  * B = 9 and B = 17 frames: at L = 8 one full wave plus a last wave with ONE frame whose other seven frame groups mirror it,

on rows of N(0, 3), a code word with erasures that keep paths apart below bit 256, an all-zero row, a tie-heavy row of +-1e-3, rows
whose second half, first half (both signs then give the same operand: -0.0 against +0.0) or second and fourth quarter are zero, a code word of +-300 with a few sign flips (depth-2 operands pass 512
in magnitude, so the generic softplus runs inside the shared evaluation; checked on the CPU) and a clean code word that the hard
decision settles.  The oracle's lists are computed once per list size for the 17 rows and shared by every case.

That one broken table column cannot pass is checked on the CPU: at L = 8 the eight paths of the oracle's list at bit 512 read every one
of the four columns on each N(0, 3) row, and all four on ONE element on the erased code word (an N(0, 3) row's paths share bits 0..255
by then, so a single element sees two of its four values there)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHARED = (5, 8, 16, 33, 64)
CONTROLS = (4, 128)
NROWS = 17
NORMAL = (0, 9, 10, 11, 12, 13, 14, 15)            # rows of plain N(0, 3)
ERASED = (4, 67, 84, 96, 130, 151, 192, 222, 236)  # row 8: a code word with these positions erased


def _sc_left_partial_sums(oracle, x):
    """The 512-bit partial-sum block of plain successive cancellation over bits 0..511, with the oracle's f."""
    frozen, _ = oracle.polar_tables()
    pos = [0]

    def rec(llr):
        n = llr.size
        if n == 1:
            i = pos[0]; pos[0] += 1
            return np.array([0 if frozen[i] else int(llr[0] >= 0.0)], np.uint8)
        a, b = llr[:n // 2], llr[n // 2:]
        ul = rec(oracle.polar_f_vec(a, b))
        ur = rec(b + (1.0 - 2.0 * ul) * a)
        return np.concatenate([ul ^ ur, ur])
    x = np.asarray(x, np.float64)
    return rec(oracle.polar_f_vec(x[:512], x[512:]))


@pytest.fixture(scope="module")
def rows(oracle):
    rng = np.random.default_rng(512)
    x = rng.normal(0.0, 3.0, (NROWS, 1024))
    x[1] = 0.0                                                        # all zero: every comparison a tie
    x[2] = np.where(rng.integers(0, 2, 1024) > 0, 1e-3, -1e-3)         # tie-heavy
    x[3, 512:] = 0.0                                                  # depth 1 of the right half is +-llr[j]
    x[4, :512] = 0.0                                                  # both signs give the same operand (llr[j + 512] +- 0.0)
    x[5, 256:512] = 0.0; x[5, 768:] = 0.0                             # the second operand of every pair is zero
    code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
    big = np.where(code > 0, 300.0, -300.0)
    big[rng.choice(1024, 5, replace=False)] *= -1.0                   # (so that the hard decision fails and skip_if_hard_ok keeps the row)
    x[6] = big
    x[7] = np.where(code > 0, 3.0, -3.0)                              # a clean code word: the hard decision passes (skip_if_hard_ok skips it)
    x[16] = big                                                       # ... and alone in the last wave at B = 17
    code8 = oracle.polar_encode(np.random.default_rng(7).integers(0, 2, 440, dtype=np.uint8))
    x[8] = np.where(code8 > 0, 4.0, -4.0); x[8, list(ERASED)] = 0.0   # erasures in the first quarter leave early bits open: the list still holds
                                                                      # paths that differ below bit 256 at bit 512 (alone in the last wave at B = 9)
    x = x.astype(np.float32).astype(np.float64)                       # the same values in both dtypes
    # the +-300 row: operands of the depth-2 f at bit 512 whose sum or difference passes the straight-line softplus's range
    ul = _sc_left_partial_sums(oracle, x[6]).astype(np.float64)
    d1 = x[6, 512:] + (1.0 - 2.0 * ul) * x[6, :512]
    a, b = d1[:256], d1[256:]
    assert max(np.abs(a + b).max(), np.abs(a - b).max()) >= 512.0
    assert np.isfinite(oracle.polar_f_vec(a, b)).all()
    assert oracle.polar_hard(x[6])[1] is False
    assert oracle.polar_hard(x[7])[1] is True
    return x


@pytest.fixture(scope="module")
def lists(oracle, rows):
    """(L) -> per row (hard_info bytes, hard_ok, n, packed candidate rows, metrics, cand_ok, candidate bits); both dtypes hold the same values"""
    hard = [oracle.polar_hard(r) for r in rows]
    cache = {}

    def get(L):
        if L not in cache:
            out = [None] * NROWS

            def work(lo, hi):
                for i in range(lo, hi):
                    n, ci, cm, cc = oracle.scl_list(rows[i], L)
                    out[i] = (np.packbits(hard[i][0]).tobytes(), hard[i][1], n, np.packbits(ci, axis=1), cm, cc, ci)
                return []
            oracle.map_records(work, NROWS, chunk=1)
            cache[L] = out
        return cache[L]
    return get


def _list_decode(oracle, x, L):
    """The oracle's list decoder (oracle/c/eso_polar.c: eso_scl_list) restated over its own f and penalty, all paths at once, so that the
    list can be looked at midway: -> (the paths' 512-bit partial-sum blocks when bit 512 opens, final candidate bits, final metrics)."""
    frozen, dpos = oracle.polar_tables()
    chan = np.asarray(x, np.float64)[None, :]
    alpha = np.zeros((1, 1024)); beta = np.zeros((1, 11, 1024), np.uint8); u = np.zeros((1, 1024), np.uint8); metric = np.zeros(1)
    at512 = None
    for i in range(1024):
        if i == 512:
            at512 = beta[:, 1, :512].copy()
        P = metric.size
        top = 1 if i == 0 else 10 - ((i & -i).bit_length() - 1)
        for lev in range(top, 11):
            size = 1024 >> lev; node = i >> (10 - lev)
            par = np.broadcast_to(chan, (P, 1024)) if lev == 1 else alpha[:, 2 * size:4 * size]
            a, b = np.ascontiguousarray(par[:, :size]), np.ascontiguousarray(par[:, size:])
            if node & 1:
                bl = beta[:, lev, (node - 1) * size:node * size]
                alpha[:, size:2 * size] = b + (1.0 - 2.0 * bl) * a
            else:
                alpha[:, size:2 * size] = oracle.polar_f_vec(a.ravel(), b.ravel()).reshape(P, size)
        lam = np.ascontiguousarray(alpha[:, 1])
        if frozen[i]:
            metric = metric + oracle.penalty_vec(lam, 0)
            bits = np.zeros(P, np.uint8)
        else:
            cm = np.stack([metric + oracle.penalty_vec(lam, 0), metric + oracle.penalty_vec(lam, 1)], axis=1).ravel()    # (path, bit) order
            keep = np.argsort(cm, kind="stable")[:L]
            src = keep >> 1; bits = (keep & 1).astype(np.uint8)
            alpha, beta, u, metric = alpha[src], beta[src], u[src], cm[keep]
        u[:, i] = bits
        lev, node = 10, i
        beta[:, 10, i] = bits
        while (node & 1) and lev > 0:
            size = 1024 >> lev
            left = beta[:, lev, (node - 1) * size:node * size]; right = beta[:, lev, node * size:(node + 1) * size]
            o = (node >> 1) * 2 * size
            beta[:, lev - 1, o:o + size] = left ^ right
            beta[:, lev - 1, o + size:o + 2 * size] = right
            node >>= 1; lev -= 1
    order = np.argsort(metric, kind="stable")
    return at512, u[order][:, dpos[:440]], metric[order]


def test_oracle_paths_use_all_four_sign_combinations(oracle, rows, lists):
    """Element j of the level takes its two signs from bits j and j + 256 of a path's 512-bit partial-sum block.  On the erased code word
    (row 8) the eight paths of the oracle's list at bit 512 show all four pairs on one element.  On an N(0, 3) row they cannot: its eight
    paths differ in the last information bits before 512 only (448..452), so they share bits 0..255, bit j ^ bit j + 256 is the same for
    all of them and an element sees two of its four values -- which two changes from element to element, and every row's list reads each
    of the four table columns on some element.  Either way no column can be wrong and the lists still come out right.
    (The restated decoder is held to the oracle's own candidates and metrics, bit for bit, before its midway state is trusted.)"""
    want = lists(8)
    for r in NORMAL + (8,):
        at512, ci, cm = _list_decode(oracle, rows[r], 8)
        assert np.array_equal(ci, want[r][6]) and np.array_equal(cm.view(np.uint64), want[r][4].view(np.uint64)), r
        assert at512.shape == (8, 512)
        combos = np.zeros((256, 4), bool)
        for k in range(8):
            combos[np.arange(256), at512[k, :256] | (at512[k, 256:] << 1)] = True
        assert combos.any(axis=0).all(), r                            # every column is read
        assert combos.sum(axis=1).max() >= 2, r                       # ... and paths of one list read different columns of one element
        if r == 8:
            assert combos.all(axis=1).any()                           # all four columns of one element


@pytest.fixture(scope="module")
def eng():
    from echoseal_amd.engine import RxEngine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = RxEngine(0, list_size_max=128)
    e.set_option("scl_multi", 1); e.set_option("scl_lanes", 1)         # one lane per path (es_scl_wide.hip) at every list size
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.mark.parametrize("L", SHARED + CONTROLS)
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
                    hinfo, hok, n, wci, wcm, wcc, _ = want[i]
                    assert hi[i].tobytes() == hinfo and bool(ho[i]) == hok, what
                    if skip and hok:
                        assert int(nc[i]) == 0 and not ci[i].any() and not cm[i].any() and not cc[i].any(), what
                        continue
                    assert int(nc[i]) == n == L, what
                    assert np.array_equal(ci[i], wci), what
                    assert np.array_equal(cm[i].view(np.uint64), wcm.view(np.uint64)), what
                    assert np.array_equal(cc[i], wcc), what
