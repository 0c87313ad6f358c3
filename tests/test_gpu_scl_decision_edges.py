"""GPU: decisions inside the list decoders that the mutant audit of their table (tests/mutants.py SCL_MUTANTS) found no test
standing on.  As in test_gpu_decision_edges.py every input is built onto one comparison, the test first shows on the CPU, with the oracle,
that it sits there, and then compares every decoder with oracle.scl_list / oracle.polar_hard bit for bit: hard_info, hard_ok, ncand, the
candidate rows, the metrics' uint64 view, cand_ok.

  * the hard decision of a zero LLR (`__ballot(v > 0.0)` in es_scl.hip, es_scl_multi.hip, es_scl_wide.hip): code words with +-0.0 on
    positions that decide whether the CRC passes.  (The all-zero frame of the other tests cannot tell `>` from `>=`: the transform of
    the all-ones word has its only 1 on leaf 1023, a frozen position, so both readings give the same information bits.)
  * the three high-word thresholds of log1p inside the straight-line softplus, reached INSIDE the tree (es_softplus_neg_fast of es_math.h
    in es_scl.hip and es_scl_multi.hip, es_softplus_neg_sl_sh of es_softplus_dev.h in es_scl_wide.hip; the decoders inline these at
    different depths in different forms, which the helper kernels of test_device_softplus_bits / test_device_f_edge_operands_bits do not
    see): an operand t with a chosen high word of exp(t) or 1 + exp(t) is handed to the f of depth d of the first chain as a - b or
    a + b, for every depth 1 .. 10.

How an exact pair reaches depth d.  f(a, -C) = (a + log1p(e^-(a+C))) - log1p(e^-(C-a)) is `a` itself, bit for bit, once C >= 100 and
2^-80 < |a| < C - 38: both softplus terms are below half an ulp of a (and f(0, -C) is the difference of two equal terms, 0).  Likewise
f(-A, -C) = -A for 38 <= A <= C - 38.  So the half of the vector that level e discards is filled with -C_e (C_9 = 180, ..., C_1 = 484,
38 apart, all below 512: no operand leaves the range of the straight-line form on the way) and the kept half arrives unchanged.
At depth d the pair (x, y) sits on element 0 and every other element is f(-100, -140) = -100, so f(x, y) goes on unchanged (its
partner is -100 at every deeper level) and is leaf 0's LLR: the best path's metric is log1p(e^-|f(x, y)|) and the second's that plus
|f(x, y)|, every other leaf adding less than 1e-43.  One ulp of either softplus term of that one f is then one ulp-sized step of two
output metrics.  With x = t + m and y = -m (or +m), |t| / 2 <= m <= 2 |t|, both x and x + y (x - y) = t are exact.  The operands below were searched on the CPU, against a host build of
es_math.h with the threshold in question moved, for pairs at which the oracle's own lists change at every list size of this file.

All list sizes at which a decoder form exists are run: 1, 8, 33 (below its capacity of 64) and 128 (one frame per two-wave block), in
batches of 9 frames (at L = 8 one full wave of eight frames and a last wave with a lone frame), the three mappings for lists up to 32."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LISTS = (1, 8, 33, 128)
FORMS = ((0, 4), (1, 4), (1, 2), (1, 1))        # (scl_multi, scl_lanes): es_scl.hip, es_scl_multi.hip at 4 and 2 lanes per path, es_scl_wide.hip
B = 9
CONST = [None] + [180.0 + 38.0 * (9 - e) for e in range(1, 10)]      # C_1 = 484 ... C_9 = 180
FILL_A, FILL_B = 100.0, 140.0


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from echoseal_amd.engine import RxEngine
    e = RxEngine(0, list_size_max=128)
    yield e
    torch.cuda.synchronize()
    e.close()


def hi32(a):
    return (np.ascontiguousarray(a, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------- rows and comparison
def tree_row(d, x, y):
    """-> (the LLR row whose first chain hands (x, y) to element 0 of the f of depth d, the depth d-1 vector that must arrive)"""
    s = 1024 >> d
    t = np.empty(2 * s)
    t[:s] = -FILL_A; t[s:] = -FILL_B; t[0] = x; t[s] = y
    arrive = t.copy()
    for e in range(d - 1, 0, -1):
        t = np.concatenate([t, np.full(t.size, -CONST[e])])
    return t, arrive


def first_chain(oracle, row, d):
    """the vector of depth d-1 on the first chain, by the oracle's own f"""
    v = np.asarray(row, np.float64)
    for _ in range(1, d):
        h = v.size // 2
        v = oracle.polar_f_vec(v[:h], v[h:])
    return v


def decode(eng, x, L, skip):
    """every decoder form that exists at this list size -> [(form, result)]"""
    out = []
    for multi, lanes in (FORMS if L <= 32 else FORMS[-1:]):
        eng.set_option("scl_multi", multi); eng.set_option("scl_lanes", lanes)
        try:
            out.append(((multi, lanes), eng.scl(x, list_size=L, skip_if_hard_ok=skip).check()))
        finally:
            eng.set_option("scl_multi", -1); eng.set_option("scl_lanes", 0)
    torch.cuda.synchronize()
    return out


def same_as_oracle(res, want_hard, want_list, L, skip, tag):
    hinfo, hok, ncand, ci, cm, cc = (t.cpu().numpy() for t in (res.hard_info, res.hard_ok, res.ncand, res.cand_info, res.cand_metric, res.cand_ok))
    for i, ((winfo, wok), (nn, wi, wm, wc)) in enumerate(zip(want_hard, want_list)):
        where = tag + (i,)
        assert np.array_equal(np.packbits(winfo), hinfo[i]) and bool(hok[i]) == wok, where
        if skip and wok:                                   # settled by the hard decision: no list, zero rows
            assert ncand[i] == 0 and not ci[i].any() and not bits(cm[i]).any() and not cc[i].any(), where
            continue
        assert int(ncand[i]) == nn, where
        assert np.array_equal(np.packbits(wi[:nn], axis=1), ci[i, :nn]), where
        assert np.array_equal(bits(wm[:nn]), bits(cm[i, :nn])), (where, wm[:2], cm[i, :2])
        assert np.array_equal(wc[:nn], cc[i, :nn]), where


def run_rows(eng, oracle, rows, dtypes, skips, tag):
    """rows in batches of B through every form, list size, LLR type and skip setting, against the oracle (one reference per row and size)"""
    rows = np.ascontiguousarray(rows)
    for dt in dtypes:
        x64 = rows.astype(dt).astype(np.float64)
        hard = [oracle.polar_hard(r) for r in x64]
        for L in LISTS:
            lists = [oracle.scl_list(r, L) for r in x64]
            for lo in range(0, len(rows), B):
                x = torch.from_numpy(rows[lo:lo + B].astype(dt)).to(eng.device)
                for skip in skips:
                    for form, res in decode(eng, x, L, skip):
                        same_as_oracle(res, hard[lo:lo + B], lists[lo:lo + B], L, skip, (tag, np.dtype(dt).name, L, skip, form, lo))


# ------------------------------------------------------------------------------------------------------- hard decision of a zero LLR
def test_zero_llrs_decide_the_hard_crc(eng, oracle):
    """Nine frames: a clean code word at +-4; four in which 1, 2, 7 and 60 positions that carry a 1 are 0.0 (every second one -0.0), so
    that `v > 0.0` reads them as 0 and the CRC fails, while `v >= 0.0` would read the code word and pass; four in which as many
    positions that carry a 0 are zero, so that `>` passes and `>=` would fail.  float32 and float64, skip_if_hard_ok 0 and 1."""
    rng = np.random.default_rng(20261)
    rows, flips = [], []
    for k, ones in ((0, True), (1, True), (2, True), (7, True), (60, True), (1, False), (2, False), (7, False), (60, False)):
        code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
        v = (2.0 * code - 1.0) * 4.0
        pos = rng.choice(np.nonzero(code == (1.0 if ones else 0.0))[0], k, replace=False)
        v[pos] = np.where(np.arange(k) % 2 == 0, 0.0, -0.0)
        rows.append(v); flips.append((k, ones))
    rows = np.stack(rows)
    # the boundary, on the CPU: the verdict of the row, and of the row with its zeros made barely positive
    for v, (k, ones) in zip(rows, flips):
        info, ok = oracle.polar_hard(v)
        info_ge, ok_ge = oracle.polar_hard(np.where(v == 0.0, 1e-30, v))
        assert int((v == 0.0).sum()) == k and int(np.signbit(v[v == 0.0]).sum()) == k // 2
        assert (ok, ok_ge) == ((True, True) if k == 0 else (False, True) if ones else (True, False)), (k, ones, ok, ok_ge)
        assert k == 0 or not np.array_equal(info, info_ge)
    run_rows(eng, oracle, rows, (np.float32, np.float64), (False, True), "zeros")


# ------------------------------------------------------------------------------------------- log1p's thresholds inside the tree
# (depth, t and m of the pair whose SUM is t, t and m of the pair whose DIFFERENCE is t), as float.hex
K0 = (      # the high word of exp(t) is 0x3FDA827A: the first word on the k = 1 side of `hy < 0x3FDA827A`
    (1, "-0x1.c3435bd361c5cp-1", "0x1.132003e3705f6p+0", "-0x1.c343571cc1c5cp-1", "0x1.8965aee9e6342p-1"),
    (2, "-0x1.c3434b2361c5cp-1", "0x1.fe3a1a3a7a840p-2", "-0x1.c343505de1c5cp-1", "0x1.d0fae9bda108ep-1"),
    (3, "-0x1.c3435268e1c5cp-1", "0x1.7bade2d769218p+0", "-0x1.c343537301c5cp-1", "0x1.9b2f3683157d9p+0"),
    (4, "-0x1.c34355d121c5cp-1", "0x1.373c31cc2cdfap+0", "-0x1.c3435e2201c5cp-1", "0x1.a86f033218c3dp-1"),
    (5, "-0x1.c3434b2361c5cp-1", "0x1.e94736a678fb0p-1", "-0x1.c343537301c5cp-1", "0x1.054ae011a0955p+0"),
    (6, "-0x1.c34355d121c5cp-1", "0x1.587a02f643709p+0", "-0x1.c343505de1c5cp-1", "0x1.f368258c5c102p-1"),
    (7, "-0x1.c343564281c5cp-1", "0x1.7c1c408e97014p+0", "-0x1.c3435d1881c5cp-1", "0x1.293dfceac601bp+0"),
    (8, "-0x1.c343537301c5cp-1", "0x1.58f61b7abaec8p+0", "-0x1.c3434c9921c5cp-1", "0x1.cd384ba7ea66bp-1"),
    (9, "-0x1.c3434d8b81c5cp-1", "0x1.24448d2c87c78p+0", "-0x1.c3435a6b01c5cp-1", "0x1.fcf1b71668d8cp-1"),
    (10, "-0x1.c3435b59e1c5cp-1", "0x1.147b66dde6e40p+0", "-0x1.c3435bd361c5cp-1", "0x1.34c763b1f659ep+0"),
)
CORNER_FIRST = (      # the high word of 1 + exp(t) is 0x3FFFFFFD: the first word of fdlibm's |f| < 2^-20 corner
    (1, "-0x1.486e918236e19p-19", "0x1.10a217fcc1b9ep-18", "-0x1.1d620c627661ap-19", "0x1.99bdbc08fe889p-20"),
    (2, "-0x1.4ce54a74f6f09p-19", "0x1.0c78365af6a30p-19", "-0x1.1d620c627661ap-19", "0x1.89ef82c22702ep-19"),
    (3, "-0x1.5c043fab3725fp-19", "0x1.d5e7d3f67c768p-20", "-0x1.1d620c627661ap-19", "0x1.deb79cd622543p-19"),
    (4, "-0x1.4ce54a74f6f09p-19", "0x1.1cc3a0d7c1e10p-18", "-0x1.6e568c2e376d5p-19", "0x1.16678e4555222p-19"),
    (5, "-0x1.29c555c73685cp-19", "0x1.369c0dacb918dp-19", "-0x1.29c555c73685cp-19", "0x1.af13578353d33p-20"),
    (6, "-0x1.6e568c2e376d5p-19", "0x1.027c050bd89f8p-18", "-0x1.1d620c627661ap-19", "0x1.26de99097726ap-19"),
    (7, "-0x1.7e65af0277ae2p-19", "0x1.764b18441ed99p-19", "-0x1.3be43f73b6b9dp-19", "0x1.9e71aec2dc084p-20"),
    (8, "-0x1.1d620c627661ap-19", "0x1.b43905e5faa38p-19", "-0x1.29c555c73685cp-19", "0x1.3514fb6567cd6p-19"),
    (9, "-0x1.486e918236e19p-19", "0x1.f80b2be4efe5cp-19", "-0x1.0a48d51b36394p-19", "0x1.c8d3e1c79df5cp-19"),
    (10, "-0x1.0a48d51b36394p-19", "0x1.1b3348be73f4bp-19", "-0x1.1d620c627661ap-19", "0x1.8adaeabae7db1p-19"),
)
CORNER_LAST = (       # the high word of 1 + exp(t) is 0x3FFFFFFF: the last word of the corner below u == 2
    (1, "-0x1.232fb631d5f4bp-21", "0x1.36eaa4c43488cp-21", "-0x1.af142d9abc9e6p-26", "0x1.5ece50ea5cda2p-26"),
    (2, "-0x1.232fb631d5f4bp-21", "0x1.e17eb4331d34ap-22", "-0x1.af142d9abc9e6p-26", "0x1.61f68aa01a803p-25"),
    (3, "-0x1.af142d9abc9e6p-26", "0x1.f9a2e3363266ep-26", "-0x1.232fb631d5f4bp-21", "0x1.143c75904eae9p-21"),
    (4, "-0x1.af142d9abc9e6p-26", "0x1.f226c3ed5cd30p-26", "-0x1.232fb631d5f4bp-21", "0x1.909cccf2d1e22p-21"),
    (5, "-0x1.af142d9abc9e6p-26", "0x1.d3b565180a765p-26", "-0x1.6ebc133eaf282p-24", "0x1.1afac0b7fc8c1p-23"),
    (6, "-0x1.af142d9abc9e6p-26", "0x1.43172b9171d43p-25", "-0x1.af142d9abc9e6p-26", "0x1.7678474df1728p-25"),
    (7, "-0x1.af142d9abc9e6p-26", "0x1.092d564befab6p-25", "-0x1.af142d9abc9e6p-26", "0x1.771bd7e0559b2p-25"),
    (8, "-0x1.6ebc133eaf282p-24", "0x1.bfe45d3932295p-25", "-0x1.af142d9abc9e6p-26", "0x1.562bc37fc7bcdp-26"),
    (9, "-0x1.af142d9abc9e6p-26", "0x1.156fb6cbcfe36p-25", "-0x1.6ebc133eaf282p-24", "0x1.e32c9a2412ec8p-24"),
    (10, "-0x1.af142d9abc9e6p-26", "0x1.0d67e6d446563p-25", "-0x1.232fb631d5f4bp-21", "0x1.d35f64b090e46p-21"),
)


def threshold_rows(oracle, table, on_boundary):
    """The 20 rows of a table (sum and difference at every depth), each shown on the CPU to deliver its operand -> (rows, t, x, y)"""
    rows, ts, xs, ys = [], [], [], []
    for d, t_sum, m_sum, t_diff, m_diff in table:
        for t, m, sign in ((float.fromhex(t_sum), float.fromhex(m_sum), -1.0), (float.fromhex(t_diff), float.fromhex(m_diff), 1.0)):
            assert t < 0.0 and abs(t) / 2 <= m <= 2 * abs(t)
            x, y = t + m, sign * m
            assert (x + y if sign < 0 else x - y) == t                         # the operand of one of f's two softplus terms, exactly
            assert on_boundary(t), (d, t.hex())
            row, arrive = tree_row(d, x, y)
            assert np.abs(row).max() < 512.0
            assert np.array_equal(bits(first_chain(oracle, row, d)), bits(arrive)), d      # (x, y) reach the f of depth d ...
            v = first_chain(oracle, row, 11)                                    # ... and f(x, y) is leaf 0's LLR
            assert bits(v)[0] == bits(oracle.polar_f_vec([x], [y]))[0] and (v[0] == 0.0 or 2.0 ** -80 < abs(v[0]) < 8.0)
            rows.append(row); ts.append(t); xs.append(x); ys.append(y)
    return np.stack(rows), np.array(ts), np.array(xs), np.array(ys)


def helpers_equal_oracle(eng, oracle, t, x, y):
    """the same operands through the two helper kernels: the softplus of es_math.h and the f of es_softplus_dev.h, on the device"""
    want = oracle.log1p_vec(oracle.exp_vec(t))
    got = eng.softplus(torch.from_numpy(t).to(eng.device)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    f, bad = eng.polar_f(torch.from_numpy(x).to(eng.device), torch.from_numpy(y).to(eng.device))
    torch.cuda.synchronize()
    f = f.cpu().numpy()
    assert not bad.cpu().numpy().any()
    assert np.array_equal(bits(f[0]), bits(oracle.polar_f_vec(x, y)))
    assert np.array_equal(bits(f[1]), bits(oracle.log1p_vec(oracle.exp_vec(-np.abs(x - y)))))
    assert np.array_equal(bits(f[2]), bits(oracle.log1p_vec(oracle.exp_vec(-np.abs(x + y)))))


def test_log1p_k_boundary_inside_the_tree(eng, oracle):
    """`hy < 0x3FDA827A` (k = 0 against k = 1 in log1p): exp(t) with the high word 0x3FDA827A itself, |t| in a window of 5.8e-7 around
    0.8813730 that 200 000 uniform draws from (0.85, 0.92) hit 1.6 times.  At every t below the two forms of log1p give different
    doubles (searched on the CPU), so the line one word further is one ulp of f and a changed metric."""
    rows, t, x, y = threshold_rows(oracle, K0, lambda t: hi32(oracle.exp_vec([t]))[0] == 0x3FDA827A)
    run_rows(eng, oracle, rows, (np.float64,), (False,), "k0")
    helpers_equal_oracle(eng, oracle, t, x, y)


def test_log1p_corner_first_word_inside_the_tree(eng, oracle):
    """`hu0 > 0x3FFFFFFC` / `(hu0 - 0x3FFFFFFD) < 3`: 1 + exp(t) with the high word 0x3FFFFFFD, the first of the corner's three.  Of its
    2^33 operands 46 give another double outside the corner (enumerated on the CPU); each t below is one whose exp(t) is one of them."""
    rows, t, x, y = threshold_rows(oracle, CORNER_FIRST, lambda t: hi32(1.0 + oracle.exp_vec([t]))[0] == 0x3FFFFFFD)
    run_rows(eng, oracle, rows, (np.float64,), (False,), "corner, first word")
    helpers_equal_oracle(eng, oracle, t, x, y)


def test_log1p_corner_last_word_inside_the_tree(eng, oracle):
    """The same for the corner's last high word, 0x3FFFFFFF (`< 3u`): three of its 2^33 operands give another double outside the corner,
    exp(t) = 0x1.fffffd2287db9p-1, 0x1.ffffedcd04efbp-1 and 0x1.ffffff2875e96p-1; every t below is one of them."""
    rows, t, x, y = threshold_rows(oracle, CORNER_LAST, lambda t: hi32(1.0 + oracle.exp_vec([t]))[0] == 0x3FFFFFFF)
    assert set(float(v).hex() for v in oracle.exp_vec(t)) <= {"0x1.fffffd2287db9p-1", "0x1.ffffedcd04efbp-1", "0x1.ffffff2875e96p-1"}
    run_rows(eng, oracle, rows, (np.float64,), (False,), "corner, last word")
    helpers_equal_oracle(eng, oracle, t, x, y)
