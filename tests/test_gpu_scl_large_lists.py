"""Lists of 257..1024 paths on the GPU (es_scl_wide_large.hip: the lane-per-path kernel at 512 and 1024 lanes per block), bit for bit
against the CPU oracle, through every layer: es_scl_batch, RxEngine.scl, PolarCode / polar_fast.decode and WatermarkDetector.

  * every new list size, float32 and float64 LLRs, both skip modes;
  * launches of more blocks than the scratch slab has slots (slots are reused), every record checked;
  * run-time K (the GK instantiations);
  * two streams of one context with launches of different block sizes interleaved (the slab guard's shape tag);
  * the public API, the limit (1024) and the refusals above it."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KEY = b"\xAA" * 32
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SIZES = (257, 300, 384, 511, 512, 513, 700, 1000, 1023, 1024)


@pytest.fixture(scope="module")
def big():
    from echoseal_amd.engine import RxEngine
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    eng = RxEngine(0, list_size_max=1024)
    yield eng
    torch.cuda.synchronize()
    eng.close()


def _rows(oracle, n_noise: int, seed: int) -> np.ndarray:
    """An all-zero row (x[0] = 1e-3), a constant-magnitude +-4 row (ties everywhere), a clean code word with a few flips at +-12,
    and N(0, 3) rows clipped to +-12."""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(1024)]
    rows[0][0] = 1e-3
    rows.append(np.where(rng.integers(0, 2, 1024) > 0, 4.0, -4.0))
    code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
    clean = np.where(code > 0, 12.0, -12.0)
    flip = clean.copy()
    flip[rng.choice(1024, 6, replace=False)] *= -1.0
    rows += [clean, flip]
    rows += list(np.clip(rng.normal(0, 3, (n_noise, 1024)), -12, 12))
    return np.stack(rows)


def _check_against_oracle(oracle, x: np.ndarray, res, L: int, what) -> None:
    """Every record of `res` (a launch with skip_if_hard_ok = 0) equals the oracle's list (compared in worker threads)."""
    ci_all = res.cand_info.cpu().numpy(); cm_all = res.cand_metric.cpu().numpy(); cc_all = res.cand_ok.cpu().numpy()
    nc_all = res.ncand.cpu().numpy(); hi_all = res.hard_info.cpu().numpy(); ho_all = res.hard_ok.cpu().numpy()

    def work(lo, hi):
        bad = []
        for i in range(lo, hi):
            xi = x[i].astype(np.float64)
            hinfo, hok = oracle.polar_hard(xi)
            if np.packbits(hinfo).tobytes() != hi_all[i].tobytes() or hok != bool(ho_all[i]):
                bad.append((i, "hard"))
            nn, ci, cm, cc = oracle.scl_list(xi, L)
            if int(nc_all[i]) != L or nn != L:
                bad.append((i, "ncand", int(nc_all[i]), nn))
            elif not np.array_equal(np.packbits(ci, axis=1), ci_all[i]):
                bad.append((i, "cand_info"))
            elif not np.array_equal(cm.view(np.uint64), cm_all[i].view(np.uint64)):
                bad.append((i, "cand_metric"))
            elif not np.array_equal(cc, cc_all[i]):
                bad.append((i, "cand_ok"))
        return bad
    bad = oracle.map_records(work, x.shape[0], chunk=1 if x.shape[0] < 64 else 8)
    assert not bad, (what, L, bad[:8])


def test_every_new_size_equals_oracle(big, oracle):
    x = _rows(oracle, 8, 1)                                       # 12 rows
    for L in SIZES:
        for dt in (np.float32, np.float64):
            xd = x.astype(dt)
            res = big.scl(torch.from_numpy(xd).to(big.device), list_size=L, skip_if_hard_ok=False).check()
            assert res.cand_metric.shape == (x.shape[0], L)
            _check_against_oracle(oracle, xd, res, L, dt.__name__)


def test_skip_if_hard_ok_at_new_sizes(big, oracle):
    """Rows whose hard decision passes skip the list (ncand = 0, rows of zeros); the others equal the oracle's list."""
    x = _rows(oracle, 5, 2)
    rng = np.random.default_rng(3)
    code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
    x = np.concatenate([x, np.where(code > 0, 5.0, -5.0)[None], np.where(code > 0, 0.5, -0.5)[None]])
    for L in (300, 512, 1000):
        res = big.scl(torch.from_numpy(x).to(big.device), list_size=L, skip_if_hard_ok=True).check()
        n_hard = 0
        for i in range(x.shape[0]):
            hinfo, hok = oracle.polar_hard(x[i])
            assert np.packbits(hinfo).tobytes() == res.hard_info[i].cpu().numpy().tobytes() and hok == bool(res.hard_ok[i]), (L, i)
            if hok:
                n_hard += 1
                assert int(res.ncand[i]) == 0 and not res.cand_info[i].any() and not res.cand_metric[i].any() and not res.cand_ok[i].any(), (L, i)
            else:
                nn, ci, cm, cc = oracle.scl_list(x[i], L)
                assert int(res.ncand[i]) == L
                assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy()), (L, i)
                assert np.array_equal(cm.view(np.uint64), res.cand_metric[i].cpu().numpy().view(np.uint64)), (L, i)
                assert np.array_equal(cc, res.cand_ok[i].cpu().numpy()), (L, i)
        assert n_hard >= 3 and n_hard < x.shape[0]


def test_more_blocks_than_slab_slots(big, oracle):
    """One block per CU is resident at 512 and 1024 paths: a launch of 2 x that + 37 records reuses every slab slot, every
    record equals the oracle (ncand never -1)."""
    n_cu = torch.cuda.get_device_properties(big.device).multi_processor_count
    B = 2 * n_cu + 37
    rng = np.random.default_rng(11)
    x = np.clip(rng.normal(0, 3, (B, 1024)), -12, 12).astype(np.float32)
    for L in (512, 1024):
        res = big.scl(torch.from_numpy(x).to(big.device), list_size=L, skip_if_hard_ok=False).check()
        _check_against_oracle(oracle, x, res, L, "B = %d" % B)


@pytest.mark.parametrize("K", [200, 1000])
def test_run_time_k_at_512(oracle, K):
    from echoseal_amd.engine import RxEngine
    eng = RxEngine(0, list_size_max=512, code_k=K)
    try:
        rng = np.random.default_rng(40 + K)
        x = np.clip(rng.normal(0, 3, (6, 1024)), -12, 12)
        x[0] = 0.0; x[0, 0] = 1e-3
        with oracle.code_k(K):
            code = oracle.polar_encode(rng.integers(0, 2, K - 8, dtype=np.uint8)).astype(np.float64)
            x[1] = np.where(code > 0, 3.0, -3.0); x[1, rng.choice(1024, 5, replace=False)] *= -1.0
            for L, dt in ((512, np.float32), (400, np.float64)):
                xd = x.astype(dt)
                res = eng.scl(torch.from_numpy(xd).to(eng.device), list_size=L, skip_if_hard_ok=False).check()
                assert res.cand_info.shape[-1] == (K - 8 + 7) // 8
                for i in range(x.shape[0]):
                    hinfo, hok = oracle.polar_hard(xd[i].astype(np.float64))
                    assert np.packbits(hinfo).tobytes() == res.hard_info[i].cpu().numpy().tobytes() and hok == bool(res.hard_ok[i]), (K, L, i)
                    nn, ci, cm, cc = oracle.scl_list(xd[i].astype(np.float64), L)
                    assert int(res.ncand[i]) == nn == L, (K, L, i)
                    assert np.array_equal(np.packbits(ci, axis=1), res.cand_info[i].cpu().numpy()), (K, L, i)
                    assert np.array_equal(cm.view(np.uint64), res.cand_metric[i].cpu().numpy().view(np.uint64)), (K, L, i)
                    assert np.array_equal(cc, res.cand_ok[i].cpu().numpy()), (K, L, i)
    finally:
        torch.cuda.synchronize()
        eng.close()


def test_two_streams_interleave_block_sizes(big):
    """Launches of 256-, 512- and 64-lane blocks on two streams of one context: each result equals its own run alone.  (Block
    sizes cut the slab into slots of different strides: launches of different sizes must not share it concurrently.)"""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(np.clip(rng.normal(0, 3, (1024, 1024)), -12, 12).astype(np.float32)).to(big.device)
    plan = [(256, x[:768]), (512, x[:300]), (64, x[:1024]), (512, x[300:700]), (256, x[500:1000]), (64, x[100:400])]
    alone = [big.scl(xs, list_size=L, skip_if_hard_ok=False) for L, xs in plan]
    torch.cuda.synchronize()
    s = [torch.cuda.Stream(big.device), torch.cuda.Stream(big.device)]
    torch.cuda.current_stream(big.device).synchronize()
    both = []
    for k, (L, xs) in enumerate(plan):
        with torch.cuda.stream(s[k % 2]):
            both.append(big.scl(xs, list_size=L, skip_if_hard_ok=False))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(alone, both)):
        a.check(); b.check()
        for name in ("hard_info", "hard_ok", "ncand", "cand_info", "cand_ok"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (k, name)
        assert torch.equal(a.cand_metric.view(torch.int64), b.cand_metric.view(torch.int64)), k


def test_public_api_large_lists(oracle):
    from echoseal_amd import polar_fast
    from echoseal_amd.fastpolar import PolarCode
    rng = np.random.default_rng(21)
    code = oracle.polar_encode(rng.integers(0, 2, 440, dtype=np.uint8)).astype(np.float64)
    llr = np.clip(2.0 * (2.0 * code - 1.0 + rng.normal(0, 1.0, 1024)) / 1.0, -12, 12)
    noise = np.clip(rng.normal(0, 3, 1024), -12, 12).astype(np.float32)
    for x, L in ((llr, 600), (noise, 600), (llr.astype(np.float32), 1000)):
        info, ok, _ = oracle.polar_decode(x.astype(np.float64), L)
        bits, pok = PolarCode(1024, 448, list_size=L, crc_size=8).decode(x)
        assert pok == ok and np.array_equal(bits, info), L
        payload, fok = polar_fast.decode(x, list_size=L, return_ok=True)
        assert fok == ok and payload == np.packbits(info).tobytes(), L


def test_detector_at_512_follows_reference_search(big):
    """The quick-test frame at list size 512: the same result (its LLRs are about half wrong, SURVEY section 0.2, so no list
    rescues it: True would be a finding) and the same scan (band, peak, counter) trace -- the search does not depend on L.
    The detector picks its engine up by itself (the large-list engine)."""
    from echoseal_amd.detector import WatermarkDetector
    g = np.load(os.path.join(GOLD, "quick32.npz"))
    det = WatermarkDetector(KEY, list_size=512)
    det._trace = []
    assert det.verify_raw_frame(g["frame"]) == bool(g["result"])
    assert det.engine.list_size_max >= 512
    assert np.array_equal(np.array(det._trace, dtype=np.int64).reshape(-1, 3), g["scan_trace"])


def test_detector_true_positive_at_512(big, oracle):
    """A sealed code word with four weakly held wrong signs, through _try_decode_frame at L = 512 (only the demodulator patched, as
    test_detector.py's L = 8 positive): the hard decision fails, the list finds the blob (checked on the oracle first), so the
    detector returns True for its counter and False for another."""
    from echoseal_amd.detector import FRAME_LEN, WatermarkDetector
    from echoseal_amd.polar_fast import encode
    det = WatermarkDetector(KEY, list_size=512, engine=big)
    blob = det.sec.seal(b"ESAL" + (3).to_bytes(4, "big") + b"\x07" * 8 + bytes(11))
    llr = (2.0 * encode(blob).astype(np.float64) - 1.0) * 6.0
    flips = np.random.default_rng(0).choice(1024, 4, replace=False)
    llr[flips] = -np.sign(llr[flips]) * 0.5
    llr = llr.astype(np.float32)
    assert oracle.polar_hard(llr.astype(np.float64))[1] is False
    _n, ci, _cm, cc = oracle.scl_list(llr.astype(np.float64), 512)
    assert np.packbits(ci, axis=1)[np.flatnonzero(cc)[0]].tobytes() == blob     # the first CRC-passing candidate is the blob
    dev = torch.from_numpy(llr).to(big.device).reshape(1, 1024)
    calls = []
    real_llr, real_scl = big.llr, big.scl
    try:
        big.llr = lambda *a, **k: dev.expand(a[0].shape[0], 1024).contiguous()
        big.scl = lambda *a, **k: (calls.append(k.get("list_size")), real_scl(*a, **k))[1]
        assert det._try_decode_frame(np.zeros(FRAME_LEN), 3) is True and det.session_nonce == b"\x07" * 8
        assert det._try_decode_frame(np.zeros(FRAME_LEN), 4) is False          # counter mismatch -> validator rejects
    finally:
        big.llr, big.scl = real_llr, real_scl
    assert calls == [512, 512]


def test_limit_is_1024(big):
    import echoseal_amd._native as nat
    from echoseal_amd import polar_fast
    from echoseal_amd.detector import WatermarkDetector
    from echoseal_amd.engine import RxEngine
    from echoseal_amd.fastpolar import PolarCode
    assert nat.ES_MAX_LIST == 1024 and big.list_size_max == 1024
    x = np.zeros(1024)
    with pytest.raises(NotImplementedError, match="1024"):
        PolarCode(1024, 448, list_size=1025, crc_size=8).decode(x)
    with pytest.raises(NotImplementedError, match="1024"):
        polar_fast.decode(x, list_size=1025)
    with pytest.raises(NotImplementedError, match="1024"):
        WatermarkDetector(KEY, list_size=1025).engine
    with pytest.raises(nat.NativeError, match=r"\[0, 1024\]"):
        RxEngine(0, list_size_max=1025)
    with pytest.raises(nat.NativeError, match="list_size"):
        big.scl(torch.zeros((1, 1024), device=big.device), list_size=1025)
