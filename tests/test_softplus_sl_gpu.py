"""The list decoder's f after the integer work came out of its softplus halves (es_softplus_dev.h), on the device: the device form (the
one-instruction wrappers, exp table at LDS address 0) against the host's es_polar_f_fast_sp on the edge operands of
test_softplus_sl_edges.py, and the headline kernel (one lane per path, lists of 8, float32 LLRs) against the CPU oracle on one full block
of 8 frames and on 9 frames -- a second, partial block --, with an all-zero and a tie-heavy frame among them."""
import numpy as np
import pytest


@pytest.mark.gpu
def test_device_f_edge_operands_bits(engine, tmp_path):
    import torch
    from test_softplus_dev_gpu import _host_lib
    from test_softplus_sl_edges import edge_pairs
    rng = np.random.default_rng(711)
    a, b = edge_pairs(rng)
    llr = lambda k: np.clip(rng.normal(0, 6, k), -12, 12)
    a = np.ascontiguousarray(np.concatenate([a, llr(2048), rng.normal(0, 0.05, 2048)]))
    b = np.ascontiguousarray(np.concatenate([b, llr(2048), rng.normal(0, 0.05, 2048)]))
    want = np.empty((3, a.size)); want_bad = np.empty(a.size, np.int32)
    _host_lib(tmp_path).eval_pairs(a.ctypes.data, b.ctypes.data, a.size, want.ctypes.data, want_bad.ctypes.data)
    got, got_bad = engine.polar_f(torch.from_numpy(a).to(engine.device), torch.from_numpy(b).to(engine.device))
    torch.cuda.synchronize()
    got = got.cpu().numpy(); got_bad = got_bad.cpu().numpy()
    assert np.array_equal(got_bad, want_bad)
    assert 0 < want_bad.sum() < a.size
    ok = want_bad == 0
    for k in range(3):
        assert np.array_equal(got[k, ok].view(np.uint64), want[k, ok].view(np.uint64)), f"row {k} differs"


@pytest.fixture(scope="module")
def nine_frames(oracle):
    """nine frames of float32 LLRs and the oracle's lists of 8 for them: frame 3 all zero, frame 5 tie-heavy (every LLR +-12 or 0)"""
    rng = np.random.default_rng(712)
    llr = np.clip(rng.normal(0, 4, (9, 1024)), -12, 12).astype(np.float32)
    llr[3] = 0.0
    llr[5] = rng.choice(np.array([-12.0, 12.0, 0.0], np.float32), 1024)
    llr[8] = np.clip(llr[8] * 6, -12, 12)             # the lone frame of the second block: heavily clipped
    return llr, [oracle.scl_list(llr[i].astype(np.float64), 8) for i in range(9)]


@pytest.mark.gpu
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("B", [8, 9])
def test_headline_kernel_lists_equal_oracle(engine, nine_frames, B, skip):
    import torch
    llr, want = nine_frames
    x = torch.from_numpy(llr[:B]).to(engine.device)
    engine.set_option("scl_multi", 1); engine.set_option("scl_lanes", 1)       # es_scl_wide_kernel<64, 8>
    try:
        got = engine.scl(x, list_size=8, skip_if_hard_ok=skip)
        torch.cuda.synchronize()
    finally:
        engine.set_option("scl_multi", -1); engine.set_option("scl_lanes", 0)
    ncand, info, metric, ok = (t.cpu().numpy() for t in (got.ncand, got.cand_info, got.cand_metric, got.cand_ok))
    hard_ok = got.hard_ok.cpu().numpy()
    for i in range(B):
        if skip and hard_ok[i]:                        # settled by the hard decision: no list
            assert ncand[i] == 0
            continue
        nn, ci, cm, cc = want[i]
        assert int(ncand[i]) == nn, i
        assert np.array_equal(np.packbits(ci[:nn], axis=1), info[i, :nn]), i
        assert np.array_equal(cm[:nn].view(np.uint64), metric[i, :nn].view(np.uint64)), i
        assert np.array_equal(cc[:nn], ok[i, :nn]), i
