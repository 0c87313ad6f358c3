"""GPU: the verdict memo alone -- es_memo_probe_batch / es_memo_insert_batch through RxEngine.open_memo / memo_probe / memo_insert,
held byte for byte to the host twin (echoseal_amd.memo.MemoModel) on records that contest most slots."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from echoseal_amd import memo as M

EINVAL = -1


def _u64(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint64)


def _claim(mem):
    return mem.claim.detach().cpu().numpy().view(np.uint32)


def _records(seed):
    """300 records with fields from tiny ranges (512 distinct records at most: exact duplicates are certain), every seventh masked."""
    rng = np.random.default_rng(seed)
    k0, k1 = M.pack(rng.integers(0, 4, 300), rng.integers(0, 4, 300), rng.integers(0, 2, 300), rng.integers(0, 8, 300), rng.integers(0, 2, 300))
    k0[::7] = M.EMPTY
    k0[5], k1[5] = k0[4], k1[4]                                             # neighbours that are one record
    return k0, k1


@pytest.mark.parametrize("slots", [64, 1])
def test_three_inserts_with_probes_between_equal_the_twin(engine, slots):
    k0, k1 = _records(slots)
    assert len({(int(a), int(b)) for a, b in zip(k0, k1)}) < 280 and (k0 == M.EMPTY).sum() >= 42
    mem, twin = engine.open_memo(slots), M.MemoModel(slots)
    assert mem.table.shape == (slots, 2) and (_u64(mem.table) == M.EMPTY).all() and (_claim(mem) == 0xFFFFFFFF).all()
    live = k0 != M.EMPTY
    assert not engine.memo_probe(mem, k0[live], k1[live]).any()             # an empty table holds nothing
    contested = 0
    for call in range(3):
        sel = slice(100 * call, 100 * call + 100)
        wrote = twin.insert(k0[sel], k1[sel])
        contested += int((k0[sel] != M.EMPTY).sum() - wrote.sum())
        engine.memo_insert(mem, k0[sel], k1[sel])
        assert np.array_equal(_u64(mem.table), twin.table), call
        assert (_claim(mem) == 0xFFFFFFFF).all(), call
        hit = engine.memo_probe(mem, k0, k1).cpu().numpy().astype(bool)
        assert np.array_equal(hit, twin.probe(k0, k1)), call
        assert hit[sel][wrote].all()                                        # what a call wrote is found right after it
        assert np.array_equal(_u64(mem.table), twin.table), call            # (a probe writes nothing)
    assert contested > 60                                                   # records that lost their slot to a lower index of their call
    if slots == 64:
        assert (twin.table[:, 0] != M.EMPTY).sum() > 48                     # most slots were contested and are taken
    # device tensors are taken as they are (int64 words), and give the same answers
    d = lambda a: torch.from_numpy(a.view(np.int64).copy()).to(engine.device)
    assert np.array_equal(engine.memo_probe(mem, d(k0), d(k1)).cpu().numpy().astype(bool), twin.probe(k0, k1))


def test_zero_records_write_nothing(engine):
    mem = engine.open_memo(64)
    k0, k1 = _records(3)
    engine.memo_insert(mem, k0[:50], k1[:50])
    before = (_u64(mem.table).copy(), _claim(mem).copy())
    engine.memo_insert(mem, k0[:0], k1[:0])
    assert engine.memo_probe(mem, k0[:0], k1[:0]).shape == (0,)
    lib, ctx, st = engine._lib, engine._ctx, engine._stream()
    assert lib.es_memo_insert_batch(ctx, None, None, 64, None, None, 0, st) == 0      # n == 0: nothing is looked at
    assert lib.es_memo_probe_batch(ctx, None, 64, None, None, 0, None, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_u64(mem.table), before[0]) and np.array_equal(_claim(mem), before[1])


def test_refusals_leave_table_and_claim_unchanged(engine):
    mem = engine.open_memo(64)
    k0, k1 = _records(4)
    engine.memo_insert(mem, k0[:50], k1[:50])
    d = lambda a: torch.from_numpy(a.view(np.int64).copy()).to(engine.device)
    a, b = d(k0[50:60]), d(k1[50:60])
    hit = torch.full((10,), 7, dtype=torch.uint8, device=engine.device)
    before = (_u64(mem.table).copy(), _claim(mem).copy())
    lib, ctx, st = engine._lib, engine._ctx, engine._stream()
    p = lambda t: t.data_ptr()
    T, C, A, B, H = p(mem.table), p(mem.claim), p(a), p(b), p(hit)
    ins = lambda table=T, claim=C, slots=64, k0=A, k1=B, n=10: lib.es_memo_insert_batch(ctx, table, claim, slots, k0, k1, n, st)
    prb = lambda table=T, slots=64, k0=A, k1=B, n=10, hit=H: lib.es_memo_probe_batch(ctx, table, slots, k0, k1, n, hit, st)
    bad = {"slots 0": dict(slots=0), "slots negative": dict(slots=-64), "slots 3": dict(slots=3), "slots 48": dict(slots=48),
           "slots 2^40 + 1": dict(slots=(1 << 40) + 1), "n negative": dict(n=-1), "n 2^32 - 1": dict(n=2 ** 32 - 1), "n 2^32": dict(n=2 ** 32),
           "n 2^40": dict(n=1 << 40), "null table": dict(table=None), "null k0": dict(k0=None), "null k1": dict(k1=None)}
    for what, kw in bad.items():
        assert ins(**kw) == EINVAL, what
        assert prb(**kw) == EINVAL, what
    assert ins(claim=None) == EINVAL and prb(hit=None) == EINVAL
    torch.cuda.synchronize()
    assert np.array_equal(_u64(mem.table), before[0]) and np.array_equal(_claim(mem), before[1])
    assert (hit.cpu().numpy() == 7).all()
    assert ins() == 0 and prb() == 0                                        # the valid call the arguments describe goes through
    torch.cuda.synchronize()
    twin = M.MemoModel(64)
    twin.insert(k0[:50], k1[:50]); twin.insert(k0[50:60], k1[50:60])
    assert np.array_equal(_u64(mem.table), twin.table) and (_claim(mem) == 0xFFFFFFFF).all()
    assert np.array_equal(hit.cpu().numpy().astype(bool), twin.probe(k0[50:60], k1[50:60]))
    with pytest.raises(ValueError, match="power of two"):
        engine.open_memo(48)
