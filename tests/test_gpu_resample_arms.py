"""GPU: every code path of the two resampling kernels against scipy.signal.resample_poly, bit for bit -- no tolerance anywhere.

1. es_resample_ragged_kernel (es_resample_ragged_batch): a tile reads its input window from LDS or, above RS_WIN_MAX samples, from global
   memory, and its polyphase table from LDS or, above RS_FILT_MAX values, from global memory.  One launch per sample type and rep runs
   all four arms at full tiles, each with k0 == 0 and k0 > 0 (tests/resample_arms.py proves which tile takes which arm from the
   descriptors, by the kernel's own formulas), records that end in a full tile and in a short one, the records on both sides of either
   threshold and a record whose products are subnormal.  A second launch gives 47 999 -> 48 000 Hz enough tiles for (yy mod up) * down
   to pass 2^31.  Scaffolding as in test_gpu_resample_ragged.py: poisoned pool, clips GAP samples apart, a sentinel behind every row.
2. es_resample_kernel (RxEngine.resample, what a single clip's conditioning runs): more outputs than the grid has lanes, inputs around
   and below the taps per phase at rising and falling rates, float64 and int16 batches.
3. verify_batch with clips at 384 kHz for a 48 kHz detector and at 192 kHz for a 44.1 kHz detector (the window-global arms) against a
   fresh detector on the clip conditioned on the host: results and traces."""
import math

import numpy as np
import pytest
from scipy.signal import resample_poly

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import resample_arms as A
from echoseal_amd import _native as nat
from echoseal_amd.detector import WatermarkDetector
from echoseal_amd.embedder import TxParams, WatermarkEmbedder, synthetic_payloads
from echoseal_amd.utils import resample_plan, resample_to

TILE = A.TILE
SENTINEL = -7.25
DTYPES = {np.int16: nat.ES_DTYPE_I16, np.float32: nat.ES_DTYPE_F32, np.float64: nat.ES_DTYPE_F64}
KEY = b"\xAA" * 32
LIST = 8


def _samples(rng, n, dtype):
    x = rng.standard_normal(n) * 0.3
    if dtype == np.int16:
        return np.clip(np.round(x * 32768), -32768, 32767).astype(np.int16)
    return x.astype(dtype)


def _reference(x, fs_in, fs_out):
    src = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
    g = math.gcd(fs_in, fs_out)
    return resample_poly(src, fs_out // g, fs_in // g).astype(np.float32)


def _pool(clips, desc, dtype):
    """The flat sample pool: the clips at their descriptors' offsets, everything between them poisoned."""
    poison = np.int16(32767) if dtype == np.int16 else dtype(np.nan)
    pool = np.full(int(desc[-1, 0]) + clips[-1].size + A.GAP, poison, dtype)
    if dtype != np.int16:
        pool[::2] = np.inf
    for o, c in zip(desc[:, 0].tolist(), clips):
        pool[o:o + c.size] = c
    return pool


_PLANS: dict = {}
_CASES: dict = {}


def _plan(recs, dtype):
    """Descriptors and filter pool; int16 and float32 records share theirs (one compute type, the same integers)."""
    key = (tuple(recs), np.dtype(np.float64 if dtype == np.float64 else np.float32))
    if key not in _PLANS:
        _PLANS[key] = A.descriptors(recs, key[1])
    return _PLANS[key]


def _case(dtype, which="arms"):
    """Clips, descriptor table, filter pool, sample pool and SciPy's outputs of one launch -- made once per sample type."""
    if (dtype, which) not in _CASES:
        rng = np.random.default_rng(4711)
        if which == "arms":
            recs = A.records()
        else:                                                               # 45 full tiles and a short one: yy reaches 46 000
            recs = [(A.n_in_for(45 * TILE + 7, 47_999, 48_000), 47_999, 48_000)]
        clips = [_samples(rng, n, dtype) for n, _, _ in recs]
        if which == "arms" and dtype != np.int16:
            clips[-1] = A.small_products_clip(dtype, recs[-1][0], rng)
        desc, filters = _plan(recs, dtype)
        refs = [_reference(c, fi, fo) for c, (_, fi, fo) in zip(clips, recs)]
        assert [r.size for r in refs] == desc[:, 7].tolist() and [c.size for c in clips] == desc[:, 1].tolist()
        _CASES[dtype, which] = (recs, clips, desc, filters, _pool(clips, desc, dtype), refs)
    return _CASES[dtype, which]


def _launch(engine, dtype, desc, filters, pool, rep, longest):
    d = engine.device
    stride = (longest + 3) // 4 * 4 + 8
    out = torch.full((desc.shape[0] * rep, stride), SENTINEL, dtype=torch.float32, device=d)
    pd, fd, dd = torch.from_numpy(pool).to(d), torch.from_numpy(filters).to(d), torch.from_numpy(desc).to(d)
    # every read stays inside the two pools: the kernel clamps to them, and the descriptors lie inside to begin with
    assert (desc[:, 0] >= 0).all() and (desc[:, 0] + desc[:, 1] <= pool.size).all() and (desc[:, 4] + desc[:, 2] * desc[:, 5] <= filters.size).all()
    rc = engine._lib.es_resample_ragged_batch(engine._ctx, pd.data_ptr(), DTYPES[dtype], pd.numel(), fd.data_ptr(), fd.numel(), dd.data_ptr(),
                                              desc.shape[0], rep, out.data_ptr(), stride, longest, torch.cuda.current_stream(d).cuda_stream)
    assert rc == 0, engine._lib.es_last_error(engine._ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_rows(got, refs, recs, desc, rep, what):
    bad = []
    for r, ref in enumerate(refs):
        for c in range(rep):
            row = got[r * rep + c]
            same = row[:ref.size].view(np.uint32) == ref.view(np.uint32)
            if not same.all():
                k = int(np.flatnonzero(~same)[0])
                arm = next(t[4] for t in A.tiles(desc[r]) if t[0] <= k < t[0] + t[1])
                bad.append((what, recs[r], "row", c, "first output", k, arm, float(row[k]), float(ref[k]), int((~same).sum())))
            assert (row[ref.size:] == np.float32(SENTINEL)).all(), (what, recs[r], c, "the sentinel behind the record")
    assert not bad, bad[:8]


# ----------------------------------------------------------------------------------------------- 1. the ragged kernel, arm by arm
@pytest.mark.parametrize("rep", [1, 4])
@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_every_arm_at_full_tiles_equals_scipy_bit_for_bit(engine, dtype, rep):
    recs, clips, desc, filters, pool, refs = _case(dtype)
    longest = max(r.size for r in refs)
    seen = A.coverage(desc, (longest + 3) // 4 * 4 + 8)
    print("tiles per arm:", sorted(seen.items()))
    assert set(seen) == A.ALL_ARMS, sorted(A.ALL_ARMS - set(seen))            # all four arms, each with k0 == 0 and with k0 > 0
    if dtype != np.int16:                                                   # the last record: subnormal products, both signs of zero
        tiny, x = np.finfo(dtype).tiny, clips[-1]
        h = filters[desc[-1, 4]:desc[-1, 4] + desc[-1, 2] * desc[-1, 5]]
        assert np.abs(x).max() * np.abs(h).max() < tiny and (np.signbit(x) & (x == 0)).any() and (~np.signbit(x) & (x == 0)).any()
        assert refs[-1].any() or dtype == np.float64                         # (float64 sums of such products round to float32 zeros ...
        assert np.signbit(refs[-1]).any() and not np.signbit(refs[-1]).all()  # ... of either sign)
    got = _launch(engine, dtype, desc, filters, pool, rep, longest)
    _check_rows(got, refs, recs, desc, rep, np.dtype(dtype).name)


@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_tile_start_beyond_32_bits_equals_scipy(engine, dtype):
    """47 999 -> 48 000 Hz (up 48 000, down 47 999) over 46 tiles: (yy mod up) * down of a tile's first output passes 2^31 from yy = 44 742
    on; the kernel forms it in 64 bits."""
    recs, clips, desc, filters, pool, refs = _case(dtype, "long")
    _, _, up, down, _, _, y0, n_out = desc[0].tolist()
    starts = [((y0 + k0) % up) * down for k0 in range(0, n_out, TILE)]
    assert sum(s >= 1 << 31 for s in starts) >= 2 and len(starts) == 46
    assert {t[4] for t in A.tiles(desc[0])} == {"window LDS, table global"}
    got = _launch(engine, dtype, desc, filters, pool, 1, n_out)
    _check_rows(got, refs, recs, desc, 1, np.dtype(dtype).name)


# ----------------------------------------------------------------------------------------------- 2. one lane per output
PAIRS_1 = [(44_100, 48_000), (48_000, 44_100), (192_000, 44_100), (384_000, 48_000)]


def _same(got, ref):
    return got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got.view(np.uint8), ref.view(np.uint8))


def test_resample_grid_stride_wraps(engine):
    """More outputs than the launch has lanes (the grid is capped at 32 blocks of 256 lanes per CU): every lane takes a second output."""
    cap = torch.cuda.get_device_properties(engine.device).multi_processor_count * 32 * 256
    B, up, down = 3, 6, 1                                                   # 8 000 -> 48 000 Hz
    n = (cap + cap // 16) // (B * up) + 1
    assert B * n * up > cap + cap // 16                                     # the launch exceeds its lanes, with a margin
    x = (np.random.default_rng(8).standard_normal((B, n)) * 0.3).astype(np.float32)
    got = engine.resample(x, 8_000, 48_000).cpu().numpy()
    assert got.shape == (B, n * up) and got.size > cap
    for r in range(B):
        assert _same(got[r], resample_poly(x[r], up, down)), r


@pytest.mark.parametrize("fs_in,fs_out", PAIRS_1)
def test_resample_short_inputs_equal_scipy(engine, fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    hpp = resample_plan(64, fs_out, fs_in, np.float32)[1]
    rng = np.random.default_rng(fs_in + fs_out)
    for dtype in (np.float32, np.float64, np.int16):
        for n in (1, 2, hpp - 1, hpp, hpp + 1):
            x = _samples(rng, n, dtype)
            assert _same(engine.resample(x, fs_in, fs_out).cpu().numpy(), resample_poly(x, up, down)), (np.dtype(dtype).name, n)


@pytest.mark.parametrize("dtype", [np.float64, np.int16])
def test_resample_batches_of_other_sample_types_equal_scipy(engine, dtype):
    rng = np.random.default_rng(31)
    for fs_in, fs_out in PAIRS_1:
        g = math.gcd(fs_in, fs_out)
        xb = np.stack([_samples(rng, 3001, dtype) for _ in range(4)])
        got = engine.resample(xb, fs_in, fs_out).cpu().numpy()
        for r in range(4):
            assert _same(got[r], resample_poly(xb[r], fs_out // g, fs_in // g)), (fs_in, fs_out, r)


# ----------------------------------------------------------------------------------------------- 3. end to end at the new rates
# No clip of this project verifies True end to end without a patched demodulator (tests/test_gpu_ragged.py plants its true positive that
# way), so "still verifies" is taken as "verify still tries frames": of the lengths 1 215 ... 3 000 tried at both target rates, 2 000 samples
# is the shortest at which the marked and the unmarked clip, conditioned from the high rate, each still reach the decoder (at 1 500 the
# 44.1 kHz marked clip has header decodes and no try).
CLIP_LEN = 2000


def _marked(fs: int, n: int, seed: int):
    """(marked, unmarked) float32 clips of n samples at fs: a noise carrier, and the same carrier with frames of counters 0, 1, ... under KEY
    mixed in as WatermarkEmbedder.process mixes them -- payloads from a seeded generator, so the clip is the same in every run."""
    tx = WatermarkEmbedder(KEY, TxParams(fs=fs))
    ctrs = list(range(-(-n // 1215)))
    tx._chip_buf = tx.make_frames(ctrs, synthetic_payloads(tx.sec, ctrs)).reshape(-1)
    carrier = (np.random.default_rng(seed).standard_normal(n) * 0.05).astype(np.float32)
    return tx.process(carrier).astype(np.float32), carrier


def _host_conditioned(x, f, fs_target):
    return np.asarray(resample_to(fs_target, x, f)[0]).astype(np.float32)


def _traced(det):
    det._trace = []; det._hdr_trace = []
    return det


@pytest.mark.parametrize("fs_in,fs_target", [(384_000, 48_000), (192_000, 44_100)])
def test_verify_batch_at_window_global_rates_equals_host_conditioning(engine, fs_in, fs_target):
    from echoseal_amd.engine import RxEngine
    eng = engine if fs_target == 48_000 else RxEngine(0, list_size_max=LIST, fs=fs_target)
    g = math.gcd(fs_in, fs_target)
    marked, plain = _marked(fs_target, CLIP_LEN, fs_target)
    queue = [(resample_poly(c.astype(np.float64), fs_in // g, fs_target // g).astype(np.float32), fs_in) for c in (marked, plain)]
    queue.append((marked[:1700].copy(), fs_target))                          # and a clip at the target rate in the same batch
    plan = eng.condition_upload([x.size for x, _ in queue], [f for _, f in queue], fs_target, np.float32).plan
    arms = {t[4] for row in plan.desc for t in A.tiles(row)}
    assert ("window global, table LDS" if fs_target == 48_000 else "window global, table global") in arms
    want, trace, hdr, tries = [], [], [], []
    for x, f in queue:
        det = _traced(WatermarkDetector(KEY, fs_target=fs_target, list_size=LIST, engine=eng))
        want.append(det.verify(_host_conditioned(x, f, fs_target), fs_target))
        trace += det._trace; hdr += det._hdr_trace; tries.append(len(det._trace))
    det = _traced(WatermarkDetector(KEY, fs_target=fs_target, list_size=LIST, engine=eng))
    got = det.verify_batch([x for x, _ in queue], [f for _, f in queue])
    print("tries per clip:", tries, "header decodes:", len(hdr))
    assert got == want and det._trace == trace and det._hdr_trace == hdr
    assert min(tries[:2]) > 0 and len(hdr) >= len(trace) > 5                 # both conditioned clips reached the decoder
    if eng is not engine:
        eng.close()
