"""GPU: the capped launches of the level mix, the live monitor and the sync kernels, each past its grid cap (tests/grid_caps.py).

As in test_gpu_grid_stride.py every comparison is of bytes and there are two checks: the large launch against the same entry point on
slices below the cap (every row), and against host code or the oracle (every row where cheap, else grid_caps.index_set).
  * the three es_mix_*_block_kernel forms at block = 1: a workgroup per sample, so past(2048 * cu) / 2 samples per row suffice; the
    host check is a vectorised NumPy restatement of WatermarkEmbedder.process for one-sample blocks, tied to the block-by-block
    host_mix of test_gpu_embed.py on a 2 000-sample prefix that holds every loudness kind, a NaN and an inf;
  * a monitor tick of 16 * cu + 4 streams: the stream correlation strides past its cap and the in-place picker four times;
  * the float64 correlation and picker, their ragged forms and the float32 screen with the exact picker on past(cap) rows of 104
    samples (42 lags)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import grid_caps as G
from echoseal_amd.tables import pack_tables
from test_embed_mix import host_embedder, host_process
from test_gpu_embed import audio, chip_stream, host_mix
from test_gpu_grid_stride import KEYS, dev, same_rows, sliced

FL = 1215
M32 = 1 << 32
KINDS = ["silence", "tiny", "quiet", "mid", "loud", "clip"]
PREFIX = 2000


# ------------------------------------------------------------------------------------------------------------------------- mix
def mix_audio(rng, n, r=0):
    """n samples that run through the loudness kinds of test_gpu_embed.audio in stretches of 250 (so a prefix of 1 500 holds them all),
    with a NaN and an inf inside the first 2 000 samples and more of both further out."""
    x = np.concatenate([audio(rng, min(250, n - s), KINDS[(s // 250 + r) % 6]) for s in range(0, n, 250)])
    x[100 + r] = np.nan; x[400 + r] = np.inf; x[1999] = -np.inf
    far = rng.integers(PREFIX, n, 40)
    x[far[:20]] = np.nan; x[far[20:30]] = np.inf; x[far[30:]] = -np.inf
    return x


def process_block1(x, chips, alpha_db=-10.0, floor_db=-35.0):
    """WatermarkEmbedder.process (echoseal_amd/embedder.py:53-68) for successive blocks of ONE sample, all blocks at once: x, chips
    float32 [n] -> (out float32 [n], scale float64 [n]).  Line by line: the mean of one square is the square; np.float32 + EPS stays
    float32; Python's max(a, b) is b only if b > a and min(a, b) is b only if b < a (a NaN first argument stays); array * Python
    float multiplies in float32."""
    from echoseal_amd.embedder import EPS, MIX_HEADROOM
    from echoseal_amd.utils import db_to_lin
    with np.errstate(all="ignore"):
        in_rms = (np.sqrt(x * x) + np.float32(EPS)).astype(np.float64)
        a = db_to_lin(alpha_db) * in_rms
        scale = np.where(db_to_lin(floor_db) > a, db_to_lin(floor_db), a)
        head = MIX_HEADROOM - np.abs(x).astype(np.float64)
        head = np.where(0.0 > head, 0.0, head)
        peak = np.abs(chips).astype(np.float64) + EPS
        q = head / peak
        scale = np.where(peak > 0.0, np.where(q < scale, q, scale), 0.0)
        return x + chips * scale.astype(np.float32), scale


def tie_to_host_mix(x, chips):
    """The restatement equals process() block by block on the prefix, which holds every loudness kind, a NaN and both infinities."""
    p = slice(0, PREFIX)
    assert np.isnan(x[p]).any() and np.isposinf(x[p]).any() and np.isneginf(x[p]).any()
    amp = np.abs(np.nan_to_num(x[p], nan=0.0, posinf=0.0, neginf=0.0))
    assert (amp == 0).any() and ((amp > 0) & (amp < 1e-20)).any() and (amp > 0.98).any() and ((amp > 0.05) & (amp < 0.98)).any()
    want, wscale = host_mix(x[p], chips[p], 1)
    got, gscale = process_block1(x[p], chips[p])
    assert got.tobytes() == want.tobytes() and np.array_equal(gscale, wscale, equal_nan=True)


def same_scales(got, want, what):
    """Gains bit for bit, except that any NaN equals any NaN: its payload is not part of process()'s result."""
    bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want)))
    assert not bad.size, (what, bad.size, bad[:8].tolist())


def test_mix_block_kernel_past_the_cap(engine):
    t = G.trip(engine.device)
    R, n = 2, G.past(t["mix_block"]) // 2 + 1
    assert R * n > t["mix_block"] >= n
    rng = np.random.default_rng(201)
    x = np.stack([mix_audio(rng, n, r) for r in range(R)])
    off = np.array([0, 5], np.int64)
    chips = np.stack([chip_stream(rng, n + 5) for _ in range(R)])
    xd, cd = dev(engine, x), dev(engine, chips)
    out, scale = engine.mix(xd, cd, block=1, chip_off=dev(engine, off), want_scale=True)
    out, scale = out.cpu().numpy(), scale.cpu().numpy()
    for r in range(R):
        o1, s1 = engine.mix(xd[r:r + 1], cd[r:r + 1], block=1, chip_off=dev(engine, off[r:r + 1]), want_scale=True)
        same_rows(out[r], o1[0].cpu().numpy(), f"row {r} vs the row mixed alone")
        same_rows(scale[r], s1[0].cpu().numpy(), f"gains of row {r} vs the row mixed alone")
        c = chips[r, off[r]: off[r] + n]
        tie_to_host_mix(x[r], c)
        want, wscale = process_block1(x[r], c)
        same_rows(out[r], want, f"row {r} vs process()")
        same_scales(scale[r], wscale, f"gains of row {r} vs process()")


def test_ragged_mix_block_kernel_past_the_cap(engine):
    """Three records of unequal length in rows of past(cap) / 3 samples, the longest last: its blocks are the second trip's."""
    t = G.trip(engine.device)
    R = 3
    stride = G.past(t["mix_block"]) // R + 1
    lens = np.array([stride // 2 + 1, stride - 4099, stride], np.int64)
    assert R * stride > t["mix_block"] and 2 * stride + lens[2] > t["mix_block"] + 1000
    rng = np.random.default_rng(202)
    x = np.full((R, stride), np.nan, np.float32)                             # the padding may hold anything
    gap = [3, 5, 0]
    base = np.cumsum([0] + [lens[r] + gap[r] for r in range(R - 1)]).astype(np.int64) + 1
    pool = chip_stream(rng, int(base[-1] + lens[-1]) + 2)
    for r in range(R):
        x[r, :lens[r]] = mix_audio(rng, int(lens[r]), r)
    xd, pd = dev(engine, x), dev(engine, pool)
    sentinel = np.float32(-777.25)
    out = torch.full_like(xd, float(sentinel))
    got, scale = engine.mix_ragged(xd, lens, pd, base, lens, block=1, want_scale=True, out=out)
    got, scale = got.cpu().numpy(), scale.cpu().numpy()
    for r in range(R):
        m = int(lens[r])
        c = pool[base[r]: base[r] + m]
        o1, s1 = engine.mix(xd[r:r + 1, :m], dev(engine, c[None]), block=1, chip_off=torch.zeros(1, dtype=torch.int64), want_scale=True)
        same_rows(got[r, :m], o1[0].cpu().numpy(), f"record {r} vs mix")
        same_rows(scale[r, :m], s1[0].cpu().numpy(), f"gains of record {r} vs mix")
        assert (got[r, m:] == sentinel).all(), r                             # nothing is written past the record
        tie_to_host_mix(x[r, :m], c)
        want, wscale = process_block1(x[r, :m], c)
        same_rows(got[r, :m], want, f"record {r} vs process()")
        same_scales(scale[r, :m], wscale, f"gains of record {r} vs process()")


def test_stream_mix_block_kernel_past_the_cap(engine):
    """embed_step at block = 1 on two streams of different keys that stand inside a frame (off != 0): audio against the
    embed(carry=) chain of each stream and against the host embedder's chips under process(); the table's ctr / off / tail after the
    tick against the chain's, so that the commit is checked too."""
    t = G.trip(engine.device)
    n = G.past(t["mix_block"]) // 2 + 1
    assert 2 * n > t["mix_block"]
    rng = np.random.default_rng(203)
    first, ctr0 = [700, 1300], [65_530, M32 - 3]
    table = engine.open_streams(KEYS[:2], [0, 1], ctr0=ctr0)
    nf0 = [-(-f // FL) for f in first]
    nf1 = [-(-(f % FL + n) // FL) - 1 for f in first]
    pay = [rng.integers(0, 256, (a + b, 55), dtype=np.uint8) for a, b in zip(nf0, nf1)]
    head = [audio(rng, f, "mid") for f in first]
    body = [mix_audio(rng, n, s) for s in range(2)]
    engine.embed_step(table, [0, 1], head, payloads=[p[:a] for p, a in zip(pay, nf0)])
    assert table.off.cpu().numpy().tolist() == [f % FL for f in first] and all(table.off_host > 0)
    res = engine.embed_step(table, [0, 1], body, block=1, payloads=[p[a:] for p, a in zip(pay, nf0)], want_scale=True)
    for s in range(2):
        prev = engine.embed(KEYS[s], head[s], ctr0=ctr0[s], payloads=dev(engine, pay[s][None, :nf0[s]]))
        one = engine.embed(KEYS[s], body[s], ctr0=prev.ctr, carry=prev, block=1, payloads=dev(engine, pay[s][None, nf0[s]:]), want_scale=True)
        got = res[s].audio.cpu().numpy()
        same_rows(got, one.audio.cpu().numpy(), f"stream {s} vs embed(carry=)")
        same_rows(res[s].scale.cpu().numpy(), one.scale[0].cpu().numpy(), f"gains of stream {s} vs embed(carry=)")
        assert (res[s].ctr, res[s].off) == (int(one.ctr[0]), int(one.off[0])), s
        assert int(table.ctr[s]) == int(one.ctr[0]) and int(table.off[s]) == int(one.off[0]), s
        same_rows(table.tail[s].cpu().numpy(), one.tail[0].cpu().numpy(), f"tail of stream {s}")
        # the host embedder: its pending chips after the first chunk, then the frames of the next counters
        tx = host_embedder(KEYS[s], ctr0[s], pay[s])
        host_process(tx, head[s], 1024)
        ctrs = [(tx.frame_ctr + k) % M32 for k in range(nf1[s])]
        chips = np.concatenate((tx._chip_buf, tx.make_frames(ctrs, pay[s][nf0[s]:]).reshape(-1)))
        assert int(table.ctr[s]) == (tx.frame_ctr + nf1[s]) % M32 and (FL - int(table.off[s])) % FL == chips.size - n
        tie_to_host_mix(body[s], chips[:n])
        want, wscale = process_block1(body[s], chips[:n])
        same_rows(got, want, f"stream {s} vs process()")
        same_scales(res[s].scale.cpu().numpy(), wscale, f"gains of stream {s} vs process()")
        same_rows(table.tail[s].cpu().numpy(), chips[-FL:], f"tail of stream {s} vs the host embedder's last frame")


# ------------------------------------------------------------------------------------------------------------- sync, 42 lags
T_ROW = 104


def sync_rows(rng, B, T=T_ROW):
    """B rows of T samples: noise over three decades of level, every other row with a preamble 1000 times as strong at a random lag
    (a peak above the threshold; the other rows take the picker's fallback); bands 0 .. 3."""
    from scipy.signal import lfilter
    from echoseal_amd.utils import mseq_63
    level = 10.0 ** rng.uniform(-4, -1, (B, 1))
    x = (rng.standard_normal((B, T)) * level).astype(np.float32)
    band = (np.arange(B) % 4).astype(np.uint8)
    ba = pack_tables()[0]
    pre = [lfilter(ba[b, :9], ba[b, 9:], 2.0 * mseq_63().astype(np.float64) - 1.0) for b in range(4)]     # as the transmitter shapes it
    for i in range(0, B, 2):
        o = int(rng.integers(0, T - 62))
        x[i, o:o + 63] += (pre[band[i]] * (1000.0 * level[i, 0])).astype(np.float32)
    return x, band


def oracle_rows(oracle, idx, y_of, band, thr, peaks, npeaks, corr_of=None):
    """Rows idx against the oracle: y_of(i) float64 samples of row i -> ncc, threshold, peaks; corr_of(i) the device's lags, if any."""
    tpl = pack_tables()[1]
    kinds = set()
    for i in idx.tolist():
        c = oracle.ncc(y_of(i), tpl[band[i]])
        if corr_of is not None:
            assert c.tobytes() == corr_of(i).tobytes(), ("corr", i)
        th, _, _ = oracle.cfar_threshold(c)
        pk, tot, fb = oracle.pick_peaks(c, th)
        word = int(npeaks[i])
        k = word & 0xFFFF
        assert np.float64(th).tobytes() == thr[i].tobytes() and k == tot and bool((word >> 30) & 1) == fb, ("thr / npeaks", i, th, float(thr[i]), word, tot, fb)
        assert peaks[i, :min(k, 32)].tolist() == pk[:min(k, 32)].tolist() and (peaks[i, min(k, 32):] == -1).all(), ("peaks", i)
        kinds.add(fb)
    return kinds


def test_float64_sync_past_the_cap(engine, oracle):
    """es_xcorr_kernel (a wave per row here, 16 * cu blocks of four) and es_pick_kernel (a row per block, 16 * cu blocks)."""
    t = G.trip(engine.device)
    B = G.past(t["xcorr_segments"])
    x, band = sync_rows(np.random.default_rng(204), B)
    bd = dev(engine, band)
    y = engine.bpf(dev(engine, x), bd)
    corr = engine.xcorr(y, bd)
    got = [a.cpu().numpy() for a in (corr,) + engine.pick(corr)]

    def part(s):
        c = engine.xcorr(y[s].contiguous(), bd[s])
        return (c,) + engine.pick(c)
    for g, w, what in zip(got, sliced(part, B, t["pick_rows"]), ("corr", "thr", "peaks", "npeaks")):
        same_rows(g, w, f"{what} vs its slices")
    yh = y.cpu().numpy()
    idx = G.index_set(B, [t["pick_rows"], t["xcorr_segments"]], seed=4)
    kinds = oracle_rows(oracle, idx, lambda i: yh[i], band, got[1], got[2], got[3], corr_of=lambda i: got[0][i])
    assert kinds == {False, True}                                           # rows with peaks above the threshold, and fallback rows


def test_ragged_sync_past_the_cap(engine, oracle):
    """es_xcorr_ragged_kernel and es_pick_ragged_kernel through sync_ragged: lengths 63 .. 104 and a few below the template."""
    t = G.trip(engine.device)
    B = G.past(t["xcorr_segments"])
    rng = np.random.default_rng(205)
    x, band = sync_rows(rng, B)
    lens = rng.integers(63, T_ROW + 1, B).astype(np.int32)
    lens[::97] = rng.integers(0, 63, lens[::97].size)
    lens[[0, B - 1, t["pick_rows"], t["xcorr_segments"]]] = T_ROW
    x[np.arange(T_ROW)[None, :] >= lens[:, None]] = np.nan                  # the padding may hold anything
    xd, bd, ld = dev(engine, x), dev(engine, band), dev(engine, lens)
    valid_y = torch.arange(T_ROW, device=engine.device)[None, :] < ld[:, None]
    valid_c = torch.arange(T_ROW - 62, device=engine.device)[None, :] < (ld[:, None] - 62)

    def run(s):
        sy = engine.sync_ragged(xd[s], ld[s], bd[s], keep_corr=True)
        return torch.where(valid_y[s], sy.y, 0.0), torch.where(valid_c[s], sy.corr, 0.0), sy.thr, sy.peaks, sy.npeaks
    got = [a.cpu().numpy() for a in run(slice(0, B))]
    for g, w, what in zip(got, sliced(run, B, t["pick_rows"]), ("y", "corr", "thr", "peaks", "npeaks")):
        same_rows(g, w, f"{what} vs its slices")
    short = lens < 63
    assert short.sum() > 100 and not got[4][short].any() and not got[2][short].any() and (got[3][short] == -1).all()
    idx = G.index_set(B, [t["pick_rows"], t["xcorr_segments"]], seed=5)
    idx = idx[~short[idx]]
    oracle_rows(oracle, idx, lambda i: got[0][i, :lens[i]], band, got[2], got[3], got[4], corr_of=lambda i: got[1][i, :lens[i] - 62])


def test_two_kernel_sync_past_the_cap(engine, oracle):
    """es_xcorr32_batch + es_pick_exact_batch: the float32 screen (a wave per row, 16 * cu blocks of four) and the exact picker (a row
    per wave, 16 * cu blocks of four)."""
    t = G.trip(engine.device)
    assert t["pick_exact_rows"] == t["xcorr_segments"]
    B = G.past(t["pick_exact_rows"])
    x, band = sync_rows(np.random.default_rng(206), B)
    bd = dev(engine, band)
    y, y32 = engine.bpf2(dev(engine, x), bd)

    def run(s):
        c32 = engine.xcorr32(y32[s].contiguous(), bd[s])
        return (c32,) + engine.pick_exact(c32, y[s].contiguous(), bd[s])
    got = [a.cpu().numpy() for a in run(slice(0, B))]
    # two halves: below one trip, and above the num_cu * 8 rows under which es_xcorr32_batch runs its small-batch kernel, whose screen
    # may differ from this one's in the last ulps (es_sync32.hip: energy summation order)
    half = -(-B // 2)
    assert t["cu"] * 8 <= B - half <= half <= t["pick_exact_rows"]
    for g, w, what in zip(got, sliced(run, B, half), ("corr32", "thr", "peaks", "npeaks", "flags")):
        same_rows(g, w, f"{what} vs its slices")
    yh = y.cpu().numpy()
    idx = G.index_set(B, [t["pick_exact_rows"]], seed=6)
    assert oracle_rows(oracle, idx, lambda i: yh[i], band, got[1], got[2], got[3]) == {False, True}


# ------------------------------------------------------------------------------------------------------------- live monitor
def test_live_monitor_many_streams(engine, oracle):
    """16 * cu + 4 streams, float32 and int16 mixed, the smallest window, ticks of 70 and 34 samples: es_xcorr_stream_kernel has
    4 S / 4 blocks, above its cap, and es_pick_at_kernel 4 S rows, four times its cap.  y_hist and corr_hist as
    test_every_launched_bandpass_form asserts them; the second tick's thr / peaks / npeaks of every row against xcorr + pick in slices
    of at most 16 * cu rows, and against the oracle on the index set."""
    from echoseal_amd.monitor import MIN_WINDOW
    from test_gpu_monitor import _band4, _u64, _whole
    t = G.trip(engine.device)
    S, n = t["xcorr_blocks"] + 4, T_ROW
    rng = np.random.default_rng(207)
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) if s % 3 else rng.integers(-3000, 3000, n).astype(np.int16) for s in range(S)]
    ref = np.zeros((4 * S, n), np.uint64)
    for grp in ([s for s in range(S) if s % 3], [s for s in range(S) if s % 3 == 0]):
        assert len(grp) <= t["xcorr_blocks"]
        y, _ = _whole(engine, [xs[s] for s in grp])
        ref[(4 * np.array(grp)[:, None] + np.arange(4)).reshape(-1)] = _u64(y)
    yd = dev(engine, ref.view(np.float64))
    band = _band4(engine, S)
    assert 4 * S > 4 * t["pick_rows"] and 4 * S > t["xcorr_segments"]

    def part(s):
        c = engine.xcorr(yd[s].contiguous(), band[s])
        return (c,) + engine.pick(c)
    corr, thr, peaks, npeaks = sliced(part, 4 * S, t["pick_rows"])
    table = engine.open_monitor(S, window=MIN_WINDOW, chunk_max=70)
    at = 0
    for ln in (70, 34):
        tick = engine.monitor_step(table, np.arange(S), [x[at: at + ln] for x in xs])
        at += ln
        assert np.array_equal(_u64(table.y_hist[:, :at]), ref[:, :at]), ln
    assert np.array_equal(_u64(table.corr_hist[:, : n - 62]), corr.view(np.uint64))
    got = [a.cpu().numpy() for a in (tick.thr, tick.peaks, tick.npeaks)]
    for g, w, what in zip(got, (thr, peaks, npeaks), ("thr", "peaks", "npeaks")):
        same_rows(g, w, f"{what} of the second tick vs xcorr + pick in slices")
    yh = ref.view(np.float64)
    idx = G.index_set(4 * S, [t["pick_rows"], t["xcorr_segments"]], seed=7)
    oracle_rows(oracle, idx, lambda i: yh[i], np.tile(np.arange(4, dtype=np.uint8), S), *got)
