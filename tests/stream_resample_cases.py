"""The streams of tests/test_gpu_monitor_rates.py, a NumPy restatement of es_resample_stream_kernel / es_resample_commit_kernel, and the
code path each tile of those streams takes, without a GPU.

A push that takes a stream from n_old to n_old + len samples finalizes outputs F(n_old) .. F(n_old + len) - 1; the kernel cuts them into
tiles of TILE.  A tile reads its input window from LDS when span <= WIN_MAX and from its two sources (tail row, chunk) otherwise, and its
polyphase table from LDS when up * hpp <= FILT_MAX and through L2 otherwise: the four arms of rs_tile.  tiles() restates rs_tile's own
formulas with the stream kernel's first output, y0 + F(n_old) + k0."""
import math

import numpy as np

from echoseal_amd.utils import finalized, stream_resample_plan

TILE = 1024                                                                    # ES_RESAMPLE_TILE
WIN_MAX, FILT_MAX = 4352, 3584                                                 # RS_WIN_MAX, RS_FILT_MAX of es_resample.hip
TAIL = 256                                                                     # ES_RSTREAM_TAIL
ARMS = ("window LDS, table LDS", "window LDS, table global", "window global, table LDS", "window global, table global")
ALL_ARMS = {(arm, k) for arm in ARMS for k in ("k0 == 0", "k0 > 0")}

# the ten pairs and the cut points the prefix property was checked at
FACT_PAIRS = [(44_100, 48_000), (8_000, 48_000), (16_000, 48_000), (22_050, 48_000), (11_025, 48_000), (32_000, 48_000), (96_000, 48_000),
              (192_000, 48_000), (47_999, 48_000), (48_000, 44_100)]
FACT_CUTS = sorted(set(list(range(1, 4)) + [20, 21, 22, 1023, 1024, 1025] + [5, 7, 10, 15, 30, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 160, 161,
                                                                            255, 256, 257, 300, 441, 500, 511, 512, 513, 777]))
assert len(FACT_CUTS) == 36

# (fs_in, fs_target) of the GPU test's streams, by the arm their full tiles take
GPU_PAIRS = {(44_100, 48_000): ARMS[0], (8_000, 48_000): ARMS[0], (384_000, 48_000): ARMS[2], (47_999, 48_000): ARMS[1], (192_000, 44_100): ARMS[3]}
EXACT_COUNTS = (TILE - 1, TILE, TILE + 1)
REST_OUTPUTS = 2 * TILE + 50                                                   # the last chunk: two full tiles and a short one


def reduced(fs_in: int, fs_target: int):
    g = math.gcd(fs_in, fs_target)
    return fs_target // g, fs_in // g


def _reachable(n_old: int, count: int, pl):
    """The chunk length after n_old samples that finalizes exactly `count` outputs, or None where F steps over F(n_old) + count."""
    f0 = finalized(n_old, pl.up, pl.down, pl.y0)
    ln = max(0, (count * pl.down) // pl.up - 2)
    while finalized(n_old + ln, pl.up, pl.down, pl.y0) - f0 < count:
        ln += 1
    return ln if finalized(n_old + ln, pl.up, pl.down, pl.y0) - f0 == count else None


def chunk_finalizing(n_old: int, count: int, pl):
    """-> (phase, length): after `phase` more samples (a chunk of its own, as few as possible) a chunk of `length` samples finalizes exactly
    `count` outputs.  Where the rate falls every count is reached at once (phase 0).  A pair that raises the rate steps over counts -- F
    grows by up to ceil(up / down) per sample -- and the phase moves the start to where the count is met; only where up / down is a whole
    number above 1 (8 -> 48 kHz: F grows in sixes) can no phase help, and the next count above is taken."""
    for phase in range(pl.up + 1):
        ln = _reachable(n_old + phase, count, pl)
        if ln is not None:
            return phase, ln
    assert pl.up % pl.down == 0 and pl.up > pl.down
    ln = 0
    while finalized(n_old + ln, pl.up, pl.down, pl.y0) - finalized(n_old, pl.up, pl.down, pl.y0) < count:
        ln += 1
    return 0, ln


def gpu_plan(fs_in: int, fs_target: int) -> list:
    """[(chunk length, outputs it is meant to finalize or None)] of one GPU-test stream: 1, 1, hpp - 2, hpp - 1, hpp and 0 samples, then
    chunks that finalize 1 023, 1 024 and 1 025 outputs (each after a phase chunk of a few samples where the pair needs one), then one
    that finalizes REST_OUTPUTS."""
    pl = stream_resample_plan(fs_in, fs_target)
    plan = [(c, None) for c in (1, 1, pl.hpp - 2, pl.hpp - 1, pl.hpp, 0)]
    for c in EXACT_COUNTS + (REST_OUTPUTS,):
        phase, ln = chunk_finalizing(sum(l for l, _ in plan), c, pl)
        if phase:
            plan.append((phase, None))
        plan.append((ln, c))
    return plan


def gpu_cuts(fs_in: int, fs_target: int) -> list:
    """The chunk lengths of gpu_plan."""
    return [ln for ln, _ in gpu_plan(fs_in, fs_target)]


def tiles(n_old: int, length: int, pl, out_stride=None):
    """[(k0, cnt, span, up * hpp, arm)] of one push, by the kernel's formulas."""
    up, down, hpp, y0 = pl.up, pl.down, pl.hpp, pl.y0
    f_old = finalized(n_old, up, down, y0)
    n_out = finalized(n_old + length, up, down, y0) - f_old
    if out_stride is not None:
        n_out = min(n_out, out_stride)
    out = []
    for k0 in range(0, n_out, TILE):
        cnt = min(n_out - k0, TILE)
        yy = y0 + f_old + k0
        t0 = ((yy % up) * down) % up
        span = ((cnt - 1) * down + t0) // up + hpp
        x_lds, h_lds = span <= WIN_MAX, up * hpp <= FILT_MAX
        out.append((k0, cnt, span, up * hpp, ARMS[(0 if x_lds else 2) + (0 if h_lds else 1)]))
    return out


def coverage(streams):
    """{(arm, 'k0 == 0' | 'k0 > 0'): tiles} over [(fs_in, fs_target, cuts)]."""
    seen: dict = {}
    for fs_in, fs_target, cuts in streams:
        pl, n = stream_resample_plan(fs_in, fs_target), 0
        for ln in cuts:
            for k0, _, _, _, arm in tiles(n, ln, pl):
                key = (arm, "k0 == 0" if k0 == 0 else "k0 > 0")
                seen[key] = seen.get(key, 0) + 1
            n += ln
    return seen


# ---- the kernels in NumPy ---------------------------------------------------------------------------------------------------------------
def fresh_state():
    return np.zeros(TAIL, np.float32), 0


def stream_step(pl, tail: np.ndarray, n_old: int, chunk: np.ndarray):
    """One record of es_resample_stream_kernel + es_resample_commit_kernel: -> (outputs float32, new tail, n_new).  Input index a < n_old
    is read from the tail row, tail[255 - (n_old - 1 - a)], a >= n_old from the chunk; indices before sample 0 are skipped; one output is
    rs_dot: accumulator from +0, products in ascending input index, multiply and add rounded separately in float32."""
    x = chunk.astype(np.float32) / np.float32(32768) if chunk.dtype == np.int16 else chunk.astype(np.float32)
    up, down, hpp, y0 = pl.up, pl.down, pl.hpp, pl.y0
    n_new = n_old + x.size
    h = pl.h_tf.reshape(up, hpp)
    out = []
    for k in range(finalized(n_old, up, down, y0), finalized(n_new, up, down, y0)):
        yy = y0 + k
        t, x_idx = (yy * down) % up, (yy * down) // up
        assert n_old <= x_idx < n_new                                          # final now, and not before
        lo = max(x_idx - hpp + 1, 0)
        assert n_old - lo <= TAIL - 1                                          # the tail row's 255 samples reach every tap
        idx = np.arange(lo, x_idx + 1)
        win = np.where(idx < n_old, tail[np.clip(TAIL - 1 - (n_old - 1 - idx), 0, TAIL - 1)], x[np.clip(idx - n_old, 0, max(x.size - 1, 0))] if x.size else 0)
        taps = h[t, hpp - idx.size:]                                           # tap m pairs with input index x_idx - hpp + 1 + m
        prod = (win.astype(np.float32) * taps).astype(np.float32)
        out.append(np.cumsum(np.concatenate((np.zeros(1, np.float32), prod)), dtype=np.float32)[-1])
    both = np.concatenate((tail, x))
    return np.asarray(out, np.float32), both[-TAIL:].copy(), n_new
