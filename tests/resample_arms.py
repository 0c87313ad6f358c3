"""The records of tests/test_gpu_resample_arms.py and the code path each of their tiles takes in es_resample_ragged_kernel, without a GPU.

A tile of TILE outputs reads its input window from LDS when span <= WIN_MAX and from global memory otherwise, and its polyphase table from
LDS when up * hpp <= FILT_MAX and from global memory otherwise: four arms (the four rs_dot calls of the kernel).  tiles() restates the
kernel's own formulas for (span, up * hpp) of every tile of a descriptor, so the GPU test can prove which arms its launch runs and the
CPU suite can prove it without a GPU (tests/test_condition_host.py, which also holds the three numbers below to es_resample.hip)."""
import math

import numpy as np

from echoseal_amd.utils import condition_plan, resample_plan, resampled_length

TILE = 1024                                                                    # ES_RESAMPLE_TILE (checked against the header by the CPU suite)
WIN_MAX, FILT_MAX, RATE_MAX = 4352, 3584, 1 << 20                              # RS_WIN_MAX, RS_FILT_MAX, RS_RATE_MAX of es_resample.hip
ARMS = ("window LDS, table LDS", "window LDS, table global", "window global, table LDS", "window global, table global")
GAP = 5                                                                        # poisoned samples before, between and after the clips

# (fs_in, fs_out) by the arm their FULL tiles take
PAIRS = [(384_000, 48_000), (352_800, 48_000),                                 # window global, table LDS: up 1 (t0 always 0) and up 20
         (192_000, 44_100), (200_000, 44_100),                                 # both global: up 147 / hpp 92 and up 441 / hpp 96
         (11_025, 48_000), (22_050, 48_000), (44_056, 48_000), (47_999, 48_000),      # window LDS, table global: up 640, 320, 6 000, 48 000
         (192_000, 48_000), (176_400, 48_000)]                                 # both LDS at the design limit: spans 4 177 and 3 838
N_OUTS = [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, 3 * TILE + 5]
SMALL_PAIR = (192_000, 44_100)                                                 # the record of subnormal products and signed zeros


def n_in_for(n_out: int, fs_in: int, fs_out: int) -> int:
    """The shortest clip at fs_in that resamples to n_out samples at fs_out -- or, where a pair that raises the rate steps over n_out,
    to the next count above it (every count is reached when the rate falls)."""
    g = math.gcd(fs_in, fs_out)
    up, down = fs_out // g, fs_in // g
    n = max(1, ((n_out - 1) * down) // up - 2)
    while resampled_length(n, fs_in, fs_out) < n_out:
        n += 1
    assert n == 1 or resampled_length(n - 1, fs_in, fs_out) < n_out
    assert resampled_length(n, fs_in, fs_out) == n_out or (up > down and resampled_length(n, fs_in, fs_out) < n_out + -(-up // down))
    return n


def tiles(desc_row, out_stride=None, tile=TILE):
    """[(k0, cnt, span, up * hpp, arm)] of one record, by the kernel's formulas; an identity record or one the kernel refuses has none."""
    _, n_in, up, down, _, hpp, y0, n_out = (int(v) for v in desc_row)
    if out_stride is not None:
        n_out = min(n_out, out_stride)
    if up == down or not (1 <= up <= RATE_MAX and 1 <= down <= RATE_MAX and 1 <= hpp <= RATE_MAX and up * hpp <= 1 << 30):
        return []
    out = []
    for k0 in range(0, n_out, tile):
        cnt = min(n_out - k0, tile)
        yy = y0 + k0
        t0 = ((yy % up) * down) % up
        span = ((cnt - 1) * down + t0) // up + hpp
        x_lds, h_lds = span <= WIN_MAX, up * hpp <= FILT_MAX
        out.append((k0, cnt, span, up * hpp, ARMS[(0 if x_lds else 2) + (0 if h_lds else 1)]))
    return out


def single_tile_span(n_out: int, fs_in: int, fs_out: int) -> int:
    """Span of the one tile of a record of n_out < TILE outputs (hpp from resample_plan at that record's own length)."""
    n_in = n_in_for(n_out, fs_in, fs_out)
    _, hpp, up, down, y0, got, _ = resample_plan(n_in, fs_out, fs_in, np.float32)
    assert got == n_out < TILE
    (_, _, span, _, _), = tiles((0, n_in, up, down, 0, hpp, y0, n_out))
    return span


def window_threshold(fs_in: int = 352_800, fs_out: int = 48_000):
    """(n_out of the single tile with the largest span still <= WIN_MAX, the next n_out: the smallest span above it), found by bisection
    over the span, which does not fall as the record grows."""
    lo, hi = 1, TILE - 1
    assert single_tile_span(lo, fs_in, fs_out) <= WIN_MAX < single_tile_span(hi, fs_in, fs_out)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if single_tile_span(mid, fs_in, fs_out) <= WIN_MAX:
            lo = mid
        else:
            hi = mid
    return lo, hi


def table_threshold():
    """((fs_in, fs_out) with the largest up * hpp <= FILT_MAX, the pair with the smallest above it) among the pairs u - 1 -> u, which are
    coprime (up = u, about 21 taps per phase); hpp from resample_plan at the length the records use."""
    sizes = {}
    for u in range(150, 200):
        n_in = n_in_for(TILE + 1, u - 1, u)
        _, hpp, up, down, _, _, _ = resample_plan(n_in, u, u - 1, np.float32)
        assert (up, down) == (u, u - 1)
        sizes[u] = up * hpp
    below = max((u for u in sizes if sizes[u] <= FILT_MAX), key=lambda u: sizes[u])
    above = min((u for u in sizes if sizes[u] > FILT_MAX), key=lambda u: sizes[u])
    return (below - 1, below), (above - 1, above)


_RECORDS: list = []


def records():
    """[(n_in, fs_in, fs_out)] of the launch: every pair at every output count, the two window-threshold records, the two table-threshold
    pairs at two tiles, and LAST the small-products record (one full both-global tile)."""
    if not _RECORDS:
        recs = [(n_in_for(k, fi, fo), fi, fo) for fi, fo in PAIRS for k in N_OUTS]
        recs += [(n_in_for(k, 352_800, 48_000), 352_800, 48_000) for k in window_threshold()]
        recs += [(n_in_for(TILE + 1, fi, fo), fi, fo) for fi, fo in table_threshold()]
        recs.append((n_in_for(TILE, *SMALL_PAIR), *SMALL_PAIR))
        _RECORDS.extend(recs)
    return list(_RECORDS)


def descriptors(recs, dtype, gap=GAP):
    """-> (desc int64 [R, 8], filters): one condition_plan per target rate, merged into one table and one filter pool; the clips `gap`
    samples apart in the sample pool."""
    desc = np.zeros((len(recs), 8), np.int64)
    filters, at = [], 0
    for target in sorted({r[2] for r in recs}):
        sel = [i for i, r in enumerate(recs) if r[2] == target]
        cp = condition_plan([recs[i][0] for i in sel], [recs[i][1] for i in sel], target, dtype)
        desc[sel] = cp.desc
        desc[sel, 4] += at
        filters.append(cp.filters); at += cp.filters.size
    desc[:, 0] = gap + np.cumsum([0] + [r[0] + gap for r in recs[:-1]])
    return desc, np.concatenate(filters)


def coverage(desc, out_stride=None):
    """{(arm, 'k0 == 0' | 'k0 > 0'): number of tiles} over a descriptor table."""
    seen: dict = {}
    for row in desc:
        for k0, _, _, _, arm in tiles(row, out_stride):
            key = (arm, "k0 == 0" if k0 == 0 else "k0 > 0")
            seen[key] = seen.get(key, 0) + 1
    return seen


ALL_ARMS = {(arm, k) for arm in ARMS for k in ("k0 == 0", "k0 > 0")}


def small_products_clip(dtype, n: int, rng):
    """Samples so small that every product x * h is subnormal in `dtype` (|h| < 1), with some -0.0 and +0.0 among them."""
    tiny = np.finfo(dtype).tiny
    x = (rng.standard_normal(n) * 0.3).astype(dtype) * dtype(tiny)
    x[::7] = -0.0
    x[3::11] = 0.0
    return x
