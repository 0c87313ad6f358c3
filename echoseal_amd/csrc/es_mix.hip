// es_mix.hip -- level mix, the last step of the transmit chain (rtwm/embedder.py:44-75 WatermarkEmbedder.process): per block of audio one
// gain from the block's RMS, its headroom and the chips' peak, then out = x + chips * gain.  Bit-identical to the NumPy code:
//
//   s      = np.add.reduce(x * x) in float32 (NumPy's order, below)
//   in_rms = (double)(sqrtf((float)((double)s / m)) + (float)1e-12)      np.mean divides the float32 sum by the count in float64 and
//                                                                        rounds to float32 (= s / (float)m while m < 2^24)
//   scale  = max(alpha * in_rms, floor); head = max(0.98 - max|x|, 0); peak = max|chips| + 1e-12      (float64, Python max / min,
//   scale  = peak > 0 ? min(scale, head / peak) : 0                                                    np.max: a NaN wins)
//   out[i] = x[i] + chips[i] * (float)scale                             (float32 multiply, float32 add, no contraction)
//
// NumPy's float32 add.reduce over a contiguous vector: the vector is cut into chunks of 8192 elements (the ufunc buffer), the chunk sums
// are added left to right starting from +0; a chunk is summed pairwise: n < 8 a plain loop from -0; n <= 128 eight accumulators
// r[j] = a[j], r[j] += a[8i + j], then ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 tail one by one; above 128 the chunk is split
// at n/2 rounded down to a multiple of 8 and the two halves are added.
//
// Two kernels.  es_mix_wave_kernel: block = 1024, one wave per block.  1024 = eight leaves of 128 = 64 chains of 16 adds: lane 8*leaf + j
// owns accumulator j of a leaf, three exchanges inside the leaves and three across them finish the sum.  The wave reads x and the chips
// once (16 bytes per lane where aligned), keeps them in registers for the maxima and the final multiply-add and writes out once; LDS only
// turns the coalesced layout into the accumulators' layout.  es_mix_block_kernel: any block length, one workgroup per block; the split
// tree of a chunk (depth <= 7 for n <= 8192) is laid out as a binary heap, thread k = node k; blocks of up to 8192 samples stay in
// registers for the final pass, longer ones are read again.
//
// Both kernels are written once, in es_mix_body.inc, and compiled three times: for recordings of one length (es_mix_batch), for records of
// unequal length in rows of one stride that take their chips from one flat pool of frames (es_mix_ragged_batch: the same block arithmetic;
// a record's blocks are those of its own length, block slots past its end do no work and write nothing), and for chunks of live streams
// (es_mix_stream_batch: the ragged form whose record first uses up the frame its stream stands in, read from the stream table where it
// lies).  es_stream_commit_kernel then moves every pushed stream on (es_stream_commit_batch): a launch of its own, because many
// workgroups of the mix read a stream's pending frame.
//
// A product or sum that is invalid (inf * 0, inf - inf) gives the negative quiet NaN the host's SSE arithmetic gives; NaNs that are
// already in x or the chips propagate unchanged on both.
#include "es_internal.h"
#include "es_wave.h"

namespace {

constexpr int MIX_CHUNK = 8192;                 // NumPy's ufunc buffer, in elements
constexpr int MIX_LEAF = 128;                   // pairwise sum: longest run summed by the eight accumulators
constexpr int MIX_THREADS = 256;
constexpr int MIX_KEEP = MIX_CHUNK / MIX_THREADS;   // samples per thread of a one-chunk block

__device__ __forceinline__ float max_nan(float m, float a) { return (a > m || a != a) ? a : m; }     // np.max: a NaN wins

__device__ __forceinline__ float wave_max_nan(float m)
{
    #pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max_nan(m, __shfl_xor(m, o));
    return m;
}

__device__ __forceinline__ float neg_qnan() { const uint32_t b = 0xFFC00000u; float f; __builtin_memcpy(&f, &b, 4); return f; }

// x + c * sf in two float32 steps; an invalid operation yields the x86 default NaN
__device__ __forceinline__ float mix_one(float x, float c, float sf)
{
    float p = c * sf;
    if (p != p && c == c && sf == sf) p = neg_qnan();
    float o = x + p;
    if (o != o && x == x && p == p) o = neg_qnan();
    return o;
}

// the gain of a block from its float32 sum of squares, its length and the two maxima (all float64 from in_rms on)
__device__ __forceinline__ double mix_scale(float s, long long m, float mx, float mc, double alpha, double floor_lin)
{
    const float mean = (float)((double)s / (double)m);
    const double in_rms = (double)(__builtin_sqrtf(mean) + (float)1e-12);
    double scale = alpha * in_rms;
    if (floor_lin > scale) scale = floor_lin;                   // Python max(a, b): b only if b > a
    double head = 0.98 - (double)mx;
    if (0.0 > head) head = 0.0;
    const double peak = (double)mc + 1e-12;
    if (peak > 0.0) {
        const double q = head / peak;
        if (q < scale) scale = q;                               // Python min(a, b): b only if b < a
    } else {
        scale = 0.0;
    }
    return scale;
}

__device__ __forceinline__ long long clamp_ll(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------- block = 1024
constexpr int WV_PAD = 8;                                       // floats between the leaves in LDS: lane 8*leaf + j reads bank 8*leaf + j + 8i
constexpr int WV_ROW = 8 * (MIX_LEAF + WV_PAD);

__device__ __forceinline__ int sq_at(int e) { return e + (e >> 7); }          // LDS index of square e: leaves 128 apart land on different banks

// sum of a run of n <= 128 squares starting at element `off` of the chunk
__device__ __forceinline__ float leaf_sum(const float* sq, int off, int n)
{
    if (n < 8) {
        float res = -0.0f;
        for (int i = 0; i < n; ++i) res += sq[sq_at(off + i)];
        return res;
    }
    float r[8];
    #pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = sq[sq_at(off + j)];
    const int n8 = n - (n & 7);
    for (int i = 8; i < n8; i += 8) {
        #pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += sq[sq_at(off + i + j)];
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = n8; i < n; ++i) res += sq[sq_at(off + i)];
    return res;
}

// records of unequal length (es_mix_ragged_batch): an index clamped to the record's own chips
__device__ __forceinline__ long long clamp_lh(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Record r of a ragged batch: its length clamped to [0, n] (the rule of es_sync_ragged_batch), and its chips [base, base + cnt) cut to the
// pool -> chips[lo .. hi].  A record without a chip is a record of length 0.  (No sum here can overflow: base + cnt is formed only where
// base < 0 < cnt or where cnt <= total - base.)
__device__ __forceinline__ long long ragged_record(long long len, long long n, long long base, long long cnt, long long total,
                                                   long long& lo, long long& hi)
{
    lo = base < 0 ? 0 : base;
    long long end = lo;                                                        // exclusive
    if (cnt > 0 && base < total) end = base < 0 ? base + cnt : (cnt > total - base ? total : base + cnt);
    if (end > total) end = total;
    hi = end - 1;
    if (end <= lo) return 0;
    return len < 0 ? 0 : (len > n ? n : len);
}

// Record r of a stream batch, a chunk of stream s: its chips are the row [the frame the stream stands in | the record's new frames], and
// its first sample takes row position `start` = off[s], or ES_FRAME_LEN where nothing is pending (off[s] = 0, and any off outside
// 1 .. ES_FRAME_LEN - 1).  -> its length clamped to [0, n], 0 for a stream outside the table; the new chips cut to the pool as
// ragged_record cuts them -> chips[lo .. hi], hi < lo where the record has none.
__device__ __forceinline__ long long stream_record(long long len, long long n, long long s, long long S, const long long* __restrict__ off,
                                                   long long base, long long cnt, long long total, long long& lo, long long& hi, long long& start)
{
    ragged_record(len, n, base, cnt, total, lo, hi);
    start = ES_FRAME_LEN;
    if (s < 0 || s >= S) return 0;
    const long long o = off[s];
    if (o > 0 && o < ES_FRAME_LEN) start = o;
    return len < 0 ? 0 : (len > n ? n : len);
}

// chip i of a stream record, i counted in the pool as if the pending frame tl[0 .. ES_FRAME_LEN) lay right before the new frames (at pb):
// below pb + ES_FRAME_LEN the pending frame, from there on the pool, clamped to the record's new chips (none: the pending frame's last chip)
__device__ __forceinline__ float stream_chip(const float* __restrict__ tl, const float* __restrict__ cp, long long pb, long long i,
                                             long long lo, long long hi)
{
    const long long p = i - pb;
    const float* src = (p < ES_FRAME_LEN || hi < lo) ? tl + clamp_ll(p, ES_FRAME_LEN - 1) : cp + clamp_lh(i, lo, hi);     // one load
    return *src;
}

#define ES_RAGGED 0
#define MIX_CHIP(i) cp[clamp_ll(i, hi)]
#include "es_mix_body.inc"
#undef MIX_CHIP
#undef ES_RAGGED
#define ES_RAGGED 1          // the same kernels for records of unequal length in one row stride, chips from one pool
#define MIX_CHIP(i) cp[clamp_lh(i, lo, hi)]
#include "es_mix_body.inc"
#undef MIX_CHIP
#undef ES_RAGGED
#define ES_RAGGED 2          // ... and for chunks of live streams: the stream's pending frame first, then new frames from the pool
#define MIX_CHIP(i) stream_chip(tl, cp, pb, i, lo, hi)
#include "es_mix_body.inc"
#undef MIX_CHIP
#undef ES_RAGGED

// After the mix of a stream batch: record r moves stream s = sid[r] on.  The chunk ends at row position end = start + len; the stream now
// stands in frame slot = end / 1215 of the row when chips of it are left (end % 1215 > 0), in the frame it has just used up when the chunk
// ended on a frame edge; slot 0 is the frame it stood in before, which stays.  One workgroup per record; records of one launch name
// different streams (the host checks), so no two workgroups write one row.
__global__ __launch_bounds__(MIX_THREADS) void es_stream_commit_kernel(long long R, long long n, const long long* __restrict__ rec_len,
        const long long* __restrict__ sid, long long S, float* tails, long long* ctr, long long* off, const float* __restrict__ chips,
        long long chips_total, const long long* __restrict__ chip_base, const long long* __restrict__ chip_cnt)
{
    for (long long r = blockIdx.x; r < R; r += gridDim.x) {
        const long long s = sid[r];
        long long lo, hi, start;
        const long long len = stream_record(rec_len[r], n, s, S, off, chip_base[r], chip_cnt[r], chips_total, lo, hi, start);
        if (s < 0 || s >= S) continue;                                         // block-uniform
        const long long end = start + len, o = end % ES_FRAME_LEN;
        const long long slot = o > 0 ? end / ES_FRAME_LEN : end / ES_FRAME_LEN - 1;          // end >= 1, and >= 1215 where o == 0
        const long long src = chip_base[r] + (slot - 1) * ES_FRAME_LEN;
        if (slot > 0 && src >= lo && src + ES_FRAME_LEN - 1 <= hi) {
            for (int i = threadIdx.x; i < ES_FRAME_LEN; i += MIX_THREADS) tails[s * ES_FRAME_LEN + i] = chips[src + i];
        }
        __syncthreads();                                                       // every thread has read off[s]
        if (threadIdx.x == 0) {
            ctr[s] = (ctr[s] + (end + ES_FRAME_LEN - 1) / ES_FRAME_LEN - 1) & 0xFFFFFFFFll;
            off[s] = o;
        }
    }
}

}  // namespace

int es_launch_mix(es_ctx* ctx, const float* x, int64_t R, int64_t n, int block, const float* chips, int64_t chips_stride,
                  const int64_t* chip_off, double alpha, double floor_lin, float* out, double* scale_out, hipStream_t st)
{
    const long long nblk = (n + block - 1) / block;
    const long long cap = (long long)ctx->num_cu * 2048;                      // the kernels stride over what a larger batch adds
    long long b_first = 0, b_count = nblk;
    // one wave per block: the reference's own block length, rows and pointers that allow 16-byte accesses
    if (block == 1024 && n % 4 == 0 && n >= 1024 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0) {
        const long long nfull = n / 1024;
        const int rc = es_launch(ctx, es_mix_wave_kernel, es_grid(R * nfull, 4, cap), MIX_THREADS, 0, st, x, (long long)R, (long long)n, nfull, chips,
                                 (long long)chips_stride, (const long long*)chip_off, alpha, floor_lin, out, scale_out, nblk);
        if (rc != ES_OK) return rc;
        b_first = nfull; b_count = nblk - nfull;                              // the short last block of each row, if any
        if (b_count == 0) return ES_OK;
    }
    return es_launch(ctx, block <= MIX_CHUNK ? es_mix_block_kernel<true> : es_mix_block_kernel<false>, es_grid(R * b_count, 1, cap), MIX_THREADS, 0, st,
                     x, (long long)R, (long long)n, (long long)block, b_first, b_count, chips, (long long)chips_stride, (const long long*)chip_off,
                     alpha, floor_lin, out, scale_out, nblk);
}

int es_launch_mix_ragged(es_ctx* ctx, const es_mix_ragged_args& a, hipStream_t st)
{
    const long long nblk = (a.n_stride + a.block - 1) / a.block;
    const long long cap = (long long)ctx->num_cu * 2048;                      // the kernels stride over what a larger batch adds
    const long long* len = (const long long*)a.len; const long long* base = (const long long*)a.chip_base; const long long* cnt = (const long long*)a.chip_cnt;
    int tail_only = 0;
    // one wave per full block under the conditions of es_launch_mix; which slots are full blocks only the device knows
    if (a.block == 1024 && a.n_stride % 4 == 0 && ((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.out & 15) == 0) {
        const long long nfull = a.n_stride / 1024;
        if (nfull) {
            const int rc = es_launch(ctx, es_mix_ragged_wave_kernel, es_grid(a.R * nfull, 4, cap), MIX_THREADS, 0, st, a.x, (long long)a.R,
                                     (long long)a.n_stride, nfull, len, a.chips, (long long)a.chips_total, base, cnt, a.alpha, a.floor_lin, a.out,
                                     a.scale_out, nblk);
            if (rc != ES_OK) return rc;
        }
        tail_only = 1;                                                        // the short last block of each record, if any
    }
    return es_launch(ctx, a.block <= MIX_CHUNK ? es_mix_ragged_block_kernel<true> : es_mix_ragged_block_kernel<false>,
                     es_grid(tail_only ? a.R : a.R * nblk, 1, cap), MIX_THREADS, 0, st, a.x, (long long)a.R, (long long)a.n_stride, (long long)a.block,
                     tail_only, len, a.chips, (long long)a.chips_total, base, cnt, a.alpha, a.floor_lin, a.out, a.scale_out, nblk);
}

int es_launch_mix_stream(es_ctx* ctx, const es_mix_stream_args& a, hipStream_t st)
{
    const long long nblk = (a.n_stride + a.block - 1) / a.block;
    const long long cap = (long long)ctx->num_cu * 2048;                      // the kernels stride over what a larger batch adds
    const long long* len = (const long long*)a.len; const long long* sid = (const long long*)a.sid; const long long* off = (const long long*)a.off;
    const long long* base = (const long long*)a.chip_base; const long long* cnt = (const long long*)a.chip_cnt;
    int tail_only = 0;
    // the cut of es_launch_mix_ragged: one wave per full block, each record's short last block on the workgroup kernel
    if (a.block == 1024 && a.n_stride % 4 == 0 && ((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.out & 15) == 0) {
        const long long nfull = a.n_stride / 1024;
        if (nfull) {
            const int rc = es_launch(ctx, es_mix_stream_wave_kernel, es_grid(a.R * nfull, 4, cap), MIX_THREADS, 0, st, a.x, (long long)a.R,
                                     (long long)a.n_stride, nfull, len, sid, (long long)a.S, a.tail, off, a.chips, (long long)a.chips_total, base, cnt,
                                     a.alpha, a.floor_lin, a.out, a.scale_out, nblk);
            if (rc != ES_OK) return rc;
        }
        tail_only = 1;
    }
    return es_launch(ctx, a.block <= MIX_CHUNK ? es_mix_stream_block_kernel<true> : es_mix_stream_block_kernel<false>,
                     es_grid(tail_only ? a.R : a.R * nblk, 1, cap), MIX_THREADS, 0, st, a.x, (long long)a.R, (long long)a.n_stride, (long long)a.block,
                     tail_only, len, sid, (long long)a.S, a.tail, off, a.chips, (long long)a.chips_total, base, cnt, a.alpha, a.floor_lin, a.out,
                     a.scale_out, nblk);
}

int es_launch_stream_commit(es_ctx* ctx, const es_stream_commit_args& a, hipStream_t st)
{
    return es_launch(ctx, es_stream_commit_kernel, es_grid(a.R, 1, (long long)ctx->num_cu * 2048), MIX_THREADS, 0, st, (long long)a.R,
                     (long long)a.n_stride, (const long long*)a.len, (const long long*)a.sid, (long long)a.S, a.tail, (long long*)a.ctr,
                     (long long*)a.off, a.chips, (long long)a.chips_total, (const long long*)a.chip_base, (const long long*)a.chip_cnt);
}
