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

__global__ __launch_bounds__(MIX_THREADS) void es_mix_wave_kernel(const float* __restrict__ x, long long R, long long n, long long nfull,
        const float* __restrict__ chips, long long chips_stride, const long long* __restrict__ chip_off, double alpha, double floor_lin,
        float* __restrict__ out, double* __restrict__ scale_out, long long nblk)
{
    __shared__ __attribute__((aligned(16))) float sq[MIX_THREADS / 64][WV_ROW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* a = sq[wv];
    const long long total = R * nfull;
    for (long long g = (long long)blockIdx.x * (MIX_THREADS / 64) + wv; g < total; g += (long long)gridDim.x * (MIX_THREADS / 64)) {
        const long long r = g / nfull, b = g - r * nfull;
        const long long t0 = b * 1024;
        const float* xp = x + r * n + t0;
        const long long c0 = (chip_off ? chip_off[r] : 0) + t0;                // first chip of the block within row r
        const float* cp = chips + r * chips_stride;
        const bool c_fast = c0 >= 0 && c0 + 1024 <= chips_stride && (((uintptr_t)(cp + c0)) & 15) == 0;   // wave-uniform
        float4 xv[4], cv[4];
        #pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const float4*>(xp + 256 * k + 4 * lane);
        if (c_fast) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) cv[k] = *reinterpret_cast<const float4*>(cp + c0 + 256 * k + 4 * lane);
        } else {                                                               // unaligned rows, and offsets that leave the row (clamped)
            const long long hi = chips_stride - 1;
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = c0 + 256 * k + 4 * lane;
                cv[k].x = cp[clamp_ll(e, hi)]; cv[k].y = cp[clamp_ll(e + 1, hi)];
                cv[k].z = cp[clamp_ll(e + 2, hi)]; cv[k].w = cp[clamp_ll(e + 3, hi)];
            }
        }
        float mx = 0.0f, mc = 0.0f;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int e = 256 * k + 4 * lane;                                  // four samples of one leaf
            float4 q;
            q.x = xv[k].x * xv[k].x; q.y = xv[k].y * xv[k].y; q.z = xv[k].z * xv[k].z; q.w = xv[k].w * xv[k].w;
            *reinterpret_cast<float4*>(a + e + WV_PAD * (e >> 7)) = q;
            mx = max_nan(max_nan(max_nan(max_nan(mx, __builtin_fabsf(xv[k].x)), __builtin_fabsf(xv[k].y)), __builtin_fabsf(xv[k].z)), __builtin_fabsf(xv[k].w));
            mc = max_nan(max_nan(max_nan(max_nan(mc, __builtin_fabsf(cv[k].x)), __builtin_fabsf(cv[k].y)), __builtin_fabsf(cv[k].z)), __builtin_fabsf(cv[k].w));
        }
        wave_fence_lds();
        const float* al = a + (MIX_LEAF + WV_PAD) * (lane >> 3) + (lane & 7);  // accumulator j = lane & 7 of leaf lane >> 3
        float s = al[0];
        #pragma unroll
        for (int i = 1; i < 16; ++i) s += al[8 * i];
        wave_fence_lds();                                                      // the next block of this wave overwrites the row
        s = s + xor_lanes_f32<1>(s, lane);                                     // (r0+r1) ...
        s = s + xor_lanes_f32<2>(s, lane);                                     // (r0+r1)+(r2+r3) ...
        s = s + xor_lanes_f32<4>(s, lane);                                     // the leaf
        s = s + xor_lanes_f32<8>(s, lane);                                     // 256
        s = s + __shfl_xor(s, 16);                                             // 512
        s = s + __shfl_xor(s, 32);                                             // 1024: one chunk
        s = 0.0f + s;
        mx = wave_max_nan(mx); mc = wave_max_nan(mc);
        const double scale = mix_scale(s, 1024, mx, mc, alpha, floor_lin);
        if (scale_out && lane == 0) scale_out[r * nblk + b] = scale;
        const float sf = (float)scale;
        float* op = out + r * n + t0;
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            float4 o;
            o.x = mix_one(xv[k].x, cv[k].x, sf); o.y = mix_one(xv[k].y, cv[k].y, sf);
            o.z = mix_one(xv[k].z, cv[k].z, sf); o.w = mix_one(xv[k].w, cv[k].w, sf);
            *reinterpret_cast<float4*>(op + 256 * k + 4 * lane) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- any block length
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

// KEEP: the block is one chunk (m <= 8192) and stays in registers for the final pass
template <bool KEEP>
__global__ __launch_bounds__(MIX_THREADS) void es_mix_block_kernel(const float* __restrict__ x, long long R, long long n, long long block,
        long long b_first, long long b_count, const float* __restrict__ chips, long long chips_stride, const long long* __restrict__ chip_off,
        double alpha, double floor_lin, float* __restrict__ out, double* __restrict__ scale_out, long long nblk)
{
    __shared__ float sq[MIX_CHUNK + MIX_CHUNK / MIX_LEAF];
    __shared__ float node[256];                                                // sums of the split tree's nodes, heap order
    __shared__ float red[2][MIX_THREADS / 64];
    __shared__ float sum_sh;
    const int t = threadIdx.x;
    const long long total = R * b_count;
    const long long hi = chips_stride - 1;

    // heap node t: children 2t+1 and 2t+2; its path from the root is the bits of t+1 below the leading one, most significant first
    const int depth = 31 - __builtin_clz((unsigned)t + 1u);

    for (long long g = blockIdx.x; g < total; g += gridDim.x) {
        const long long r = g / b_count, b = b_first + (g - r * b_count);
        const long long t0 = b * block;
        const long long m = (n - t0 < block) ? (n - t0) : block;
        const float* xp = x + r * n + t0;
        const float* cp = chips + r * chips_stride;
        const long long c0 = (chip_off ? chip_off[r] : 0) + t0;
        float xr[KEEP ? MIX_KEEP : 1], cr[KEEP ? MIX_KEEP : 1];
        float mx = 0.0f, mc = 0.0f, s = 0.0f;                                  // s: thread 0 adds the chunk sums left to right

        for (long long ch = 0; ch < m; ch += MIX_CHUNK) {
            const int nc = (int)((m - ch < MIX_CHUNK) ? (m - ch) : MIX_CHUNK);
            __syncthreads();                                                   // the previous chunk (or block) has been summed
            if constexpr (KEEP) {
                #pragma unroll
                for (int i = 0; i < MIX_KEEP; ++i) {
                    const int e = t + MIX_THREADS * i;
                    if (e < nc) {
                        xr[i] = xp[e]; cr[i] = cp[clamp_ll(c0 + e, hi)];
                        sq[sq_at(e)] = xr[i] * xr[i];
                        mx = max_nan(mx, __builtin_fabsf(xr[i])); mc = max_nan(mc, __builtin_fabsf(cr[i]));
                    }
                }
            } else {
                for (int e = t; e < nc; e += MIX_THREADS) {
                    const float xv = xp[ch + e], cv = cp[clamp_ll(c0 + ch + e, hi)];
                    sq[sq_at(e)] = xv * xv;
                    mx = max_nan(mx, __builtin_fabsf(xv)); mc = max_nan(mc, __builtin_fabsf(cv));
                }
            }
            // this thread's node of the chunk's split tree
            int off = 0, len = nc;
            bool valid = t < 255;
            for (int d = depth - 1; d >= 0 && valid; --d) {
                if (len <= MIX_LEAF) { valid = false; break; }
                const int n2 = (len >> 1) & ~7;
                if (((t + 1) >> d) & 1) { off += n2; len -= n2; } else len = n2;
            }
            const bool leaf = valid && len <= MIX_LEAF;
            __syncthreads();
            if (leaf) node[t] = leaf_sum(sq, off, len);
            for (int d = 7; d >= 0; --d) {                                     // inner nodes, deepest first (a tree of n <= 8192 is at most 7 deep)
                __syncthreads();
                if (valid && !leaf && depth == d) node[t] = node[2 * t + 1] + node[2 * t + 2];
            }
            __syncthreads();
            if (t == 0) s += node[0];
        }

        mx = wave_max_nan(mx); mc = wave_max_nan(mc);
        if ((t & 63) == 0) { red[0][t >> 6] = mx; red[1][t >> 6] = mc; }
        if (t == 0) sum_sh = s;
        __syncthreads();
        mx = red[0][0]; mc = red[1][0];
        #pragma unroll
        for (int w = 1; w < MIX_THREADS / 64; ++w) { mx = max_nan(mx, red[0][w]); mc = max_nan(mc, red[1][w]); }
        const double scale = mix_scale(sum_sh, m, mx, mc, alpha, floor_lin);
        if (scale_out && t == 0) scale_out[r * nblk + b] = scale;
        const float sf = (float)scale;
        float* op = out + r * n + t0;
        if constexpr (KEEP) {
            #pragma unroll
            for (int i = 0; i < MIX_KEEP; ++i) {
                const int e = t + MIX_THREADS * i;
                if (e < (int)m) op[e] = mix_one(xr[i], cr[i], sf);
            }
        } else {
            for (long long e = t; e < m; e += MIX_THREADS) op[e] = mix_one(xp[e], cp[clamp_ll(c0 + e, hi)], sf);
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
