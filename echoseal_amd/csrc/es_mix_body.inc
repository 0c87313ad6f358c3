// es_mix_body.inc -- the two level-mix kernels, included three times by es_mix.hip: ES_RAGGED 0 = es_mix_wave_kernel / es_mix_block_kernel
// (every recording n samples, chip row r of chips_stride chips), ES_RAGGED 1 = es_mix_ragged_wave_kernel / es_mix_ragged_block_kernel
// (recording r has len[r] samples in a row of n, its chips lie at chip_base[r] of one flat pool), ES_RAGGED 2 = es_mix_stream_wave_kernel /
// es_mix_stream_block_kernel (record r is a chunk of stream sid[r]: its chips are the rest of the stream's pending frame, tails[sid[r]] from
// off[sid[r]] on, and then the record's new frames at chip_base[r] of the pool; both are read where they lie).  The arithmetic of a block
// is one text; what differs is where a block's samples and chips lie and which block slots exist.  MIX_CHIP(i): chip i of the row or pool.

// ---------------------------------------------------------------------------------------------------------------- block = 1024
#if ES_RAGGED == 2
// the ragged kernel's slots; c0 = pool index of the block's first chip, as if the pending frame lay in the pool right before chip_base[r]
__global__ __launch_bounds__(MIX_THREADS) void es_mix_stream_wave_kernel(const float* __restrict__ x, long long R, long long n, long long nfull,
        const long long* __restrict__ rec_len, const long long* __restrict__ sid, long long S, const float* __restrict__ tails,
        const long long* __restrict__ off, const float* __restrict__ chips, long long chips_total, const long long* __restrict__ chip_base,
        const long long* __restrict__ chip_cnt, double alpha, double floor_lin, float* __restrict__ out, double* __restrict__ scale_out,
        long long nblk)
#elif ES_RAGGED
// slot g = (row r, block b) of R * nfull slots, nfull = n / 1024: only the slots that are full blocks of their record do work
__global__ __launch_bounds__(MIX_THREADS) void es_mix_ragged_wave_kernel(const float* __restrict__ x, long long R, long long n, long long nfull,
        const long long* __restrict__ rec_len, const float* __restrict__ chips, long long chips_total, const long long* __restrict__ chip_base,
        const long long* __restrict__ chip_cnt, double alpha, double floor_lin, float* __restrict__ out, double* __restrict__ scale_out,
        long long nblk)
#else
__global__ __launch_bounds__(MIX_THREADS) void es_mix_wave_kernel(const float* __restrict__ x, long long R, long long n, long long nfull,
        const float* __restrict__ chips, long long chips_stride, const long long* __restrict__ chip_off, double alpha, double floor_lin,
        float* __restrict__ out, double* __restrict__ scale_out, long long nblk)
#endif
{
    __shared__ __attribute__((aligned(16))) float sq[MIX_THREADS / 64][WV_ROW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* a = sq[wv];
    const long long total = R * nfull;
    for (long long g = (long long)blockIdx.x * (MIX_THREADS / 64) + wv; g < total; g += (long long)gridDim.x * (MIX_THREADS / 64)) {
        const long long r = g / nfull, b = g - r * nfull;
        const long long t0 = b * 1024;
        const float* xp = x + r * n + t0;
#if ES_RAGGED == 2
        long long lo, hi, start;                                               // the record's new chips: chips[lo .. hi] of the pool
        if (t0 + 1024 > stream_record(rec_len[r], n, sid[r], S, off, chip_base[r], chip_cnt[r], chips_total, lo, hi, start)) continue;
        const long long pb = chip_base[r] - ES_FRAME_LEN;                      // where the pending frame would start
        const long long c0 = pb + start + t0;
        const float* cp = chips;
        const float* tl = tails + sid[r] * ES_FRAME_LEN;
        const bool c_fast = start + t0 >= ES_FRAME_LEN && c0 >= lo && c0 + 1024 <= hi + 1 && (((uintptr_t)(cp + c0)) & 15) == 0;   // wave-uniform
#elif ES_RAGGED
        long long lo, hi;                                                      // the record's chips: chips[lo .. hi] of the pool
        if (t0 + 1024 > ragged_record(rec_len[r], n, chip_base[r], chip_cnt[r], chips_total, lo, hi)) continue;   // wave-uniform
        const long long c0 = chip_base[r] + t0;                                // first chip of the block within the pool
        const float* cp = chips;
        const bool c_fast = c0 >= lo && c0 + 1024 <= hi + 1 && (((uintptr_t)(cp + c0)) & 15) == 0;          // wave-uniform
#else
        const long long c0 = (chip_off ? chip_off[r] : 0) + t0;                // first chip of the block within row r
        const float* cp = chips + r * chips_stride;
        const bool c_fast = c0 >= 0 && c0 + 1024 <= chips_stride && (((uintptr_t)(cp + c0)) & 15) == 0;   // wave-uniform
#endif
        float4 xv[4], cv[4];
        #pragma unroll
        for (int k = 0; k < 4; ++k) xv[k] = *reinterpret_cast<const float4*>(xp + 256 * k + 4 * lane);
        if (c_fast) {
            #pragma unroll
            for (int k = 0; k < 4; ++k) cv[k] = *reinterpret_cast<const float4*>(cp + c0 + 256 * k + 4 * lane);
        } else {                                                               // unaligned rows, offsets that leave the row (clamped), two sources
#if !ES_RAGGED
            const long long hi = chips_stride - 1;
#endif
            #pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = c0 + 256 * k + 4 * lane;
                cv[k].x = MIX_CHIP(e); cv[k].y = MIX_CHIP(e + 1); cv[k].z = MIX_CHIP(e + 2); cv[k].w = MIX_CHIP(e + 3);
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
// KEEP: the block is one chunk (m <= 8192) and stays in registers for the final pass
#if ES_RAGGED == 2
template <bool KEEP>
__global__ __launch_bounds__(MIX_THREADS) void es_mix_stream_block_kernel(const float* __restrict__ x, long long R, long long n, long long block,
        int tail_only, const long long* __restrict__ rec_len, const long long* __restrict__ sid, long long S, const float* __restrict__ tails,
        const long long* __restrict__ off, const float* __restrict__ chips, long long chips_total, const long long* __restrict__ chip_base,
        const long long* __restrict__ chip_cnt, double alpha, double floor_lin, float* __restrict__ out, double* __restrict__ scale_out,
        long long nblk)
#elif ES_RAGGED
// tail_only: item g = record g's short last block (the full ones ran on the wave kernel); else item g = (row, block slot) of R * nblk
template <bool KEEP>
__global__ __launch_bounds__(MIX_THREADS) void es_mix_ragged_block_kernel(const float* __restrict__ x, long long R, long long n, long long block,
        int tail_only, const long long* __restrict__ rec_len, const float* __restrict__ chips, long long chips_total,
        const long long* __restrict__ chip_base, const long long* __restrict__ chip_cnt, double alpha, double floor_lin, float* __restrict__ out,
        double* __restrict__ scale_out, long long nblk)
#else
template <bool KEEP>
__global__ __launch_bounds__(MIX_THREADS) void es_mix_block_kernel(const float* __restrict__ x, long long R, long long n, long long block,
        long long b_first, long long b_count, const float* __restrict__ chips, long long chips_stride, const long long* __restrict__ chip_off,
        double alpha, double floor_lin, float* __restrict__ out, double* __restrict__ scale_out, long long nblk)
#endif
{
    __shared__ float sq[MIX_CHUNK + MIX_CHUNK / MIX_LEAF];
    __shared__ float node[256];                                                // sums of the split tree's nodes, heap order
    __shared__ float red[2][MIX_THREADS / 64];
    __shared__ float sum_sh;
    const int t = threadIdx.x;
#if ES_RAGGED
    const long long total = tail_only ? R : R * nblk;
#else
    const long long total = R * b_count;
    const long long hi = chips_stride - 1;
#endif

    // heap node t: children 2t+1 and 2t+2; its path from the root is the bits of t+1 below the leading one, most significant first
    const int depth = 31 - __builtin_clz((unsigned)t + 1u);

    for (long long g = blockIdx.x; g < total; g += gridDim.x) {
#if ES_RAGGED
        const long long r = tail_only ? g : g / nblk;
#if ES_RAGGED == 2
        long long lo, hi, start;                                               // the record's new chips: chips[lo .. hi] of the pool
        const long long nr = stream_record(rec_len[r], n, sid[r], S, off, chip_base[r], chip_cnt[r], chips_total, lo, hi, start);
#else
        long long lo, hi;                                                      // the record's chips: chips[lo .. hi] of the pool
        const long long nr = ragged_record(rec_len[r], n, chip_base[r], chip_cnt[r], chips_total, lo, hi);
#endif
        const long long b = tail_only ? nr / block : g - r * nblk;
        const long long t0 = b * block;
        if (t0 >= nr) continue;                                                // a slot past the record's end (block-uniform)
        const long long m = (nr - t0 < block) ? (nr - t0) : block;
        const float* xp = x + r * n + t0;
        const float* cp = chips;
#if ES_RAGGED == 2
        const long long pb = chip_base[r] - ES_FRAME_LEN;                      // where the pending frame would start
        const long long c0 = pb + start + t0;
        const float* tl = tails + sid[r] * ES_FRAME_LEN;
#else
        const long long c0 = chip_base[r] + t0;
#endif
#else
        const long long r = g / b_count, b = b_first + (g - r * b_count);
        const long long t0 = b * block;
        const long long m = (n - t0 < block) ? (n - t0) : block;
        const float* xp = x + r * n + t0;
        const float* cp = chips + r * chips_stride;
        const long long c0 = (chip_off ? chip_off[r] : 0) + t0;
#endif
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
                        xr[i] = xp[e]; cr[i] = MIX_CHIP(c0 + e);
                        sq[sq_at(e)] = xr[i] * xr[i];
                        mx = max_nan(mx, __builtin_fabsf(xr[i])); mc = max_nan(mc, __builtin_fabsf(cr[i]));
                    }
                }
            } else {
                for (int e = t; e < nc; e += MIX_THREADS) {
                    const float xv = xp[ch + e], cv = MIX_CHIP(c0 + ch + e);
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
            for (long long e = t; e < m; e += MIX_THREADS) op[e] = mix_one(xp[e], MIX_CHIP(c0 + e), sf);
        }
    }
}
