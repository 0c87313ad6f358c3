// es_pick_body.inc -- the float64 threshold / peak kernel, included twice by es_sync.hip: ES_RAGGED 0 = es_pick_kernel<IN_LDS, NT> (rows
// of n lags), ES_RAGGED 1 = es_pick_ragged_kernel<NT> (record `rec` has len[rec] - 62 lags, len clamped to [0, T], at the row stride
// T - 62, read from global memory), ES_RAGGED 2 = es_pick_at_kernel<NT> (record `rec` is a window read in place: nlag[rec] lags from
// column col[rec] of row row[rec] (NULL = rec) of n_rows rows of `stride` columns; col is clamped to [0, stride], nlag to what the row
// holds from there, a row outside the array is a window without a lag).  One text; the equal-length kernel is compiled from exactly
// the tokens it always was.
#if ES_RAGGED == 2
template <int NT>
__global__ __launch_bounds__(NT) void es_pick_at_kernel(const double* __restrict__ corr, long long n_rows, int stride, long long B,
        const int32_t* __restrict__ row, const int32_t* __restrict__ col, const int32_t* __restrict__ nlag, double* __restrict__ thr_out,
        int32_t* __restrict__ peaks, int32_t* __restrict__ npeaks)
{
    constexpr bool IN_LDS = false;                    // windows of any length inside long rows: always read from global memory
#elif ES_RAGGED
template <int NT>
__global__ __launch_bounds__(NT) void es_pick_ragged_kernel(const double* __restrict__ corr, long long B, int T,
        const int32_t* __restrict__ len, double* __restrict__ thr_out, int32_t* __restrict__ peaks, int32_t* __restrict__ npeaks)
{
    constexpr bool IN_LDS = false;                    // rows of any length: always read from global memory
#else
template <bool IN_LDS, int NT>
__global__ __launch_bounds__(NT) void es_pick_kernel(const double* __restrict__ corr, long long B,
        int n, double* __restrict__ thr_out, int32_t* __restrict__ peaks, int32_t* __restrict__ npeaks)
{
#endif
    __shared__ double s_row[IN_LDS ? PK_LDS_N : 1];
    __shared__ uint32_t s_hist[256];
    __shared__ uint64_t s_pref;
    __shared__ int s_k;
    __shared__ double s_bv[NT];
    __shared__ int s_bi[NT];
    __shared__ int s_taken[5];
    __shared__ int s_flag;
    __shared__ uint32_t s_cnt;
    const int min_distance = ES_FRAME_LEN / 2;        // 607

    for (long long rec = blockIdx.x; rec < B; rec += gridDim.x) {
#if ES_RAGGED
#if ES_RAGGED == 2
        const long long rw = row ? (long long)row[rec] : rec;
        int c0 = col[rec];
        c0 = c0 < 0 ? 0 : (c0 > stride ? stride : c0);
        int n = nlag[rec];                             // the window's own lag count
        if (n > stride - c0) n = stride - c0;
        if (rw < 0 || rw >= n_rows) n = 0;
        const double* cg = corr + (rw < 0 || rw >= n_rows ? 0 : rw) * stride + c0;
#else
        int Tr = len[rec];
        Tr = Tr < 0 ? 0 : (Tr > T ? T : Tr);
        const int n = Tr - (ES_PRE_L - 1);             // the record's own lag count
        const double* cg = corr + rec * (T - (ES_PRE_L - 1));
#endif
        if (n < 1) {                                   // shorter than the template: no lag, no peak (rtwm/detector.py:71-73); block-uniform
            if (threadIdx.x < ES_MAX_PEAKS) peaks[rec * ES_MAX_PEAKS + threadIdx.x] = -1;
            if (threadIdx.x == 0) { npeaks[rec] = 0; thr_out[rec] = 0.0; }
            continue;
        }
#else
        const double* cg = corr + rec * n;
#endif
        const double* c = cg;
        if (IN_LDS) {
            for (int i = threadIdx.x; i < n; i += NT) s_row[i] = cg[i];
            c = s_row;
        }
        __syncthreads();
        double thr = 0.95;
        if (!block_threshold_saturates<NT>(c, n, s_hist, &s_k)) {      // (usually proven in one pass; else the exact order statistics)
            const double med = block_median<false, NT>(c, n, 0.0, s_hist, &s_pref, &s_k);
            const double mad = block_median<true, NT>(c, n, med, s_hist, &s_pref, &s_k) + 1e-12;
            thr = med + 4.5 * 1.4826 * mad;
            if (0.95 < thr) thr = 0.95;
        }

        // ascending scan over lags >= thr; each candidate is checked by the whole block
        int total = 0;
        for (int base = 0; base < n; base += NT) {
            const int i = base + threadIdx.x;
            const bool cand = (i < n) && !(c[i] < thr);
            unsigned long long mask[NT / 64];
            if (threadIdx.x == 0) s_cnt = 0;
            __syncthreads();
            const unsigned long long bal = __ballot(cand);
            if ((threadIdx.x & 63) == 0) { ((unsigned long long*)s_bv)[threadIdx.x >> 6] = bal; if (bal) atomicOr(&s_cnt, 1u); }
            __syncthreads();
            if (s_cnt == 0) continue;                  // no candidate among these 256 lags (uniform)
            #pragma unroll
            for (int w = 0; w < NT / 64; ++w) mask[w] = ((unsigned long long*)s_bv)[w];
            __syncthreads();
            for (int w = 0; w < NT / 64; ++w) {
                unsigned long long m = mask[w];
                while (m) {                            // uniform across the block
                    const int bit = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int ci = base + 64 * w + bit;
                    const double cv = c[ci];
                    int lo = ci - min_distance; if (lo < 0) lo = 0;
                    int hi = ci + min_distance + 1; if (hi > n) hi = n;
                    int bigger = 0;
                    for (int j = lo + threadIdx.x; j < hi; j += NT) bigger |= (c[j] > cv);
                    if (__syncthreads_or(bigger) == 0) {
                        if (threadIdx.x == 0 && total < ES_MAX_PEAKS) peaks[rec * ES_MAX_PEAKS + total] = ci;
                        ++total;
                    }
                }
            }
        }

        if (total == 0) {
            // fallback: five largest correlations, descending; equal values -> higher index first
            const int kmax = n < 5 ? n : 5;
            for (int r = 0; r < kmax; ++r) {
                double bv = 0.0; int bidx = -1;
                for (int i = threadIdx.x; i < n; i += NT) {
                    bool used = false;
                    for (int qd = 0; qd < r; ++qd) used |= (s_taken[qd] == i);
                    if (used) continue;
                    const double ci = c[i];
                    if (bidx < 0 || ci > bv || (ci == bv && i > bidx)) { bv = ci; bidx = i; }
                }
                s_bv[threadIdx.x] = bv; s_bi[threadIdx.x] = bidx;
                __syncthreads();
                for (int sft = NT / 2; sft > 0; sft >>= 1) {
                    if (threadIdx.x < sft) {
                        const double ov = s_bv[threadIdx.x + sft]; const int oi = s_bi[threadIdx.x + sft];
                        const double mv = s_bv[threadIdx.x]; const int mi = s_bi[threadIdx.x];
                        if (oi >= 0 && (mi < 0 || ov > mv || (ov == mv && oi > mi))) {
                            s_bv[threadIdx.x] = ov; s_bi[threadIdx.x] = oi;
                        }
                    }
                    __syncthreads();
                }
                if (threadIdx.x == 0) { s_taken[r] = s_bi[0]; peaks[rec * ES_MAX_PEAKS + r] = s_bi[0]; }
                __syncthreads();
            }
            if (threadIdx.x == 0) npeaks[rec] = kmax | (1 << 30);
            total = kmax;
        } else if (threadIdx.x == 0) {
            npeaks[rec] = total;
        }
        if ((int)threadIdx.x >= total && threadIdx.x < ES_MAX_PEAKS) peaks[rec * ES_MAX_PEAKS + threadIdx.x] = -1;   // unused tail
        if (threadIdx.x == 0) thr_out[rec] = thr;
        (void)s_flag;
        __syncthreads();
    }
}
