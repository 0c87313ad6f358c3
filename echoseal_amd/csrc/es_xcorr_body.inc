// es_xcorr_body.inc -- the float64 correlation kernel, included twice by es_sync.hip: ES_RAGGED 0 = es_xcorr_kernel (every record T
// samples), ES_RAGGED 1 = es_xcorr_ragged_kernel (record `rec` = the first len[rec] samples, clamped to [0, T], of its row; T stays the row
// stride of y, T - 62 that of corr, and the segment grid is that of T).  One text, so the two cannot drift apart, and the equal-length
// kernel is compiled from exactly the tokens it always was.
#if ES_RAGGED
__global__ __launch_bounds__(64 * XC_WAVES) void es_xcorr_ragged_kernel(const double* __restrict__ y, long long B,
        int T, const int32_t* __restrict__ len, const uint8_t* __restrict__ band, const es_band_tables* __restrict__ tabs,
        double* __restrict__ corr)
#else
__global__ __launch_bounds__(64 * XC_WAVES) void es_xcorr_kernel(const double* __restrict__ y, long long B,
        int T, const uint8_t* __restrict__ band, const es_band_tables* __restrict__ tabs,
        double* __restrict__ corr)
#endif
{
    __shared__ double s_buf[XC_WAVES][XC_NS + 2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* s = s_buf[wv];
    const int n_lags = T - (ES_PRE_L - 1);
    const int nseg = (n_lags + XC_SEG - 1) / XC_SEG;
    const long long n_items = B * nseg;
    const long long stride = (long long)gridDim.x * XC_WAVES;
    for (long long item = (long long)blockIdx.x * XC_WAVES + wv; item < n_items; item += stride) {
        const long long rec = item / nseg;
        const int lag0 = (int)(item % nseg) * XC_SEG;
#if ES_RAGGED
        int Tr = __builtin_amdgcn_readfirstlane(len[rec]);                 // samples of this record
        Tr = Tr < 0 ? 0 : (Tr > T ? T : Tr);
        if (lag0 >= Tr - (ES_PRE_L - 1)) continue;                         // wholly past the record's lags (wave-uniform): no work
        const int nr = Tr - (ES_PRE_L - 1);                                // lags of this record
        const double* yr = y + rec * T + lag0;
        const int nsamp = (Tr - lag0 < XC_NS) ? Tr - lag0 : XC_NS;         // past the record's end: zeros, as past T below
#else
        const double* yr = y + rec * T + lag0;
        const int nsamp = (T - lag0 < XC_NS) ? T - lag0 : XC_NS;
#endif
        {   // all 20 row loads are issued before the first one is consumed (one HBM round trip, not 20)
            double stage[(XC_NS + 63) / 64];
            #pragma unroll
            for (int u = 0; u < (XC_NS + 63) / 64; ++u) { const int i = lane + 64 * u; stage[u] = (i < nsamp) ? yr[i] : 0.0; }
            #pragma unroll
            for (int u = 0; u < (XC_NS + 63) / 64; ++u) { const int i = lane + 64 * u; if (i < XC_NS) s[i] = stage[u]; }
        }
        // wave-uniform band index -> template taps come through scalar loads
        const double* tpl = tabs->tpl[__builtin_amdgcn_readfirstlane((int)band[rec])];
        wave_fence_lds();

        const double* w = s + lane * XC_R;
        double num[XC_R];
        #pragma unroll
        for (int r = 0; r < XC_R; ++r) num[r] = 0.0;
        // en[r] first collects head[r] (descending partial sums of the first 18 squares), then
        // + core (squares 18..62, ascending), then + tail (squares 63..62+r, ascending): all >= 0.
        double en[XC_R], sq_head[XC_R - 1];
        double core = 0.0, tail_run = 0.0;
        // sample m meets lag r at tap k = m - r (0 <= k < 63)
        #define XC_FMAS(m, v)                                                                   \
            _Pragma("unroll") for (int r = 0; r < XC_R; ++r) {                                  \
                const int k = (m) - r;                                                          \
                if (k >= 0 && k < ES_PRE_L) num[r] = __builtin_fma((v), tpl[k], num[r]);        \
            }
        #pragma unroll
        for (int m = 0; m < XC_R - 1; ++m) {                     // samples 0..17: head squares
            const double v = w[m];
            sq_head[m] = v * v;
            XC_FMAS(m, v)
        }
        en[XC_R - 1] = 0.0;
        #pragma unroll
        for (int r = XC_R - 2; r >= 0; --r) en[r] = en[r + 1] + sq_head[r];
        #pragma unroll
        for (int m = XC_R - 1; m < ES_PRE_L; ++m) {              // samples 18..62: common core
            const double v = w[m];
            core = core + v * v;
            XC_FMAS(m, v)
        }
        #pragma unroll
        for (int r = 0; r < XC_R; ++r) en[r] = en[r] + core;
        #pragma unroll
        for (int m = ES_PRE_L; m < ES_PRE_L - 1 + XC_R; ++m) {   // samples 63..80: m = 62 + r closes lag r
            const double v = w[m];
            tail_run = tail_run + v * v;
            en[m - (ES_PRE_L - 1)] = en[m - (ES_PRE_L - 1)] + tail_run;
            XC_FMAS(m, v)
        }
        #undef XC_FMAS
        wave_fence_lds();                           // every lane has finished reading its window
        #pragma unroll
        for (int r = 0; r < XC_R; ++r) s[lane * XC_R + r] = num[r] / (__builtin_sqrt(en[r]) + 1e-12);
        wave_fence_lds();
#if ES_RAGGED
        const int nl = (nr - lag0 < XC_SEG) ? nr - lag0 : XC_SEG;
#else
        const int nl = (n_lags - lag0 < XC_SEG) ? n_lags - lag0 : XC_SEG;
#endif
        double* cr = corr + rec * n_lags + lag0;
        for (int i = lane; i < nl; i += 64) cr[i] = s[i];
        wave_fence_lds();
    }
}
