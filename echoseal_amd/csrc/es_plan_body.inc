// es_plan_body.inc -- the candidate planner, included twice by es_keyring.hip: ES_RAGGED 0 = es_plan_kernel (every row T samples),
// ES_RAGGED 1 = es_plan_ragged_kernel (row r has len_p[r] samples: which of its peaks can hold a frame is judged against that).
// One wave per (key, row): the candidate (peak slot, counter) pairs of _scan_band_multi_frame in try order.
#if ES_RAGGED
__global__ __launch_bounds__(256) void es_plan_ragged_kernel(const int32_t* __restrict__ peaks_p, const int32_t* __restrict__ npeaks_p,
        const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p, long long rows, const int32_t* __restrict__ len_p,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p,
        long long N, int C, uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p, int32_t* __restrict__ count_p,
        int32_t* __restrict__ looked_p)
#else
__global__ __launch_bounds__(256) void es_plan_kernel(const int32_t* __restrict__ peaks_p, const int32_t* __restrict__ npeaks_p,
        const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p, long long rows, int T,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p,
        long long N, int C, uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p, int32_t* __restrict__ count_p,
        int32_t* __restrict__ looked_p)
#endif
{
    const int lane = threadIdx.x & 63;
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // wave-uniform
    if (pair >= N * rows) return;
    const long long k = pair / rows, row = pair - k * rows;
#if ES_RAGGED
    const int T = ((g_ci32*)len_p)[row];                                              // the row's own sample count
#endif
    g_ci32* peaks = (g_ci32*)peaks_p + row * ES_MAX_PEAKS;
    g_cu8* hop = (g_cu8*)hop_p + k * (long long)C;
    g_u8* slot_out = (g_u8*)slot_p + pair * ES_MAX_TRIES;
    g_u32* ctr_out = (g_u32*)cctr_p + pair * ES_MAX_TRIES;
    const int band = ((g_cu8*)rowband_p)[row];
    int npk = ((g_ci32*)npeaks_p)[row] & 0xFFFF;
    npk = npk < ES_PEAK_LIMIT ? npk : ES_PEAK_LIMIT;
    const long long p0 = ((g_ci32*)base_p)[row];
    int tried = 0, looked = 0;
    #pragma unroll 1
    for (int s = 0; s < npk && tried < ES_MAX_TRIES; ++s) {
        const int start = peaks[s];
        if (start < 0 || (long long)start + ES_FRAME_LEN > T) continue;               // only peaks that can hold a frame
        const long long p = p0 + looked;
        if (p < 0 || p >= P) break;                                                   // (a header table that does not cover the row: host error)
        ++looked;
        const bool hok = ((g_cu8*)hok_p)[k * P + p] != 0;
        const int lo16 = ((g_ci32*)hlo_p)[k * P + p];
        const int est = (int)((2LL * start + ES_FRAME_LEN) / (2 * ES_FRAME_LEN));     // round(start / 1215): 1215 is odd, no ties
        bool wide = true;
        if (!hok) {                                                                   // the +-3 window, gated by the hop alone
            const int c = est - 3 + lane;
            const bool v = lane < 7 && c >= 0 && c < C && hop[c] == band;
            const unsigned long long m = __ballot(v);
            if (m) {
                const int pos = tried + lanes_below(m);
                if (v && pos < ES_MAX_TRIES) { slot_out[pos] = (uint8_t)s; ctr_out[pos] = (uint32_t)c; }
                tried += __popcll(m);
                wide = false;
            }
        }
        if (wide) {                                                                   // the +-200 window; with a header also gated by lo16
            const int lo = est - 200 > 0 ? est - 200 : 0, hi = est + 200;
            #pragma unroll 1
            for (int c0 = lo; c0 <= hi && tried < ES_MAX_TRIES; c0 += 64) {
                const int c = c0 + lane;
                const bool v = c <= hi && c < C && hop[c] == band && (!hok || (c & 0xFFFF) == lo16);
                const unsigned long long m = __ballot(v);
                const int pos = tried + lanes_below(m);
                if (v && pos < ES_MAX_TRIES) { slot_out[pos] = (uint8_t)s; ctr_out[pos] = (uint32_t)c; }
                tried += __popcll(m);
            }
        }
        tried = tried < ES_MAX_TRIES ? tried : ES_MAX_TRIES;
    }
    if (lane == 0) {
        ((g_i32*)count_p)[pair] = tried;
        if (looked_p) ((g_i32*)looked_p)[pair] = looked;
    }
}
