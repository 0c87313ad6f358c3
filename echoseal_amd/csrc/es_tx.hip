// es_tx.hip -- frame generator: the +-1 chip sequence of a frame and the finishing step after
// the band-pass, so that whole batches of synthetic frames are produced on the device:
//   polar code bits (es_polar_encode_batch) + PN row (es_schedule_batch) + counter -> 63 preamble | 128 header | 1024
//   spread payload chips (rtwm/embedder.py:78-115 _make_frame_chips: header = lo16(ctr) MSB first, each bit repeated 8
//   times, times the header PN pn_bits(0, 128); payload chip i = code bit i times PN bit 191 + i);
//   band-pass with zero initial state carried through the frame (rtwm/embedder.py:117-136: two lfilter calls with the
//   state handed over = one pass; es_bpf_batch, bit-exact SciPy order); then the peak rule of :137-141
//   (peak = max|chips| + 1e-12; if peak > 3: chips *= 1/peak) and the cast to float32.
// The chips of a frame are written once, in tx_symbols_frame; two thin symbol kernels hand it the 16 header-PN bytes in LDS: one header
// PN for the batch, passed by value (es_tx_frames_batch), or that of each frame's key read from the key ring (es_tx_frames_keyed_batch:
// rtwm/embedder.py:50, 105 per key).
#include "es_internal.h"
#include <cstring>

namespace {

constexpr int ES_RING_HDR_PN = 272;                               // byte offset of the header PN in a key-ring row (include/echoseal_hip.h)

// the 1215 chips of frame f, by one workgroup; hdr_pn: the frame's 16 header-PN bytes, in LDS
__device__ __forceinline__ void tx_symbols_frame(const uint8_t* __restrict__ code, const uint8_t* __restrict__ pn_rows,
        const uint32_t* __restrict__ ctr, unsigned long long pre_bits, const uint8_t* hdr_pn, long long f, float* __restrict__ sym)
{
    const uint32_t lo16 = ctr[f] & 0xFFFFu;
    const uint8_t* pn = pn_rows + f * ES_PN_BYTES;
    for (int i = threadIdx.x; i < ES_FRAME_LEN; i += 256) {
        float v;
        if (i < ES_PRE_L) {
            v = ((pre_bits >> (63 - i)) & 1ull) ? 1.0f : -1.0f;                           // bit i of the packed MLS, MSB first
        } else if (i < ES_PRE_L + ES_HDR_L) {
            const int k = i - ES_PRE_L;
            const uint32_t hb = (lo16 >> (15 - (k >> 3))) & 1u;                           // 16 bits, each repeated 8 times
            const uint32_t pb = (hdr_pn[k >> 3] >> (7 - (k & 7))) & 1u;
            v = (hb ? 1.0f : -1.0f) * (pb ? 1.0f : -1.0f);
        } else {
            const int k = i - (ES_PRE_L + ES_HDR_L);
            const uint32_t pb = (pn[i >> 3] >> (7 - (i & 7))) & 1u;                       // PN bit 191 + k
            v = (code[f * ES_POLAR_N + k] ? 1.0f : -1.0f) * (pb ? 1.0f : -1.0f);
        }
        sym[f * ES_FRAME_LEN + i] = v;
    }
}

struct HdrPn { uint32_t w[4]; };                                  // the 16 packed header-PN bytes in memory order, by value

// one header PN for the batch, a kernel argument like pre_bits
__global__ __launch_bounds__(256) void es_tx_symbols_kernel(const uint8_t* __restrict__ code, const uint8_t* __restrict__ pn_rows,
        const uint32_t* __restrict__ ctr, unsigned long long pre_bits, HdrPn hdr_pn_v, long long B, float* __restrict__ sym)
{
    __shared__ uint8_t hdr_pn[16];
    if (threadIdx.x < 16)                                             // byte t = bits 8 (t & 3) .. of word t >> 2, read from the argument segment: no private copy
        hdr_pn[threadIdx.x] = (uint8_t)(hdr_pn_v.w[threadIdx.x >> 2] >> (8 * (threadIdx.x & 3)));
    __syncthreads();
    for (long long f = blockIdx.x; f < B; f += gridDim.x) tx_symbols_frame(code, pn_rows, ctr, pre_bits, hdr_pn, f, sym);
}

// frame f takes its header PN from ring row key[f], bytes 272..287; a key index outside [0, N) reads nothing of the ring and gives a
// header PN of zero bytes
__global__ __launch_bounds__(256) void es_tx_symbols_keyed_kernel(const uint8_t* __restrict__ code, const uint8_t* __restrict__ pn_rows,
        const uint32_t* __restrict__ ctr, unsigned long long pre_bits, const uint8_t* __restrict__ ring, long long N,
        const int32_t* __restrict__ key_p, long long B, float* __restrict__ sym)
{
    __shared__ uint8_t hdr_pn[16];
    for (long long f = blockIdx.x; f < B; f += gridDim.x) {
        const long long key = key_p[f];                                                   // block-uniform
        const bool have = key >= 0 && key < N;
        __syncthreads();                                                                  // the previous frame has read its header PN
        if (threadIdx.x < 16) hdr_pn[threadIdx.x] = have ? ring[key * ES_KEYRING_BYTES + ES_RING_HDR_PN + threadIdx.x] : (uint8_t)0;
        __syncthreads();
        tx_symbols_frame(code, pn_rows, ctr, pre_bits, hdr_pn, f, sym);
    }
}

// one wave per frame: peak over the float64 chips, optional rescale, cast
__global__ __launch_bounds__(256) void es_tx_finish_kernel(const double* __restrict__ y, long long B, float* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long long stride = (long long)gridDim.x * 4;
    for (long long f = (long long)blockIdx.x * 4 + wv; f < B; f += stride) {
        const double* yr = y + f * ES_FRAME_LEN;
        double m = 0.0;
        for (int i = lane; i < ES_FRAME_LEN; i += 64) { const double a = __builtin_fabs(yr[i]); m = (a > m || a != a) ? a : m; }   // NaN wins, as np.max
        #pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const double t = __shfl_xor(m, o); m = (t > m || t != t) ? t : m; }
        const double peak = m + 1e-12;
        const bool scale = peak > 3.0;
        const double inv = 1.0 / peak;
        for (int i = lane; i < ES_FRAME_LEN; i += 64) {
            double v = yr[i];
            if (scale) v = v * inv;
            out[f * ES_FRAME_LEN + i] = (float)v;
        }
    }
}

}  // namespace

int es_launch_tx_frames(es_ctx* ctx, const uint8_t* code, const uint8_t* pn_rows, const uint8_t* band, const uint32_t* ctr,
                        unsigned long long pre_bits, const uint8_t* hdr_pn16, int64_t B, double* y_ws, float* frames, hipStream_t st)
{
    HdrPn hdr_pn;
    std::memcpy(hdr_pn.w, hdr_pn16, 16);
    const long long cap = (long long)ctx->num_cu * 16;
    int rc = es_launch(ctx, es_tx_symbols_kernel, es_grid(B, 1, cap), 256, 0, st, code, pn_rows, ctr, pre_bits, hdr_pn, (long long)B,
                       frames);
    if (rc != ES_OK) return rc;
    rc = es_launch_bpf(ctx, frames, ES_DTYPE_F32, B, ES_FRAME_LEN, band, y_ws, nullptr, st);
    if (rc != ES_OK) return rc;
    return es_launch(ctx, es_tx_finish_kernel, es_grid(B, 4, cap), 256, 0, st, y_ws, (long long)B, frames);
}

int es_launch_tx_frames_keyed(es_ctx* ctx, const uint8_t* code, const uint8_t* pn_rows, const uint8_t* band, const uint32_t* ctr,
                              unsigned long long pre_bits, const uint8_t* ring, int64_t N, const int32_t* key, int64_t B, double* y_ws,
                              float* frames, hipStream_t st)
{
    const long long cap = (long long)ctx->num_cu * 16;
    int rc = es_launch(ctx, es_tx_symbols_keyed_kernel, es_grid(B, 1, cap), 256, 0, st, code, pn_rows, ctr, pre_bits, ring, (long long)N, key,
                       (long long)B, frames);
    if (rc != ES_OK) return rc;
    rc = es_launch_bpf(ctx, frames, ES_DTYPE_F32, B, ES_FRAME_LEN, band, y_ws, nullptr, st);
    if (rc != ES_OK) return rc;
    return es_launch(ctx, es_tx_finish_kernel, es_grid(B, 4, cap), 256, 0, st, y_ws, (long long)B, frames);
}
