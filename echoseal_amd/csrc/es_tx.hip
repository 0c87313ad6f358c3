// es_tx.hip -- frame generator: the +-1 chip sequence of a frame and the finishing step after
// the band-pass, so that whole batches of synthetic frames are produced on the device:
//   polar code bits (es_polar_encode_batch) + PN row (es_schedule_batch) + counter -> 63 preamble | 128 header | 1024
//   spread payload chips (rtwm/embedder.py:78-115 _make_frame_chips: header = lo16(ctr) MSB first, each bit repeated 8
//   times, times the header PN pn_bits(0, 128); payload chip i = code bit i times PN bit 191 + i);
//   band-pass with zero initial state carried through the frame (rtwm/embedder.py:117-136: two lfilter calls with the
//   state handed over = one pass; es_bpf_batch, bit-exact SciPy order); then the peak rule of :137-141
//   (peak = max|chips| + 1e-12; if peak > 3: chips *= 1/peak) and the cast to float32.
// The symbol kernel is written once, in es_tx_body.inc, and compiled twice: with one header PN for the batch (es_tx_frames_batch) and
// with the header PN of each frame's key read from the key ring (es_tx_frames_keyed_batch: rtwm/embedder.py:50, 105 per key).
#include "es_internal.h"

namespace {

constexpr int ES_RING_HDR_PN = 272;                               // byte offset of the header PN in a key-ring row (include/echoseal_hip.h)

#define ES_KEYED 0
#include "es_tx_body.inc"
#undef ES_KEYED
#define ES_KEYED 1          // the same kernel with a header PN per frame, from the key ring
#include "es_tx_body.inc"
#undef ES_KEYED

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
    if (!ctx->d_hdr_pn) ES_HIP_CHECK(ctx, hipMalloc(&ctx->d_hdr_pn, 16));
    ES_HIP_CHECK(ctx, hipMemcpyAsync(ctx->d_hdr_pn, hdr_pn16, 16, hipMemcpyHostToDevice, st));
    const long long cap = (long long)ctx->num_cu * 16;
    int rc = es_launch(ctx, es_tx_symbols_kernel, es_grid(B, 1, cap), 256, 0, st, code, pn_rows, ctr, pre_bits,
                       ctx->d_hdr_pn, (long long)B, frames);
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
