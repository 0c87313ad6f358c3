// es_api.hip -- C ABI of libechoseal_hip.so (see include/echoseal_hip.h): context, tables,
// argument checking and dispatch to the kernel launchers.  No torch types, no global state.
#include "es_internal.h"
#include "es_exp_tab.h"

#include <cmath>
#include <cstring>
#include <new>

namespace {
std::string g_create_err;
const uint64_t kExpTab[ES_EXP_TAB_WORDS] = ES_EXP_TAB_INIT;

struct DeviceGuard {
    int prev = -1; bool ok = true;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; ok = (hipSetDevice(dev) == hipSuccess); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

int fail(es_ctx* ctx, int code, const char* msg) { ctx->err = msg; return code; }

bool capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}
}  // namespace

int es_slab_enter(es_ctx* ctx, int domain, int shape, bool shareable, hipStream_t st)
{
    if (capturing(st)) return ES_OK;                            // a captured graph orders its own nodes
    es_ctx::slab_use& u = ctx->slab[domain];
    for (size_t k = 0; k < u.users.size();) {
        es_ctx::slab_use::user& w = u.users[k];
        const bool compatible = shareable && w.shareable && w.shape == shape;
        if (w.st != st && hipEventQuery(w.done) == hipSuccess) {               // that stream's last launch here has finished: forget it
            (void)hipEventDestroy(w.done);
            u.users[k] = u.users.back(); u.users.pop_back();
            continue;
        }
        // another slot geometry (or a kernel that indexes the slab by block): this launch is ordered behind that user's last one ON THE DEVICE.
        // (Also for an entry of `st` itself: normally a no-op, and right if the handle value belongs to a new stream by now.)
        if (!compatible) ES_HIP_CHECK(ctx, hipStreamWaitEvent(st, w.done, 0));
        ++k;
    }
    return ES_OK;
}

int es_slab_leave(es_ctx* ctx, int domain, int shape, bool shareable, hipStream_t st)
{
    if (capturing(st)) return ES_OK;
    es_ctx::slab_use& u = ctx->slab[domain];
    es_ctx::slab_use::user* mine = nullptr;
    for (es_ctx::slab_use::user& w : u.users) if (w.st == st) mine = &w;
    if (!mine) {
        hipEvent_t ev;
        ES_HIP_CHECK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        u.users.push_back({st, ev, shape, shareable});
        mine = &u.users.back();
    }
    mine->shape = shape; mine->shareable = shareable;
    ES_HIP_CHECK(ctx, hipEventRecord(mine->done, st));
    return ES_OK;
}

// A launch that draws its frames from a counter gets a counter of its own.  Eager launches rotate over the first ES_CURSOR_RING -
// ES_CURSOR_CAPTURED counters (one is reused only after that many further launches of the context); a launch recorded into a stream
// capture takes one of the last ES_CURSOR_CAPTURED for good -- its graph may be replayed at any time, beside any eager launch.
#define ES_STR_(x) #x
#define ES_STR(x) ES_STR_(x)
int es_cursor_next(es_ctx* ctx, hipStream_t st, int** cursor)
{
    if (capturing(st)) {
        if (ctx->cursor_captured >= ES_CURSOR_CAPTURED) {
            ctx->err = "es_scl_batch: this context has recorded its " ES_STR(ES_CURSOR_CAPTURED) " list-decoder launches with skip_if_hard_ok into stream captures; use another context";
            return ES_ENOMEM;
        }
        *cursor = ctx->d_cursors + (ES_CURSOR_RING - 1 - ctx->cursor_captured++);
        return ES_OK;
    }
    *cursor = ctx->d_cursors + (ctx->cursor_next++ % (ES_CURSOR_RING - ES_CURSOR_CAPTURED));
    return ES_OK;
}

extern "C" {

int es_abi_version(void) { return ES_ABI_VERSION; }

int es_info_bytes(const es_ctx* ctx) { return (ctx && ctx->n_info >= 9) ? (ctx->n_info - 8 + 7) / 8 : ES_INFO_BYTES; }

const char* es_last_error(const es_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

es_ctx* es_create(int device, int list_size_max)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "no HIP device visible"; return nullptr; }
    if (device < 0 || device >= ndev) { g_create_err = "device index out of range"; return nullptr; }
    if (list_size_max < 0 || list_size_max > ES_MAX_LIST) {
        g_create_err = "list_size_max must be in [0, " + std::to_string(ES_MAX_LIST) + "] (0: a front-end context without list-decoder scratch)";
        return nullptr;
    }
    es_ctx* ctx = new (std::nothrow) es_ctx();
    if (!ctx) { g_create_err = "out of host memory"; return nullptr; }
    ctx->device = device;
    ctx->list_size_max = list_size_max;
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    if (!g.ok || hipGetDeviceProperties(&prop, device) != hipSuccess) { g_create_err = "hipGetDeviceProperties failed"; delete ctx; return nullptr; }
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    es_host_sbox(ctx->h_sbox);
    if (hipMalloc(&ctx->d_tables, sizeof(es_band_tables)) != hipSuccess ||
        hipMalloc(&ctx->d_data_pos, sizeof(uint16_t) * ES_POLAR_N) != hipSuccess ||
        hipMalloc(&ctx->d_exp_tab, sizeof(kExpTab)) != hipSuccess ||
        hipMemcpy(ctx->d_exp_tab, kExpTab, sizeof(kExpTab), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&ctx->d_sbox, sizeof ctx->h_sbox) != hipSuccess ||
        hipMemcpy(ctx->d_sbox, ctx->h_sbox, sizeof ctx->h_sbox, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_err = "device allocation failed in es_create";
        es_destroy(ctx);
        return nullptr;
    }
    if (list_size_max == 0) return ctx;                /* front-end context (band-pass, sync, demodulator, header, TX ...): no list-decoder slabs */
    /* every launch-time buffer the SCL kernel needs is allocated here, so es_scl_batch only
       enqueues work (hipGraph-capturable) */
    ctx->scl_scratch_bytes = es_scl_scratch_bytes(ctx);
    if (es_scl_multi_scratch_bytes(ctx) > ctx->scl_scratch_bytes) ctx->scl_scratch_bytes = es_scl_multi_scratch_bytes(ctx);
    if (hipMalloc(&ctx->d_scl_scratch, ctx->scl_scratch_bytes) != hipSuccess) {
        g_create_err = "device allocation of the SCL scratch slab failed";
        ctx->d_scl_scratch = nullptr;
        es_destroy(ctx);
        return nullptr;
    }
    if (hipMalloc(&ctx->d_slot_bits, 64 * sizeof(unsigned)) != hipSuccess || hipMemset(ctx->d_slot_bits, 0, 64 * sizeof(unsigned)) != hipSuccess) {
        g_create_err = "device allocation of the slab slot bitmap failed";
        es_destroy(ctx);
        return nullptr;
    }
    ctx->wide_enabled = list_size_max > 32;
    ctx->wide_scratch_bytes = es_scl_wide_scratch_bytes(ctx, &ctx->wide_lanes);
    ctx->wide_slot_words = (int)((ctx->wide_lanes / 64 + 31) / 32);                 /* a bit per one-wave block of the slab, at least 128 words */
    if (ctx->wide_slot_words < 128) ctx->wide_slot_words = 128;
    if (hipMalloc(&ctx->d_wide_slot_bits, ctx->wide_slot_words * sizeof(unsigned)) != hipSuccess ||
        hipMemset(ctx->d_wide_slot_bits, 0, ctx->wide_slot_words * sizeof(unsigned)) != hipSuccess) {
        g_create_err = "device allocation of the slab slot bitmap failed";
        es_destroy(ctx);
        return nullptr;
    }
    if (hipMalloc(&ctx->d_cursors, ES_CURSOR_RING * sizeof(int)) != hipSuccess || hipMemset(ctx->d_cursors, 0, ES_CURSOR_RING * sizeof(int)) != hipSuccess) {
        g_create_err = "device allocation of the frame counters failed";
        es_destroy(ctx);
        return nullptr;
    }
    if (ctx->wide_scratch_bytes && hipMalloc(&ctx->d_wide_scratch, ctx->wide_scratch_bytes) != hipSuccess) {
        g_create_err = "device allocation of the wide-list SCL scratch slab failed";
        ctx->d_wide_scratch = nullptr;
        es_destroy(ctx);
        return nullptr;
    }
    return ctx;
}

void es_destroy(es_ctx* ctx)
{
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    for (es_ctx::slab_use& u : ctx->slab) for (es_ctx::slab_use::user& w : u.users) (void)hipEventDestroy(w.done);
    if (ctx->d_tables) (void)hipFree(ctx->d_tables);
    if (ctx->d_data_pos) (void)hipFree(ctx->d_data_pos);
    if (ctx->d_exp_tab) (void)hipFree(ctx->d_exp_tab);
    if (ctx->d_scl_scratch) (void)hipFree(ctx->d_scl_scratch);
    if (ctx->d_slot_bits) (void)hipFree(ctx->d_slot_bits);
    if (ctx->d_ws_corr) (void)hipFree(ctx->d_ws_corr);
    if (ctx->d_wide_scratch) (void)hipFree(ctx->d_wide_scratch);
    if (ctx->d_wide_slot_bits) (void)hipFree(ctx->d_wide_slot_bits);
    if (ctx->d_sbox) (void)hipFree(ctx->d_sbox);
    if (ctx->d_cursors) (void)hipFree(ctx->d_cursors);
    delete ctx;
}

int es_set_tables(es_ctx* ctx, const double* ba, const double* tpl, const float* taps,
                  const int32_t* ntaps, const uint8_t* frozen)
{
    if (!ctx) return ES_EINVAL;
    if (!ba || !tpl || !taps || !ntaps || !frozen) return fail(ctx, ES_EINVAL, "es_set_tables: null table pointer");
    es_band_tables h;
    std::memset(&h, 0, sizeof h);
    for (int b = 0; b < ES_NBANDS; ++b) {
        const double a0 = ba[b * 18 + 9];
        if (a0 == 0.0) return fail(ctx, ES_EINVAL, "es_set_tables: a[0] is zero");
        for (int k = 0; k < 18; ++k) h.ba[b][k] = ba[b * 18 + k] / a0;    // SciPy normalises by a[0]
        for (int k = 0; k < ES_PRE_L; ++k) { h.tpl[b][k] = tpl[b * ES_PRE_L + k]; h.tpl32[b][k] = (float)tpl[b * ES_PRE_L + k]; }
        if (ntaps[b] < 1 || ntaps[b] > ES_MAX_TAPS) return fail(ctx, ES_EINVAL, "es_set_tables: ntaps out of range");
        h.ntaps[b] = ntaps[b];
        if (b == 0 || ntaps[b] > ctx->max_ntaps) ctx->max_ntaps = ntaps[b];
        for (int k = 0; k < ntaps[b]; ++k) h.taps[b][k] = taps[b * ES_MAX_TAPS + k];
        double e = 0.0;                                                     // c_b of include/echoseal_coherent.h: the taps in forward order
        for (int k = ntaps[b] - 1; k >= 0; --k) e = e + (double)h.taps[b][k] * (double)h.taps[b][k];
        ctx->mf_norm[b] = std::sqrt(191.0 * e);
    }
    uint16_t dpos[ES_POLAR_N];
    std::memset(dpos, 0, sizeof dpos);
    std::memset(&ctx->frozen, 0, sizeof ctx->frozen);
    int n = 0;
    for (int i = 0; i < ES_POLAR_N; ++i) {
        if (frozen[i]) ctx->frozen.w[i >> 5] |= (1u << (i & 31));
        else dpos[n++] = (uint16_t)i;
    }
    // 448 is the reference's own code (rtwm/polar_fast.py:8-9); its PolarCode class takes any K (rtwm/fastpolar.py:209-234), and so does
    // es_scl_batch (at least one information bit in front of the CRC-8).
    if (n < 9)
        return fail(ctx, ES_EINVAL, "es_set_tables: the frozen mask must leave K >= 9 information positions (448 for every entry point but es_scl_batch)");
    ctx->n_info = n;
    DeviceGuard g(ctx->device);
    ES_HIP_CHECK(ctx, hipMemcpy(ctx->d_tables, &h, sizeof h, hipMemcpyHostToDevice));
    ES_HIP_CHECK(ctx, hipMemcpy(ctx->d_data_pos, dpos, sizeof dpos, hipMemcpyHostToDevice));
    ctx->tables_ready = true;
    return ES_OK;
}

#define ES_REQUIRE_DEFAULT_CODE(ctx, who)                                                  \
    do {                                                                                   \
        if ((ctx)->n_info != ES_POLAR_K) return fail((ctx), ES_EINVAL, who ": this entry point serves the reference's own code only (448 information positions, 55-byte payloads)"); \
    } while (0)

#define ES_REQUIRE_READY(ctx)                                                              \
    do {                                                                                   \
        if (!(ctx)) return ES_EINVAL;                                                      \
        if (!(ctx)->tables_ready) return fail((ctx), ES_ENOTREADY, "es_set_tables has not been called"); \
    } while (0)

int es_bpf_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                 const uint8_t* band_dev, double* y_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_bpf_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_bpf_batch: dtype must be f32 or i16");
    if (B == 0 || T == 0) return ES_OK;
    if (!frames_dev || !band_dev || !y_dev) return fail(ctx, ES_EINVAL, "es_bpf_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_bpf(ctx, frames_dev, dtype, B, T, band_dev, y_dev, nullptr, (hipStream_t)stream);
}

int es_bpf2_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                  const uint8_t* band_dev, double* y_dev, float* y32_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_bpf2_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_bpf2_batch: dtype must be f32 or i16");
    if (B == 0 || T == 0) return ES_OK;
    if (!frames_dev || !band_dev || !y_dev || !y32_dev) return fail(ctx, ES_EINVAL, "es_bpf2_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_bpf(ctx, frames_dev, dtype, B, T, band_dev, y_dev, y32_dev, (hipStream_t)stream);
}

int es_xcorr32_batch(es_ctx* ctx, const float* y32_dev, int64_t B, int T, const uint8_t* band_dev,
                     float* corr32_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_xcorr32_batch: negative size");
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_xcorr32_batch: record shorter than the 63-chip template");
    if (B == 0) return ES_OK;
    if (!y32_dev || !band_dev || !corr32_dev) return fail(ctx, ES_EINVAL, "es_xcorr32_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_xcorr32(ctx, y32_dev, B, T, band_dev, corr32_dev, (hipStream_t)stream);
}

int es_pick_exact_batch(es_ctx* ctx, const float* corr32_dev, const double* y_dev, int64_t B, int T,
                        const uint8_t* band_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev,
                        uint8_t* flags_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_pick_exact_batch: negative size");
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_pick_exact_batch: record shorter than the 63-chip template");
    if (B == 0) return ES_OK;
    if (!corr32_dev || !y_dev || !band_dev || !thr_dev || !peaks_dev || !npeaks_dev || !flags_dev)
        return fail(ctx, ES_EINVAL, "es_pick_exact_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_pick_exact(ctx, corr32_dev, y_dev, B, T, band_dev, thr_dev, peaks_dev, npeaks_dev, flags_dev,
                                (hipStream_t)stream);
}

int es_sync_fused_batch(es_ctx* ctx, const float* y32_dev, const double* y_dev, int64_t B, int T,
                        const uint8_t* band_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev,
                        uint8_t* flags_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_sync_fused_batch: negative size");
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_sync_fused_batch: record shorter than the 63-chip template");
    if (B == 0) return ES_OK;
    if (!y32_dev || !y_dev || !band_dev || !thr_dev || !peaks_dev || !npeaks_dev || !flags_dev)
        return fail(ctx, ES_EINVAL, "es_sync_fused_batch: null pointer");
    DeviceGuard g(ctx->device);
    /* one launch: records the screen cannot settle are settled by the same wave from float64 re-evaluations (flags_dev
       then carries the reason code, for information) */
    return es_launch_sync_fused(ctx, y32_dev, y_dev, B, T, band_dev, thr_dev, peaks_dev, npeaks_dev, flags_dev, (hipStream_t)stream);
}

int es_front_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const uint8_t* band_dev,
                   const uint8_t* pn_dev, const int32_t* start_dev, double* y_dev, float* y32_dev, double* thr_dev,
                   int32_t* peaks_dev, int32_t* npeaks_dev, uint8_t* flags_dev, float* llr_dev, void* stream)
{
    /* es_bpf2_batch -> es_sync_fused_batch -> es_llr_batch (variant 0) in one call: the same three launches, one trip through the binding.
       Every argument is checked before the first launch, so a bad call enqueues nothing. */
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_front_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_front_batch: dtype must be f32 or i16");
    if (B == 0) return ES_OK;
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_front_batch: record shorter than the 63-chip template");
    if (!frames_dev || !band_dev || !pn_dev || !y_dev || !y32_dev || !thr_dev || !peaks_dev || !npeaks_dev || !flags_dev || !llr_dev)
        return fail(ctx, ES_EINVAL, "es_front_batch: null pointer");
    int rc = es_bpf2_batch(ctx, frames_dev, dtype, B, T, band_dev, y_dev, y32_dev, stream);
    if (rc != ES_OK) return rc;
    rc = es_sync_fused_batch(ctx, y32_dev, y_dev, B, T, band_dev, thr_dev, peaks_dev, npeaks_dev, flags_dev, stream);
    if (rc != ES_OK) return rc;
    return es_llr_batch(ctx, y_dev, B, T, start_dev, band_dev, pn_dev, 0, llr_dev, nullptr, nullptr, stream);
}

int es_front_peak_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const uint8_t* band_dev,
                        const uint8_t* pn_dev, double* y_dev, float* y32_dev, double* thr_dev, int32_t* peaks_dev,
                        int32_t* npeaks_dev, uint8_t* flags_dev, float* llr_dev, void* stream)
{
    /* es_bpf2_batch -> es_sync_fused_batch -> es_llr_at_batch at each record's first peak (peaks_dev[i * ES_MAX_PEAKS], -1 = none
       read as 0), variant 0.  Every argument is checked before the first launch, so a bad call enqueues nothing. */
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_front_peak_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_front_peak_batch: dtype must be f32 or i16");
    if (B == 0) return ES_OK;
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_front_peak_batch: record shorter than the 63-chip template");
    if (T - (ES_PRE_L - 1) > 4096) return fail(ctx, ES_EINVAL, "es_front_peak_batch: more than 4096 lags; use the float64 path");
    if (!frames_dev || !band_dev || !pn_dev || !y_dev || !y32_dev || !thr_dev || !peaks_dev || !npeaks_dev || !flags_dev || !llr_dev)
        return fail(ctx, ES_EINVAL, "es_front_peak_batch: null pointer");
    int rc = es_bpf2_batch(ctx, frames_dev, dtype, B, T, band_dev, y_dev, y32_dev, stream);
    if (rc != ES_OK) return rc;
    rc = es_sync_fused_batch(ctx, y32_dev, y_dev, B, T, band_dev, thr_dev, peaks_dev, npeaks_dev, flags_dev, stream);
    if (rc != ES_OK) return rc;
    return es_llr_at_batch(ctx, y_dev, B, T, B, nullptr, peaks_dev, ES_MAX_PEAKS, band_dev, pn_dev, 0, llr_dev, nullptr, nullptr, stream);
}

int es_reserve(es_ctx* ctx, int64_t B_max, int T_max)
{
    if (!ctx) return ES_EINVAL;
    if (B_max < 0 || T_max < 0) return fail(ctx, ES_EINVAL, "es_reserve: negative size");
    DeviceGuard g(ctx->device);
    const size_t need = (T_max >= ES_PRE_L) ? (size_t)B_max * (size_t)(T_max - (ES_PRE_L - 1)) * sizeof(double) : 0;
    if (need > ctx->ws_corr_bytes) {
        if (ctx->d_ws_corr) ES_HIP_CHECK(ctx, hipFree(ctx->d_ws_corr));
        ctx->d_ws_corr = nullptr; ctx->ws_corr_bytes = 0;
        if (hipMalloc(&ctx->d_ws_corr, need) != hipSuccess) return fail(ctx, ES_ENOMEM, "es_reserve: device allocation of the float64 correlation workspace failed");
        ctx->ws_corr_bytes = need;
    }
    return ES_OK;
}

int es_xcorr_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const uint8_t* band_dev,
                   double* corr_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_xcorr_batch: negative size");
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_xcorr_batch: record shorter than the 63-chip template");
    if (B == 0) return ES_OK;
    if (!y_dev || !band_dev || !corr_dev) return fail(ctx, ES_EINVAL, "es_xcorr_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_xcorr(ctx, y_dev, B, T, band_dev, corr_dev, (hipStream_t)stream);
}

int es_pick_batch(es_ctx* ctx, const double* corr_dev, int64_t B, int n_lags, double* thr_dev,
                  int32_t* peaks_dev, int32_t* npeaks_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || n_lags < 1) return fail(ctx, ES_EINVAL, "es_pick_batch: bad size");
    if (B == 0) return ES_OK;
    if (!corr_dev || !thr_dev || !peaks_dev || !npeaks_dev) return fail(ctx, ES_EINVAL, "es_pick_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_pick(ctx, corr_dev, B, n_lags, thr_dev, peaks_dev, npeaks_dev, (hipStream_t)stream);
}

int es_sync_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                  const uint8_t* band_dev, double* y_dev, double* corr_dev, double* thr_dev,
                  int32_t* peaks_dev, int32_t* npeaks_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_sync_batch: record shorter than the 63-chip template");
    if (B <= 0) return B == 0 ? ES_OK : fail(ctx, ES_EINVAL, "es_sync_batch: negative batch");
    DeviceGuard g(ctx->device);
    const int n_lags = T - (ES_PRE_L - 1);
    double* corr = corr_dev;
    if (!corr) {                                          // workspace grows monotonically; never freed in-call
        const size_t need = (size_t)B * n_lags * sizeof(double);
        if (need > ctx->ws_corr_bytes) { const int rc0 = es_reserve(ctx, B, T); if (rc0) return rc0; }
        corr = ctx->d_ws_corr;
    }
    int rc = es_bpf_batch(ctx, frames_dev, dtype, B, T, band_dev, y_dev, stream);
    if (rc) return rc;
    rc = es_xcorr_batch(ctx, y_dev, B, T, band_dev, corr, stream);
    if (rc) return rc;
    return es_pick_batch(ctx, corr, B, n_lags, thr_dev, peaks_dev, npeaks_dev, stream);
}

int es_sync_ragged_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const int32_t* len_dev,
                         const uint8_t* band_dev, double* y_dev, double* corr_dev, double* thr_dev,
                         int32_t* peaks_dev, int32_t* npeaks_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (T < ES_PRE_L) return fail(ctx, ES_EINVAL, "es_sync_ragged_batch: rows shorter than the 63-chip template");
    if (B <= 0) return B == 0 ? ES_OK : fail(ctx, ES_EINVAL, "es_sync_ragged_batch: negative batch");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_sync_ragged_batch: dtype must be f32 or i16");
    if (!frames_dev || !len_dev || !band_dev || !y_dev || !thr_dev || !peaks_dev || !npeaks_dev)
        return fail(ctx, ES_EINVAL, "es_sync_ragged_batch: null pointer");
    DeviceGuard g(ctx->device);
    double* corr = corr_dev;
    if (!corr) {                                          // the workspace of es_sync_batch, sized for rows of T
        const size_t need = (size_t)B * (T - (ES_PRE_L - 1)) * sizeof(double);
        if (need > ctx->ws_corr_bytes) { const int rc0 = es_reserve(ctx, B, T); if (rc0) return rc0; }
        corr = ctx->d_ws_corr;
    }
    // the band-pass runs every stored row to T: it is causal with zero initial state, so y[i][0 : len[i]] is the record's own output
    // whatever the padding holds; correlation and pick then stop at each record's end
    int rc = es_launch_bpf(ctx, frames_dev, dtype, B, T, band_dev, y_dev, nullptr, (hipStream_t)stream);
    if (rc) return rc;
    rc = es_launch_xcorr_ragged(ctx, y_dev, B, T, len_dev, band_dev, corr, (hipStream_t)stream);
    if (rc) return rc;
    return es_launch_pick_ragged(ctx, corr, B, T, len_dev, thr_dev, peaks_dev, npeaks_dev, (hipStream_t)stream);
}

int es_llr_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const int32_t* start_dev,
                 const uint8_t* band_dev, const uint8_t* pn_dev, int variant, float* llr_dev,
                 int32_t* best_s_dev, float* score_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_llr_batch: negative size");
    if (variant != 0 && variant != 1) return fail(ctx, ES_EINVAL, "es_llr_batch: variant must be 0 or 1");
    if (B == 0) return ES_OK;
    if (!y_dev || !band_dev || !pn_dev || !llr_dev) return fail(ctx, ES_EINVAL, "es_llr_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_llr(ctx, y_dev, B, T, start_dev, {nullptr, 0, 1}, band_dev, pn_dev, variant, llr_dev, best_s_dev,
                         score_dev, (hipStream_t)stream);
}

int es_header_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const int32_t* start_dev,
                    const uint8_t* band_dev, const uint8_t* hdr_pn_dev, uint8_t* ok_dev, int32_t* val_dev,
                    float* score_dev, int32_t* best_s_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_header_batch: negative size");
    if (B == 0) return ES_OK;
    if (!y_dev || !band_dev || !hdr_pn_dev || !ok_dev || !val_dev || !score_dev)
        return fail(ctx, ES_EINVAL, "es_header_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_header(ctx, y_dev, B, T, start_dev, {nullptr, 0, 1}, band_dev, hdr_pn_dev, ok_dev, val_dev, score_dev,
                            best_s_dev, (hipStream_t)stream);
}

int es_llr_at_batch(es_ctx* ctx, const double* y_dev, int64_t n_rows, int T, int64_t B, const int32_t* row_dev,
                    const int32_t* start_dev, int start_stride, const uint8_t* band_dev, const uint8_t* pn_dev, int variant,
                    float* llr_dev, int32_t* best_s_dev, float* score_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0 || n_rows < 0) return fail(ctx, ES_EINVAL, "es_llr_at_batch: negative size");
    if (start_stride < 1) return fail(ctx, ES_EINVAL, "es_llr_at_batch: start_stride must be >= 1");
    if (variant != 0 && variant != 1) return fail(ctx, ES_EINVAL, "es_llr_at_batch: variant must be 0 or 1");
    if (B == 0) return ES_OK;
    if (n_rows < 1) return fail(ctx, ES_EINVAL, "es_llr_at_batch: no rows to read");
    if (!y_dev || !band_dev || !pn_dev || !llr_dev) return fail(ctx, ES_EINVAL, "es_llr_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_llr(ctx, y_dev, B, T, start_dev, {row_dev, n_rows, start_stride}, band_dev, pn_dev, variant, llr_dev,
                         best_s_dev, score_dev, (hipStream_t)stream);
}

int es_header_at_batch(es_ctx* ctx, const double* y_dev, int64_t n_rows, int T, int64_t B, const int32_t* row_dev,
                       const int32_t* start_dev, int start_stride, const uint8_t* band_dev, const uint8_t* hdr_pn_dev,
                       uint8_t* ok_dev, int32_t* val_dev, float* score_dev, int32_t* best_s_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || T < 0 || n_rows < 0) return fail(ctx, ES_EINVAL, "es_header_at_batch: negative size");
    if (start_stride < 1) return fail(ctx, ES_EINVAL, "es_header_at_batch: start_stride must be >= 1");
    if (B == 0) return ES_OK;
    if (n_rows < 1) return fail(ctx, ES_EINVAL, "es_header_at_batch: no rows to read");
    if (!y_dev || !band_dev || !hdr_pn_dev || !ok_dev || !val_dev || !score_dev)
        return fail(ctx, ES_EINVAL, "es_header_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_header(ctx, y_dev, B, T, start_dev, {row_dev, n_rows, start_stride}, band_dev, hdr_pn_dev, ok_dev, val_dev,
                            score_dev, best_s_dev, (hipStream_t)stream);
}

int es_scl_batch(es_ctx* ctx, const void* llr_dev, int dtype, int64_t B, int list_size,
                 int skip_if_hard_ok, uint8_t* hard_info_dev, uint8_t* hard_ok_dev,
                 uint8_t* cand_info_dev, double* cand_metric_dev, uint8_t* cand_ok_dev,
                 int32_t* ncand_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_scl_batch: negative batch");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_F64) return fail(ctx, ES_EINVAL, "es_scl_batch: dtype must be f32 or f64");
    if (ctx->list_size_max == 0) return fail(ctx, ES_EINVAL, "es_scl_batch: this is a front-end context (es_create with list_size_max = 0): it has no list-decoder scratch");
    if (list_size < 1 || list_size > ctx->list_size_max)
        return fail(ctx, ES_EINVAL, "es_scl_batch: list_size must be in [1, list_size_max]");
    if (B == 0) return ES_OK;
    if (!llr_dev || !hard_info_dev || !hard_ok_dev || !cand_info_dev || !cand_metric_dev || !cand_ok_dev || !ncand_dev)
        return fail(ctx, ES_EINVAL, "es_scl_batch: null pointer");
    DeviceGuard g(ctx->device);
    const es_scl_io io{llr_dev, dtype, B, list_size, skip_if_hard_ok, hard_info_dev, hard_ok_dev, cand_info_dev, cand_metric_dev, cand_ok_dev, ncand_dev};
    const hipStream_t st = (hipStream_t)stream;
    if (ctx->n_info != ES_POLAR_K && !ctx->d_wide_scratch)
        return fail(ctx, ES_EINVAL, "es_scl_batch: a code other than K = 448 runs on the lane-per-path kernel only, and this context has no scratch for it (list_size_max <= 32 and scl_lanes 1 never requested before es_reserve)");
    if (list_size > 32 || ctx->n_info != ES_POLAR_K)
        return es_launch_scl_wide(ctx, io, st);
    const int lp = es_list_cap(list_size);                    // the kernels are built for powers of two; any size runs on the next one
    // Which mapping?  Measured on one MI355X (tools/mapping_sweep.py, round 3; milliseconds per launch at L = 8):
    //      B        one frame per wave   4 lanes per path   2 lanes per path   1 lane per path
    //    2 048            1.68                 2.02               2.89              3.46
    //    4 096            3.29                 2.58               3.01              3.72
    //    8 192            6.54                 4.77               4.09              4.03
    //   16 384           13.13                 8.19               8.14              6.46
    //   65 536           52.39                30.13              27.04             21.73
    // One lane per path (es_scl_wide.hip: fewest instructions per frame, but a wave carries 64/L frames through the whole decode) wins
    // once the batch yields about one such wave per SIMD -- earlier for long lists, never for L = 1; it needs that kernel's slab
    // (list_size_max > 32, or es_set_option "scl_lane_slab").
    const long long wide_waves = (long long)B * lp / 64;
    const long long wide_min = (lp <= 8 ? 1024LL : lp == 16 ? 768LL : 256LL) * ctx->num_cu / 256;      // (L = 2: 4.3 against 4.6 ms at 32 768 frames, 6.9 against 8.1 at 65 536)
    const bool lane_auto = ctx->scl_lanes == 0 && ctx->scl_multi < 0 && ctx->d_wide_scratch && lp >= 2 && wide_waves >= wide_min;
    if ((ctx->scl_lanes == 1 && ctx->scl_multi != 0) || lane_auto)
        return es_launch_scl_wide(ctx, io, st);
    if (lp <= 32) {
        // Several frames per wave (es_scl_multi.hip, 16/L frames per wave at four lanes per path) against one frame per wave: the
        // break-even is ~3 000 frames for L <= 8 (1.5 of the former's waves per SIMD at L = 8), ~1 500 frames for L = 16, ~512 for L = 32
        // (where both map one frame to a wave and the multi-frame kernel's smaller footprint -- three waves per SIMD, non-persistent
        // blocks -- wins as soon as the batch exceeds one wave per SIMD).
        const bool fits = lp <= 8 ? B >= 12LL * ctx->num_cu : B >= (lp == 16 ? 6LL : 2LL) * ctx->num_cu + (lp == 32);
        const bool multi = ctx->scl_multi == 1 || (ctx->scl_multi < 0 && fits);
        if (multi) return es_launch_scl_multi(ctx, io, st);
    }
    return es_launch_scl(ctx, io, st);
}

int es_schedule_batch(es_ctx* ctx, const uint8_t* aes_key16_host, const uint8_t* band_key32_host, const uint32_t* ctr_dev,
                      uint32_t ctr0, int64_t n, uint8_t* pn_rows_dev, uint8_t* band_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0) return fail(ctx, ES_EINVAL, "es_schedule_batch: negative count");
    if (n == 0) return ES_OK;
    if (!aes_key16_host || !band_key32_host || !pn_rows_dev || !band_dev) return fail(ctx, ES_EINVAL, "es_schedule_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_schedule(ctx, aes_key16_host, band_key32_host, ctr_dev, ctr0, n, pn_rows_dev, band_dev, (hipStream_t)stream);
}

int es_tx_frames_batch(es_ctx* ctx, const uint8_t* code_dev, const uint8_t* pn_rows_dev, const uint8_t* band_dev,
                       const uint32_t* ctr_dev, const uint8_t* preamble8_host, const uint8_t* hdr_pn16_host, int64_t B,
                       double* y_ws_dev, float* frames_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0) return fail(ctx, ES_EINVAL, "es_tx_frames_batch: negative batch");
    if (B == 0) return ES_OK;
    if (!code_dev || !pn_rows_dev || !band_dev || !ctr_dev || !preamble8_host || !hdr_pn16_host || !y_ws_dev || !frames_dev)
        return fail(ctx, ES_EINVAL, "es_tx_frames_batch: null pointer");
    unsigned long long pre = 0;
    for (int i = 0; i < 8; ++i) pre = (pre << 8) | preamble8_host[i];      // 63 MLS bits, MSB first, in the top 63 bits
    DeviceGuard g(ctx->device);
    return es_launch_tx_frames(ctx, code_dev, pn_rows_dev, band_dev, ctr_dev, pre, hdr_pn16_host, B, y_ws_dev, frames_dev,
                               (hipStream_t)stream);
}

int es_mix_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n, int block, const float* chips_dev, int64_t chips_stride,
                 const int64_t* chip_off_dev, double alpha, double floor, float* out_dev, double* scale_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;                        /* no tables involved: any context serves it, a front-end one included */
    if (block < 1) return fail(ctx, ES_EINVAL, "es_mix_batch: block must be >= 1");
    if (R < 0 || n < 0 || chips_stride < 0) return fail(ctx, ES_EINVAL, "es_mix_batch: negative size");
    if (R == 0 || n == 0) return ES_OK;
    if (!x_dev || !chips_dev || !out_dev) return fail(ctx, ES_EINVAL, "es_mix_batch: null pointer");
    if (out_dev != x_dev && out_dev < x_dev + R * n && x_dev < out_dev + R * n)
        return fail(ctx, ES_EINVAL, "es_mix_batch: out_dev partly overlaps x_dev (only out_dev == x_dev may alias)");
    if (chips_stride < 1 || (!chip_off_dev && chips_stride < n))
        return fail(ctx, ES_EINVAL, "es_mix_batch: a chip row is shorter than the recording (chips_stride < n at offset 0)");
    DeviceGuard g(ctx->device);
    return es_launch_mix(ctx, x_dev, R, n, block, chips_dev, chips_stride, chip_off_dev, alpha, floor, out_dev, scale_dev, (hipStream_t)stream);
}

int es_mix_ragged_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n_stride, const int64_t* len_dev, int block,
                        const float* chips_dev, int64_t chips_total, const int64_t* chip_base_dev, const int64_t* chip_cnt_dev,
                        double alpha, double floor, float* out_dev, double* scale_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;                        /* no tables involved: any context serves it, a front-end one included */
    if (block < 1) return fail(ctx, ES_EINVAL, "es_mix_ragged_batch: block must be >= 1");
    if (R < 0 || n_stride < 0 || chips_total < 0) return fail(ctx, ES_EINVAL, "es_mix_ragged_batch: negative size");
    if (R == 0 || n_stride == 0) return ES_OK;
    if (!x_dev || !len_dev || !chips_dev || !chip_base_dev || !chip_cnt_dev || !out_dev)
        return fail(ctx, ES_EINVAL, "es_mix_ragged_batch: null pointer");
    if (out_dev != x_dev && out_dev < x_dev + R * n_stride && x_dev < out_dev + R * n_stride)
        return fail(ctx, ES_EINVAL, "es_mix_ragged_batch: out_dev partly overlaps x_dev (only out_dev == x_dev may alias)");
    if (chips_total == 0) return ES_OK;                /* no record has a chip: every record is of length 0 */
    DeviceGuard g(ctx->device);
    return es_launch_mix_ragged(ctx, {x_dev, R, n_stride, len_dev, block, chips_dev, chips_total, chip_base_dev, chip_cnt_dev, alpha, floor,
                                      out_dev, scale_dev}, (hipStream_t)stream);
}

namespace {
/* The records of a stream launch as the host laid them out, rec_host [R][ES_STREAM_REC_WORDS] = (sid, off, len, chip_base, chip_cnt): refused
 * here, before anything is enqueued, where the kernels could only clamp. */
int check_stream_records(es_ctx* ctx, const int64_t* rec, int64_t R, int64_t n_stride, int64_t S, int64_t chips_total)
{
    std::vector<uint8_t> seen((size_t)S, 0);
    for (int64_t r = 0; r < R; ++r) {
        const int64_t sid = rec[ES_STREAM_REC_WORDS * r], off = rec[ES_STREAM_REC_WORDS * r + 1], len = rec[ES_STREAM_REC_WORDS * r + 2];
        const int64_t base = rec[ES_STREAM_REC_WORDS * r + 3], cnt = rec[ES_STREAM_REC_WORDS * r + 4];
        if (sid < 0 || sid >= S) return fail(ctx, ES_EINVAL, "stream records: a sid outside the table");
        if (seen[(size_t)sid]) return fail(ctx, ES_EINVAL, "stream records: a stream named twice in one launch");
        seen[(size_t)sid] = 1;
        if (off < 0 || off >= ES_FRAME_LEN) return fail(ctx, ES_EINVAL, "stream records: off outside 0 .. 1214");
        if (len < 0 || len > n_stride) return fail(ctx, ES_EINVAL, "stream records: a length outside 0 .. n_stride");
        const int64_t end = (off > 0 ? off : ES_FRAME_LEN) + len;
        if (cnt != ((end + ES_FRAME_LEN - 1) / ES_FRAME_LEN - 1) * ES_FRAME_LEN)
            return fail(ctx, ES_EINVAL, "stream records: chip_cnt is not 1215 * the new frames the chunk needs");
        if (base < 0 || cnt > chips_total || base > chips_total - cnt)
            return fail(ctx, ES_EINVAL, "stream records: the pool is shorter than chip_base + chip_cnt");
    }
    return ES_OK;
}
}  // namespace

int es_mix_stream_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n_stride, const int64_t* len_dev, int block,
                        const int64_t* sid_dev, int64_t S, const float* tail_dev, const int64_t* off_dev, const float* chips_dev,
                        int64_t chips_total, const int64_t* chip_base_dev, const int64_t* chip_cnt_dev, const int64_t* rec_host,
                        double alpha, double floor, float* out_dev, double* scale_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (block < 1) return fail(ctx, ES_EINVAL, "es_mix_stream_batch: block must be >= 1");
    if (R < 0 || n_stride < 0 || chips_total < 0 || S < 0) return fail(ctx, ES_EINVAL, "es_mix_stream_batch: negative size");
    if (R == 0 || n_stride == 0) return ES_OK;
    if (!x_dev || !len_dev || !sid_dev || !tail_dev || !off_dev || !chip_base_dev || !chip_cnt_dev || !rec_host || !out_dev ||
        (!chips_dev && chips_total > 0))
        return fail(ctx, ES_EINVAL, "es_mix_stream_batch: null pointer");
    if (out_dev != x_dev && out_dev < x_dev + R * n_stride && x_dev < out_dev + R * n_stride)
        return fail(ctx, ES_EINVAL, "es_mix_stream_batch: out_dev partly overlaps x_dev (only out_dev == x_dev may alias)");
    const int rc = check_stream_records(ctx, rec_host, R, n_stride, S, chips_total);
    if (rc != ES_OK) return rc;
    DeviceGuard g(ctx->device);
    return es_launch_mix_stream(ctx, {x_dev, R, n_stride, len_dev, block, sid_dev, S, tail_dev, off_dev, chips_dev, chips_total, chip_base_dev,
                                      chip_cnt_dev, alpha, floor, out_dev, scale_dev}, (hipStream_t)stream);
}

int es_stream_commit_batch(es_ctx* ctx, int64_t R, int64_t n_stride, const int64_t* len_dev, const int64_t* sid_dev, int64_t S,
                           float* tail_dev, int64_t* ctr_dev, int64_t* off_dev, const float* chips_dev, int64_t chips_total,
                           const int64_t* chip_base_dev, const int64_t* chip_cnt_dev, const int64_t* rec_host, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (R < 0 || n_stride < 0 || chips_total < 0 || S < 0) return fail(ctx, ES_EINVAL, "es_stream_commit_batch: negative size");
    if (R == 0) return ES_OK;
    if (!len_dev || !sid_dev || !tail_dev || !ctr_dev || !off_dev || !chip_base_dev || !chip_cnt_dev || !rec_host || (!chips_dev && chips_total > 0))
        return fail(ctx, ES_EINVAL, "es_stream_commit_batch: null pointer");
    const int rc = check_stream_records(ctx, rec_host, R, n_stride, S, chips_total);
    if (rc != ES_OK) return rc;
    DeviceGuard g(ctx->device);
    return es_launch_stream_commit(ctx, {R, n_stride, len_dev, sid_dev, S, tail_dev, ctr_dev, off_dev, chips_dev, chips_total, chip_base_dev,
                                         chip_cnt_dev}, (hipStream_t)stream);
}

namespace {
/* The records of a monitor tick as the host laid them out, rec_host [R][ES_MONITOR_REC_WORDS] = (sid, len, col, move, base): refused here,
 * before anything is enqueued, where the kernels could only clamp.  -> ES_OK; *any_move: some row is moved down first; *nseg: the most
 * correlation segments a record's new lags touch (0: no record completes a lag). */
int check_monitor_records(es_ctx* ctx, const int64_t* rec, int64_t R, int64_t n_stride, int64_t S, int H, bool* any_move, int* nseg)
{
    const int64_t SEG = (int64_t)XC_SEG;
    std::vector<uint8_t> seen((size_t)S, 0);
    *any_move = false; *nseg = 0;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t* w = rec + ES_MONITOR_REC_WORDS * r;
        const int64_t sid = w[0], len = w[1], col = w[2], move = w[3], base = w[4];
        if (sid < 0 || sid >= S) return fail(ctx, ES_EINVAL, "monitor records: a sid outside the table");
        if (seen[(size_t)sid]) return fail(ctx, ES_EINVAL, "monitor records: a stream named twice in one launch");
        seen[(size_t)sid] = 1;
        if (len < 0 || len > n_stride) return fail(ctx, ES_EINVAL, "monitor records: a length outside 0 .. n_stride");
        if (col < 0 || col > H || len > H - col) return fail(ctx, ES_EINVAL, "monitor records: the chunk does not fit its history row");
        if (move < 0 || move % SEG || move > H - col) return fail(ctx, ES_EINVAL, "monitor records: move is not a multiple of 1216 inside the row");
        if (base < 0 || base % SEG) return fail(ctx, ES_EINVAL, "monitor records: base is not a multiple of 1216");
        if (move) *any_move = true;
        const int64_t first = col > ES_PRE_L - 1 ? col - (ES_PRE_L - 1) : 0, end = col + len - (ES_PRE_L - 1);
        if (end > first) {
            const int64_t n = (end + SEG - 1) / SEG - first / SEG;
            if (n > *nseg) *nseg = (int)n;
        }
    }
    return ES_OK;
}
}  // namespace

int es_bpf_stream_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t R, int64_t n_stride, const int64_t* sid_dev, const int64_t* len_dev,
                        const int64_t* col_dev, const int64_t* move_dev, const int64_t* base_dev, const int64_t* rec_host, int64_t S, int H,
                        const uint8_t* band_dev, double* z_dev, int64_t* pos_dev, double* y_hist_dev, double* corr_hist_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (R < 0 || n_stride < 0 || S < 0 || H < 0) return fail(ctx, ES_EINVAL, "es_bpf_stream_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_bpf_stream_batch: dtype must be f32 or i16");
    if (R == 0) return ES_OK;
    if (R > (int64_t)1 << 27) return fail(ctx, ES_EINVAL, "es_bpf_stream_batch: more than 2^27 records");
    if (!sid_dev || !len_dev || !col_dev || !move_dev || !base_dev || !rec_host || !band_dev || !z_dev || !pos_dev || !y_hist_dev || !corr_hist_dev ||
        (!x_dev && n_stride > 0))
        return fail(ctx, ES_EINVAL, "es_bpf_stream_batch: null pointer");
    bool any_move; int nseg;
    const int rc = check_monitor_records(ctx, rec_host, R, n_stride, S, H, &any_move, &nseg);
    if (rc != ES_OK) return rc;
    DeviceGuard g(ctx->device);
    return es_launch_bpf_stream(ctx, {R, n_stride, sid_dev, len_dev, col_dev, move_dev, base_dev, S, H, band_dev, z_dev, pos_dev, y_hist_dev,
                                      corr_hist_dev, any_move}, x_dev, dtype, (hipStream_t)stream);
}

int es_xcorr_stream_batch(es_ctx* ctx, const double* y_hist_dev, int64_t R, int64_t n_stride, const int64_t* sid_dev, const int64_t* len_dev,
                          const int64_t* col_dev, const int64_t* rec_host, int64_t S, int H, const uint8_t* band_dev, double* corr_hist_dev,
                          void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (R < 0 || n_stride < 0 || S < 0 || H < 0) return fail(ctx, ES_EINVAL, "es_xcorr_stream_batch: negative size");
    if (R == 0) return ES_OK;
    if (!y_hist_dev || !sid_dev || !len_dev || !col_dev || !rec_host || !band_dev || !corr_hist_dev)
        return fail(ctx, ES_EINVAL, "es_xcorr_stream_batch: null pointer");
    bool any_move; int nseg;
    const int rc = check_monitor_records(ctx, rec_host, R, n_stride, S, H, &any_move, &nseg);
    if (rc != ES_OK) return rc;
    if (nseg == 0) return ES_OK;                       /* no chunk completes a lag */
    DeviceGuard g(ctx->device);
    return es_launch_xcorr_stream(ctx, {R, n_stride, sid_dev, len_dev, col_dev, nullptr, nullptr, S, H, band_dev, nullptr, nullptr,
                                        const_cast<double*>(y_hist_dev), corr_hist_dev, false}, nseg, (hipStream_t)stream);
}

int es_pick_at_batch(es_ctx* ctx, const double* corr_dev, int64_t n_rows, int stride, int64_t B, const int32_t* row_dev, const int32_t* col_dev,
                     const int32_t* nlag_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || n_rows < 0 || stride < 0) return fail(ctx, ES_EINVAL, "es_pick_at_batch: negative size");
    if (B == 0) return ES_OK;
    if (n_rows < 1) return fail(ctx, ES_EINVAL, "es_pick_at_batch: no rows to read");
    if (!corr_dev || !col_dev || !nlag_dev || !thr_dev || !peaks_dev || !npeaks_dev) return fail(ctx, ES_EINVAL, "es_pick_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_pick_at(ctx, corr_dev, n_rows, stride, B, row_dev, col_dev, nlag_dev, thr_dev, peaks_dev, npeaks_dev, (hipStream_t)stream);
}

int es_tx_frames_keyed_batch(es_ctx* ctx, const uint8_t* code_dev, const uint8_t* pn_rows_dev, const uint8_t* band_dev,
                             const uint32_t* ctr_dev, const uint8_t* preamble8_host, const uint8_t* ring_dev, int64_t N,
                             const int32_t* key_dev, int64_t B, double* y_ws_dev, float* frames_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (B < 0 || N < 0) return fail(ctx, ES_EINVAL, "es_tx_frames_keyed_batch: negative count");
    if (B == 0) return ES_OK;
    if (N == 0) return fail(ctx, ES_EINVAL, "es_tx_frames_keyed_batch: frames but an empty key ring (every key index is outside [0, N))");
    if (!code_dev || !pn_rows_dev || !band_dev || !ctr_dev || !preamble8_host || !ring_dev || !key_dev || !y_ws_dev || !frames_dev)
        return fail(ctx, ES_EINVAL, "es_tx_frames_keyed_batch: null pointer");
    unsigned long long pre = 0;
    for (int i = 0; i < 8; ++i) pre = (pre << 8) | preamble8_host[i];      // 63 MLS bits, MSB first, in the top 63 bits
    DeviceGuard g(ctx->device);
    return es_launch_tx_frames_keyed(ctx, code_dev, pn_rows_dev, band_dev, ctr_dev, pre, ring_dev, N, key_dev, B, y_ws_dev, frames_dev,
                                     (hipStream_t)stream);
}

int es_resample_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t B, int64_t n_in, const void* h_tf_dev, int h_per_phase,
                      int up, int down, int64_t y0, int64_t n_out, void* out_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (B < 0 || n_in < 0 || n_out < 0) return fail(ctx, ES_EINVAL, "es_resample_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_F64) return fail(ctx, ES_EINVAL, "es_resample_batch: dtype must be f32 or f64");
    if (up < 1 || down < 1 || h_per_phase < 1 || y0 < 0) return fail(ctx, ES_EINVAL, "es_resample_batch: bad rate / filter geometry");
    if (B == 0 || n_out == 0) return ES_OK;
    if (!x_dev || !h_tf_dev || !out_dev) return fail(ctx, ES_EINVAL, "es_resample_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_resample(ctx, x_dev, dtype, B, n_in, h_tf_dev, h_per_phase, up, down, y0, n_out, out_dev, (hipStream_t)stream);
}

int es_resample_ragged_batch(es_ctx* ctx, const void* pool_dev, int dtype, int64_t pool_n, const void* filt_dev, int64_t filt_n,
                             const int64_t* desc_dev, int64_t R, int rep, float* out_dev, int64_t out_stride, int64_t max_out,
                             void* stream)
{
    if (!ctx) return ES_EINVAL;                        /* no tables involved: any context serves it, a front-end one included */
    if (rep < 1) return fail(ctx, ES_EINVAL, "es_resample_ragged_batch: rep must be >= 1");
    if (pool_n < 0 || filt_n < 0 || R < 0 || out_stride < 0 || max_out < 0) return fail(ctx, ES_EINVAL, "es_resample_ragged_batch: negative size");
    if (dtype != ES_DTYPE_I16 && dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_F64)
        return fail(ctx, ES_EINVAL, "es_resample_ragged_batch: dtype must be i16, f32 or f64");
    if (R == 0 || max_out == 0 || out_stride == 0) return ES_OK;
    if (!pool_dev || !filt_dev || !desc_dev || !out_dev) return fail(ctx, ES_EINVAL, "es_resample_ragged_batch: null pointer");
    if (max_out > out_stride) max_out = out_stride;    /* the kernel clamps every n_out to the row */
    if (R > (int64_t)0x7fffffff / ((max_out + ES_RESAMPLE_TILE - 1) / ES_RESAMPLE_TILE))
        return fail(ctx, ES_EINVAL, "es_resample_ragged_batch: more than 2^31 - 1 tiles in one launch");
    DeviceGuard g(ctx->device);
    return es_launch_resample_ragged(ctx, {pool_dev, dtype, pool_n, filt_dev, filt_n, desc_dev, R, rep, out_dev, out_stride, max_out},
                                     (hipStream_t)stream);
}

int es_resample_stream_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t R, int64_t n_stride, const int64_t* sid_dev,
                             const int64_t* len_dev, const int64_t* rec_host, int64_t S, const int64_t* rate_dev, const float* filt_dev,
                             int64_t filt_n, float* tail_dev, int64_t* nin_dev, float* out_dev, int64_t out_stride, void* stream)
{
    if (!ctx) return ES_EINVAL;                        /* no tables involved, as es_resample_ragged_batch */
    if (R < 0 || n_stride < 0 || S < 0 || filt_n < 0 || out_stride < 0) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: negative size");
    if (dtype != ES_DTYPE_F32 && dtype != ES_DTYPE_I16) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: dtype must be f32 or i16");
    if (R == 0) return ES_OK;
    if (R > (int64_t)1 << 20 || n_stride > (int64_t)1 << 30 || out_stride > (int64_t)1 << 30)
        return fail(ctx, ES_EINVAL, "es_resample_stream_batch: more than 2^20 records or rows of more than 2^30 samples");
    if (!sid_dev || !len_dev || !rec_host || !rate_dev || !tail_dev || !nin_dev || (!x_dev && n_stride > 0) || (!out_dev && out_stride > 0) ||
        (!filt_dev && filt_n > 0))
        return fail(ctx, ES_EINVAL, "es_resample_stream_batch: null pointer");
    std::vector<uint8_t> seen((size_t)S, 0);
    int64_t max_out = 0;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t* w = rec_host + ES_RSTREAM_REC_WORDS * r;
        const int64_t sid = w[0], len = w[1], n_old = w[2], f_old = w[3], cnt = w[4], up = w[5], down = w[6], y0 = w[7];
        if (sid < 0 || sid >= S) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: a sid outside the table");
        if (seen[(size_t)sid]) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: a stream named twice in one launch");
        seen[(size_t)sid] = 1;
        if (len < 0 || len > n_stride) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: a length outside 0 .. n_stride");
        if (up < 1 || down < 1 || up > ES_RESAMPLE_RATE_MAX || down > ES_RESAMPLE_RATE_MAX || y0 < 0 || y0 > ES_RSTREAM_Y0_MAX)
            return fail(ctx, ES_EINVAL, "es_resample_stream_batch: rate words outside their range");
        if (n_old < 0 || n_old > ((int64_t)1 << 62) / up - len)
            return fail(ctx, ES_EINVAL, "es_resample_stream_batch: a stream position whose n * up leaves 62 bits");
        const int64_t f0 = up == down ? n_old : es_rs_finalized(n_old, up, down, y0);
        const int64_t f1 = up == down ? n_old + len : es_rs_finalized(n_old + len, up, down, y0);
        if (f_old != f0 || cnt != f1 - f0) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: counts that disagree with the rate words");
        if (cnt > out_stride) return fail(ctx, ES_EINVAL, "es_resample_stream_batch: more outputs than an output row holds");
        if (cnt > max_out) max_out = cnt;
    }
    DeviceGuard g(ctx->device);
    return es_launch_resample_stream(ctx, {x_dev, dtype, R, n_stride, sid_dev, len_dev, S, rate_dev, filt_dev, filt_n, tail_dev, nin_dev, out_dev,
                                           out_stride, max_out}, (hipStream_t)stream);
}

int es_set_option(es_ctx* ctx, const char* name, int value)
{
    if (!ctx || !name) return ES_EINVAL;
    if (std::strcmp(name, "scl_multi") == 0) {
        if (value < -1 || value > 1) return fail(ctx, ES_EINVAL, "es_set_option: scl_multi takes -1 (auto), 0 or 1");
        ctx->scl_multi = value;
        return ES_OK;
    }
    if (std::strcmp(name, "scl_prio") == 0) {
        if (value < 0 || value > 3) return fail(ctx, ES_EINVAL, "es_set_option: scl_prio takes 0..3");
        ctx->scl_prio = value;
        return ES_OK;
    }
    if (std::strcmp(name, "scl_lanes") == 0 || std::strcmp(name, "scl_lane_slab") == 0) {
        const bool slab_only = std::strcmp(name, "scl_lane_slab") == 0;
        if (slab_only ? (value != 1) : (value != 0 && value != 1 && value != 2 && value != 4))
            return fail(ctx, ES_EINVAL, slab_only ? "es_set_option: scl_lane_slab takes 1" : "es_set_option: scl_lanes takes 0 (by batch size), 1, 2 or 4");
        if (value == 1 && !ctx->d_wide_scratch) {             // one lane per path: the slab of es_scl_wide.hip (allocated here, never in an enqueue call)
            DeviceGuard g(ctx->device);
            ctx->wide_enabled = true;
            ctx->wide_scratch_bytes = es_scl_wide_scratch_bytes(ctx, &ctx->wide_lanes);
            if (hipMalloc(&ctx->d_wide_scratch, ctx->wide_scratch_bytes) != hipSuccess) {
                ctx->d_wide_scratch = nullptr; ctx->wide_enabled = false;
                return fail(ctx, ES_ENOMEM, "es_set_option: device allocation of the lane-per-path scratch slab failed");
            }
        }
        if (!slab_only) ctx->scl_lanes = value;
        return ES_OK;
    }
    return fail(ctx, ES_EINVAL, "es_set_option: unknown option");
}

int es_polar_encode_batch(es_ctx* ctx, const uint8_t* info_dev, int64_t B, uint8_t* code_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    ES_REQUIRE_DEFAULT_CODE(ctx, "es_polar_encode_batch");
    if (B < 0) return fail(ctx, ES_EINVAL, "es_polar_encode_batch: negative batch");
    if (B == 0) return ES_OK;
    if (!info_dev || !code_dev) return fail(ctx, ES_EINVAL, "es_polar_encode_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_polar_encode(ctx, info_dev, B, code_dev, (hipStream_t)stream);
}

int es_softplus_batch(es_ctx* ctx, const double* t_dev, int64_t n, double* out_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0) return fail(ctx, ES_EINVAL, "es_softplus_batch: negative count");
    if (n == 0) return ES_OK;
    if (!t_dev || !out_dev) return fail(ctx, ES_EINVAL, "es_softplus_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_softplus(ctx, t_dev, n, out_dev, (hipStream_t)stream);
}

int es_polar_f_batch(es_ctx* ctx, const double* a_dev, const double* b_dev, int64_t n, double* out_dev, int32_t* bad_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0) return fail(ctx, ES_EINVAL, "es_polar_f_batch: negative count");
    if (n == 0) return ES_OK;
    if (!a_dev || !b_dev || !out_dev || !bad_dev) return fail(ctx, ES_EINVAL, "es_polar_f_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_polar_f_dev(ctx, a_dev, b_dev, n, out_dev, bad_dev, (hipStream_t)stream);
}

int es_aead_check_batch(es_ctx* ctx, const uint8_t* key32_host, const uint8_t* blobs_dev, int64_t n, int group,
                        const uint32_t* ctr_dev, uint8_t* ok_dev, uint8_t* plain_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (n < 0 || group < 1) return fail(ctx, ES_EINVAL, "es_aead_check_batch: negative count or group < 1");
    if (n == 0) return ES_OK;
    if (!key32_host || !blobs_dev || !ctr_dev || !ok_dev) return fail(ctx, ES_EINVAL, "es_aead_check_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_aead_check(ctx, key32_host, blobs_dev, n, group, ctr_dev, ok_dev, plain_dev, (hipStream_t)stream);
}

int es_aead_seal_batch(es_ctx* ctx, const uint8_t* key32_host, const uint8_t* nonces_dev, const uint8_t* plain_dev, int64_t n,
                       uint8_t* blobs_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0) return fail(ctx, ES_EINVAL, "es_aead_seal_batch: negative count");
    if (n == 0) return ES_OK;
    if (!key32_host || !nonces_dev || !plain_dev || !blobs_dev) return fail(ctx, ES_EINVAL, "es_aead_seal_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_aead_seal(ctx, key32_host, nonces_dev, plain_dev, n, blobs_dev, (hipStream_t)stream);
}

int es_select_batch(es_ctx* ctx, const uint8_t* key32_host, const uint32_t* ctr_dev, int64_t B, int L,
                    const uint8_t* hard_info_dev, const uint8_t* hard_ok_dev, const uint8_t* cand_info_dev,
                    const double* cand_metric_dev, const uint8_t* cand_ok_dev, const int32_t* ncand_dev,
                    uint8_t* payload_dev, int8_t* ok_dev, int32_t* which_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    ES_REQUIRE_DEFAULT_CODE(ctx, "es_select_batch");
    if (B < 0 || L < 1) return fail(ctx, ES_EINVAL, "es_select_batch: negative batch or list size < 1");
    if (B == 0) return ES_OK;
    if (!hard_info_dev || !hard_ok_dev || !cand_info_dev || !cand_metric_dev || !cand_ok_dev || !ncand_dev ||
        !payload_dev || !ok_dev || !which_dev) return fail(ctx, ES_EINVAL, "es_select_batch: null pointer");
    if (key32_host && !ctr_dev) return fail(ctx, ES_EINVAL, "es_select_batch: a key needs the expected counters");
    DeviceGuard g(ctx->device);
    return es_launch_select(ctx, key32_host, ctr_dev, B, L, hard_info_dev, hard_ok_dev, cand_info_dev, cand_metric_dev,
                            cand_ok_dev, ncand_dev, payload_dev, ok_dev, which_dev, (hipStream_t)stream);
}

int es_keyring_derive_batch(es_ctx* ctx, const uint8_t* master32_dev, int64_t N, uint8_t* ring_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (N < 0) return fail(ctx, ES_EINVAL, "es_keyring_derive_batch: negative count");
    if (N == 0) return ES_OK;
    if (!master32_dev || !ring_dev) return fail(ctx, ES_EINVAL, "es_keyring_derive_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_keyring_derive(ctx, master32_dev, N, ring_dev, (hipStream_t)stream);
}

int es_schedule_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint32_t* ctr_dev, int64_t n,
                            uint8_t* pn_rows_dev, uint8_t* band_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0 || N < 0) return fail(ctx, ES_EINVAL, "es_schedule_keyed_batch: negative count");
    if (n == 0 || (!pn_rows_dev && !band_dev)) return ES_OK;
    if (N == 0) return fail(ctx, ES_EINVAL, "es_schedule_keyed_batch: records but an empty key ring (every key index is outside [0, N))");
    if (!ring_dev || !key_dev || !ctr_dev) return fail(ctx, ES_EINVAL, "es_schedule_keyed_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_schedule_keyed(ctx, ring_dev, N, key_dev, ctr_dev, n, pn_rows_dev, band_dev, (hipStream_t)stream);
}

int es_aead_check_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* blobs_dev, int64_t n,
                              int group, const uint32_t* ctr_dev, uint8_t* ok_dev, uint8_t* plain_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (n < 0 || N < 0 || group < 1) return fail(ctx, ES_EINVAL, "es_aead_check_keyed_batch: negative count or group < 1");
    if (n == 0) return ES_OK;
    if (N == 0) return fail(ctx, ES_EINVAL, "es_aead_check_keyed_batch: records but an empty key ring");
    if (!ring_dev || !key_dev || !blobs_dev || !ctr_dev || !ok_dev) return fail(ctx, ES_EINVAL, "es_aead_check_keyed_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_aead_check_keyed(ctx, ring_dev, N, key_dev, blobs_dev, n, group, ctr_dev, ok_dev, plain_dev, (hipStream_t)stream);
}

int es_aead_seal_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* nonces_dev,
                             const uint8_t* plain_dev, int64_t n, uint8_t* blobs_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (n < 0 || N < 0) return fail(ctx, ES_EINVAL, "es_aead_seal_keyed_batch: negative count");
    if (n == 0) return ES_OK;
    if (N == 0) return fail(ctx, ES_EINVAL, "es_aead_seal_keyed_batch: records but an empty key ring (every key index is outside [0, N))");
    if (!ring_dev || !key_dev || !nonces_dev || !plain_dev || !blobs_dev) return fail(ctx, ES_EINVAL, "es_aead_seal_keyed_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_aead_seal_keyed(ctx, ring_dev, N, key_dev, nonces_dev, plain_dev, n, blobs_dev, (hipStream_t)stream);
}

int es_select_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint32_t* ctr_dev, int64_t B, int L,
                          const uint8_t* hard_info_dev, const uint8_t* hard_ok_dev, const uint8_t* cand_info_dev,
                          const double* cand_metric_dev, const uint8_t* cand_ok_dev, const int32_t* ncand_dev,
                          uint8_t* payload_dev, int8_t* ok_dev, int32_t* which_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    ES_REQUIRE_DEFAULT_CODE(ctx, "es_select_keyed_batch");
    if (B < 0 || N < 0 || L < 1) return fail(ctx, ES_EINVAL, "es_select_keyed_batch: negative count or list size < 1");
    if (B == 0) return ES_OK;
    if (N == 0) return fail(ctx, ES_EINVAL, "es_select_keyed_batch: records but an empty key ring");
    if (!ring_dev || !key_dev || !ctr_dev || !hard_info_dev || !hard_ok_dev || !cand_info_dev || !cand_metric_dev || !cand_ok_dev ||
        !ncand_dev || !payload_dev || !ok_dev || !which_dev) return fail(ctx, ES_EINVAL, "es_select_keyed_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_select_keyed(ctx, ring_dev, N, key_dev, ctr_dev, B, L, hard_info_dev, hard_ok_dev, cand_info_dev, cand_metric_dev,
                                  cand_ok_dev, ncand_dev, payload_dev, ok_dev, which_dev, (hipStream_t)stream);
}

int es_plan_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev, const int32_t* hdr_base_dev,
                  int64_t rows, int T, const uint8_t* hdr_ok_dev, const int32_t* hdr_lo16_dev, int64_t P, const uint8_t* hop_dev, int64_t N,
                  int C, uint8_t* cand_slot_dev, uint32_t* cand_ctr_dev, int32_t* count_dev, int32_t* looked_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (rows < 0 || N < 0 || P < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_plan_batch: negative size");
    if (rows == 0 || N == 0) return ES_OK;
    if (rows * N > ((int64_t)1 << 31)) return fail(ctx, ES_EINVAL, "es_plan_batch: more than 2^31 (key, row) pairs in one call");
    // the widest window ends at round((T - 1215) / 1215) + 200: the hop table must reach it
    if (C < (T + ES_FRAME_LEN - 1) / ES_FRAME_LEN + 201) return fail(ctx, ES_EINVAL, "es_plan_batch: hop table narrower than ceil(T / 1215) + 201 counters");
    if (!peaks_dev || !npeaks_dev || !rowband_dev || !hdr_base_dev || !hop_dev || !cand_slot_dev || !cand_ctr_dev || !count_dev ||
        (P > 0 && (!hdr_ok_dev || !hdr_lo16_dev))) return fail(ctx, ES_EINVAL, "es_plan_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_plan(ctx, peaks_dev, npeaks_dev, rowband_dev, hdr_base_dev, rows, T, hdr_ok_dev, hdr_lo16_dev, P, hop_dev, N, C,
                          cand_slot_dev, cand_ctr_dev, count_dev, looked_dev, (hipStream_t)stream);
}

int es_plan_ragged_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev,
                         const int32_t* hdr_base_dev, int64_t rows, const int32_t* len_dev, int T_max, const uint8_t* hdr_ok_dev,
                         const int32_t* hdr_lo16_dev, int64_t P, const uint8_t* hop_dev, int64_t N, int C, uint8_t* cand_slot_dev,
                         uint32_t* cand_ctr_dev, int32_t* count_dev, int32_t* looked_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (rows < 0 || N < 0 || P < 0 || T_max < 0) return fail(ctx, ES_EINVAL, "es_plan_ragged_batch: negative size");
    if (rows == 0 || N == 0) return ES_OK;
    if (rows * N > ((int64_t)1 << 31)) return fail(ctx, ES_EINVAL, "es_plan_ragged_batch: more than 2^31 (key, row) pairs in one call");
    // the widest window ends at round((T_max - 1215) / 1215) + 200: the hop table must reach it
    if (C < (T_max + ES_FRAME_LEN - 1) / ES_FRAME_LEN + 201) return fail(ctx, ES_EINVAL, "es_plan_ragged_batch: hop table narrower than ceil(T_max / 1215) + 201 counters");
    if (!peaks_dev || !npeaks_dev || !rowband_dev || !hdr_base_dev || !len_dev || !hop_dev || !cand_slot_dev || !cand_ctr_dev || !count_dev ||
        (P > 0 && (!hdr_ok_dev || !hdr_lo16_dev))) return fail(ctx, ES_EINVAL, "es_plan_ragged_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_plan_ragged(ctx, peaks_dev, npeaks_dev, rowband_dev, hdr_base_dev, rows, len_dev, hdr_ok_dev, hdr_lo16_dev, P, hop_dev,
                                 N, C, cand_slot_dev, cand_ctr_dev, count_dev, looked_dev, (hipStream_t)stream);
}

int es_plan_at_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev, const int32_t* hdr_base_dev,
                     int64_t rows, const int32_t* len_dev, int T_max, const uint8_t* hdr_ok_dev, const int32_t* hdr_lo16_dev, int64_t P,
                     const uint8_t* hop_dev, int64_t N, int C, const int64_t* pos0_dev, const uint32_t* ctr0_dev, const int32_t* hop_row_dev,
                     const uint32_t* hop_base_dev, int HR, uint8_t* cand_slot_dev, uint32_t* cand_ctr_dev, int32_t* count_dev,
                     int32_t* looked_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (rows < 0 || N < 0 || P < 0 || T_max < 0) return fail(ctx, ES_EINVAL, "es_plan_at_batch: negative size");
    if (rows == 0 || N == 0) return ES_OK;
    if (rows * N > ((int64_t)1 << 31)) return fail(ctx, ES_EINVAL, "es_plan_at_batch: more than 2^31 (key, row) pairs in one call");
    if (HR < 1) return fail(ctx, ES_EINVAL, "es_plan_at_batch: no hop row");
    // a hop row starts 200 counters before the estimate at the row's first sample and must reach 200 past the one at its last frame
    if (C < (T_max + ES_FRAME_LEN - 1) / ES_FRAME_LEN + 402) return fail(ctx, ES_EINVAL, "es_plan_at_batch: hop rows narrower than ceil(T_max / 1215) + 402 counters");
    if (!peaks_dev || !npeaks_dev || !rowband_dev || !hdr_base_dev || !len_dev || !hop_dev || !pos0_dev || !ctr0_dev || !hop_row_dev ||
        !hop_base_dev || !cand_slot_dev || !cand_ctr_dev || !count_dev || (P > 0 && (!hdr_ok_dev || !hdr_lo16_dev)))
        return fail(ctx, ES_EINVAL, "es_plan_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_plan_at(ctx, peaks_dev, npeaks_dev, rowband_dev, hdr_base_dev, rows, len_dev, hdr_ok_dev, hdr_lo16_dev, P, hop_dev, N, C,
                             pos0_dev, ctr0_dev, hop_row_dev, hop_base_dev, HR, cand_slot_dev, cand_ctr_dev, count_dev, looked_dev,
                             (hipStream_t)stream);
}

int es_hop_window_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const uint32_t* hop_base_dev, int64_t HR, int64_t C, uint8_t* hop_dev,
                        void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (N < 0 || HR < 0 || C < 0) return fail(ctx, ES_EINVAL, "es_hop_window_batch: negative count");
    if (N == 0 || HR == 0 || C == 0) return ES_OK;
    if (HR > ((int64_t)1 << 31) || C > ((int64_t)1 << 31) || N > ((int64_t)1 << 31) || N * HR > ((int64_t)1 << 40) / C)
        return fail(ctx, ES_EINVAL, "es_hop_window_batch: more than 2^40 (key, hop row, column) entries in one call");
    if (!ring_dev || !hop_base_dev || !hop_dev) return fail(ctx, ES_EINVAL, "es_hop_window_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_hop_window(ctx, ring_dev, N, hop_base_dev, HR, C, hop_dev, (hipStream_t)stream);
}

// ---- presence (include/echoseal_presence.h) ----
// what both presence calls refuse of the correlation rows
static const char* presence_rows(int64_t rows, int64_t stride, int64_t B)
{
    return (rows < 0 || stride < 0 || B < 0) ? ": negative count"
           : stride > 0x7FFFFFFFll ? ": stride above 2^31 - 1"
           : (B > ((int64_t)1 << 40) || rows / 4 < B) ? ": rows < 4 B" : nullptr;
}

int es_phase_fold_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                        double* fold_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_rows(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_phase_fold_batch") + why).c_str());
    if (B == 0) return ES_OK;
    if (B > 0x7FFFFFFFll / 5) return fail(ctx, ES_EINVAL, "es_phase_fold_batch: more than 2^31 - 1 blocks of five per clip in one call");
    if (!nlag_dev || !fold_dev || (!corr_dev && stride >= ES_FRAME_LEN)) return fail(ctx, ES_EINVAL, "es_phase_fold_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_phase_fold(ctx, corr_dev, stride, nlag_dev, B, fold_dev, (hipStream_t)stream);
}

int es_hop_score_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                       const int32_t* phase_dev, int P, const uint8_t* hop_dev, int64_t K, int64_t Ccols, int64_t n_origins,
                       double* score_dev, int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_rows(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_hop_score_batch") + why).c_str());
    if (K < 0 || Ccols < 0 || n_origins < 0) return fail(ctx, ES_EINVAL, "es_hop_score_batch: negative count");
    if (P < 1 || P > ES_FRAME_LEN) return fail(ctx, ES_EINVAL, "es_hop_score_batch: P must be in 1 .. 1215");
    const int64_t Jmax = stride / ES_FRAME_LEN, NB = n_origins / ES_HOP_ORIGINS + (n_origins % ES_HOP_ORIGINS != 0);
    if (Ccols < n_origins + Jmax - 1) return fail(ctx, ES_EINVAL, "es_hop_score_batch: Ccols < n_origins + Jmax - 1 (Jmax = stride / 1215)");
    if (B == 0 || K == 0) return ES_OK;
    if (K > 0x7FFFFFFFll / B || (NB > 0 && B * K > 0x7FFFFFFFll / NB))
        return fail(ctx, ES_EINVAL, "es_hop_score_batch: more than 2^31 - 1 blocks of (clip, key, 256 origins) in one call");
    const bool scored = NB > 0 && Jmax > 0;                                 // otherwise no block reads rows, phases or hop bytes
    if (!nlag_dev || !score_dev || !origin_dev || !rank_dev || (NB > 0 && (!scratch_dev || !phase_dev)) || (scored && (!corr_dev || !hop_dev)))
        return fail(ctx, ES_EINVAL, "es_hop_score_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_hop_score(ctx, corr_dev, stride, nlag_dev, B, phase_dev, P, hop_dev, K, Ccols, n_origins, score_dev, origin_dev, rank_dev,
                               scratch_dev, (hipStream_t)stream);
}

// ---- the coherent presence test (include/echoseal_coherent.h) ----
int es_mf_rows_batch(es_ctx* ctx, const double* y_dev, int64_t rows, int64_t T, const int32_t* len_dev, const uint8_t* band_dev,
                     double* m_dev, double* a_dev, double* d_dev, void* stream)
{
    ES_REQUIRE_READY(ctx);
    if (rows < 0 || T < 0) return fail(ctx, ES_EINVAL, "es_mf_rows_batch: negative count");
    if (T > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_mf_rows_batch: T above 2^31 - 1");
    if (rows == 0 || T == 0) return ES_OK;
    if (rows > 0x7FFFFFFFll / ((T + ES_MF_TILE - 1) / ES_MF_TILE))
        return fail(ctx, ES_EINVAL, "es_mf_rows_batch: more than 2^31 - 1 blocks of (record, 256 outputs) in one call");
    if (!y_dev || !len_dev || !band_dev || !m_dev || !a_dev || !d_dev) return fail(ctx, ES_EINVAL, "es_mf_rows_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_mf_rows(ctx, y_dev, rows, T, len_dev, band_dev, m_dev, a_dev, d_dev, (hipStream_t)stream);
}

int es_coherent_score_batch(es_ctx* ctx, const double* m_dev, const double* a_dev, const double* d_dev, int64_t rows, int64_t T,
                            const int32_t* nslot_dev, int64_t B, const int32_t* phase_dev, int P, const uint8_t* ring_dev,
                            const uint8_t* hop_dev, int64_t K, int64_t Ccols, uint32_t lo, int64_t n_origins, double* score_dev,
                            int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_rows(rows, T, B)) return fail(ctx, ES_EINVAL, (std::string("es_coherent_score_batch") + why).c_str());
    if (K < 0 || Ccols < 0 || n_origins < 0) return fail(ctx, ES_EINVAL, "es_coherent_score_batch: negative count");
    if (P < 1 || P > ES_FRAME_LEN) return fail(ctx, ES_EINVAL, "es_coherent_score_batch: P must be in 1 .. 1215");
    const int64_t Jmax = T > 190 ? (T - 190) / ES_FRAME_LEN : 0, NB = n_origins / ES_HOP_ORIGINS + (n_origins % ES_HOP_ORIGINS != 0);
    if (Ccols < n_origins + Jmax - 1)
        return fail(ctx, ES_EINVAL, "es_coherent_score_batch: Ccols < n_origins + Jmax - 1 (Jmax = max(0, T - 190) / 1215)");
    if (B == 0 || K == 0) return ES_OK;
    if (K > 0x7FFFFFFFll / B || (NB > 0 && B * K > 0x7FFFFFFFll / NB))
        return fail(ctx, ES_EINVAL, "es_coherent_score_batch: more than 2^31 - 1 blocks of (clip, key, 256 origins) in one call");
    const bool scored = NB > 0 && Jmax > 0;                                 // otherwise no block reads rows, phases, ring or hop bytes
    if (!nslot_dev || !score_dev || !origin_dev || !rank_dev || (NB > 0 && (!scratch_dev || !phase_dev || !ring_dev)) ||
        (scored && (!m_dev || !a_dev || !d_dev || !hop_dev)))
        return fail(ctx, ES_EINVAL, "es_coherent_score_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_coherent_score(ctx, m_dev, a_dev, d_dev, T, nslot_dev, B, phase_dev, P, ring_dev, hop_dev, K, Ccols, lo, n_origins, score_dev,
                                    origin_dev, rank_dev, scratch_dev, (hipStream_t)stream);
}

// ---- presence along a table of per-slot offsets (include/echoseal_warp.h) ----
int es_warp_fold_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                       const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev, int64_t D, int64_t Jw,
                       double* fold_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_rows(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_warp_fold_batch") + why).c_str());
    if (D < 0 || Jw < 0) return fail(ctx, ES_EINVAL, "es_warp_fold_batch: negative count");
    if (B == 0 || D == 0) return ES_OK;
    if (D > 0x7FFFFFFFll / 5 || B > 0x7FFFFFFFll / 5 / D)
        return fail(ctx, ES_EINVAL, "es_warp_fold_batch: more than 2^31 - 1 blocks of five per (clip, row) in one call");
    const bool read = Jw > 0 && stride >= ES_FRAME_LEN;                     // otherwise J == 0 everywhere: neither rows nor offsets are read
    if (!nlag_dev || !nwarp_dev || !nslot_dev || !fold_dev || (read && (!corr_dev || !warp_dev)))
        return fail(ctx, ES_EINVAL, "es_warp_fold_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_warp_fold(ctx, corr_dev, stride, nlag_dev, B, es_warp_tab{warp_dev, nwarp_dev, nslot_dev, D, Jw}, fold_dev, (hipStream_t)stream);
}

int es_warp_score_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                        const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev, int64_t D, int64_t Jw,
                        const int32_t* hyp_dev, int64_t H, const uint8_t* hop_dev, int64_t K, int64_t Ccols, int64_t n_origins,
                        double* score_dev, int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_rows(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_warp_score_batch") + why).c_str());
    if (D < 0 || Jw < 0 || K < 0 || Ccols < 0 || n_origins < 0) return fail(ctx, ES_EINVAL, "es_warp_score_batch: negative count");
    if (H < 1 || H > 0x7FFFFFFFll || D > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_warp_score_batch: H must be in 1 .. 2^31 - 1, D below 2^31");
    const int64_t NB = n_origins / ES_HOP_ORIGINS + (n_origins % ES_HOP_ORIGINS != 0);
    if (Ccols < n_origins + Jw - 1) return fail(ctx, ES_EINVAL, "es_warp_score_batch: Ccols < n_origins + Jw - 1");
    if (B == 0 || K == 0) return ES_OK;
    if (K > 0x7FFFFFFFll / B || (NB > 0 && B * K > 0x7FFFFFFFll / NB))
        return fail(ctx, ES_EINVAL, "es_warp_score_batch: more than 2^31 - 1 blocks of (clip, key, 256 origins) in one call");
    const bool scored = NB > 0 && Jw > 0 && stride >= ES_FRAME_LEN;             // otherwise J == 0 everywhere: no block reads rows, entries or hop bytes
    if (!nlag_dev || !score_dev || !origin_dev || !rank_dev || (NB > 0 && (!scratch_dev || !nslot_dev)) ||
        (scored && (!corr_dev || !nwarp_dev || !hyp_dev || !hop_dev || (D > 0 && !warp_dev))))
        return fail(ctx, ES_EINVAL, "es_warp_score_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_warp_score(ctx, corr_dev, stride, nlag_dev, B, es_warp_tab{warp_dev, nwarp_dev, nslot_dev, D, Jw}, hyp_dev, H, hop_dev, K, Ccols,
                                n_origins, score_dev, origin_dev, rank_dev, scratch_dev, (hipStream_t)stream);
}

// ---- presence over records anywhere in a table of rows (include/echoseal_live_presence.h) ----
// what both _at calls refuse of the table: no "four rows per record" here, records name their rows and may share them
static const char* presence_table(int64_t rows, int64_t stride, int64_t B)
{
    return (rows < 0 || stride < 0 || B < 0) ? ": negative count"
           : (stride > 0x7FFFFFFFll || rows > 0x7FFFFFFFll) ? ": rows or stride above 2^31 - 1"
           : B > ((int64_t)1 << 40) ? ": more than 2^40 records" : nullptr;
}

int es_warp_fold_at_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int64_t* row_dev, const int64_t* col_dev,
                          const int32_t* nlag_dev, int64_t B, const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev,
                          int64_t D, int64_t Jw, double* fold_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_table(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_warp_fold_at_batch") + why).c_str());
    if (D < 0 || Jw < 0) return fail(ctx, ES_EINVAL, "es_warp_fold_at_batch: negative count");
    if (B == 0 || D == 0) return ES_OK;
    if (D > 0x7FFFFFFFll / 5 || B > 0x7FFFFFFFll / 5 / D)
        return fail(ctx, ES_EINVAL, "es_warp_fold_at_batch: more than 2^31 - 1 blocks of five per (record, row) in one call");
    const bool read = Jw > 0 && rows > 0 && stride >= ES_FRAME_LEN;         // otherwise J == 0 everywhere: neither rows nor offsets are read
    if (!row_dev || !col_dev || !nlag_dev || !nwarp_dev || !nslot_dev || !fold_dev || (read && (!corr_dev || !warp_dev)))
        return fail(ctx, ES_EINVAL, "es_warp_fold_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_warp_fold_at(ctx, corr_dev, rows, stride, row_dev, col_dev, nlag_dev, B, es_warp_tab{warp_dev, nwarp_dev, nslot_dev, D, Jw},
                                  fold_dev, (hipStream_t)stream);
}

int es_warp_score_at_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int64_t* row_dev, const int64_t* col_dev,
                           const int32_t* nlag_dev, int64_t B, const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev,
                           int64_t D, int64_t Jw, const int32_t* hyp_dev, int64_t H, const uint8_t* hop_dev, int64_t K, int64_t HR,
                           int64_t Ccols, const int32_t* hop_row_dev, int64_t n_origins, double* score_dev, int64_t* origin_dev,
                           int32_t* rank_dev, void* scratch_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_table(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_warp_score_at_batch") + why).c_str());
    if (D < 0 || Jw < 0 || K < 0 || Ccols < 0 || n_origins < 0) return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: negative count");
    if (H < 1 || H > 0x7FFFFFFFll || D > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: H must be in 1 .. 2^31 - 1, D below 2^31");
    if (HR < 1 || HR > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: HR must be in 1 .. 2^31 - 1");
    const int64_t NB = n_origins / ES_HOP_ORIGINS + (n_origins % ES_HOP_ORIGINS != 0);
    if (Ccols < n_origins + Jw - 1) return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: Ccols < n_origins + Jw - 1");
    if (B == 0 || K == 0) return ES_OK;
    if (K > 0x7FFFFFFFll / B || (NB > 0 && B * K > 0x7FFFFFFFll / NB))
        return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: more than 2^31 - 1 blocks of (record, key, 256 origins) in one call");
    const bool scored = NB > 0 && Jw > 0 && rows > 0 && stride >= ES_FRAME_LEN; // otherwise J == 0 everywhere: no block reads rows, entries or hop bytes
    if (!score_dev || !origin_dev || !rank_dev ||
        (NB > 0 && (!scratch_dev || !row_dev || !col_dev || !nlag_dev || !nslot_dev || !hop_row_dev)) ||
        (scored && (!corr_dev || !nwarp_dev || !hyp_dev || !hop_dev || (D > 0 && !warp_dev))))
        return fail(ctx, ES_EINVAL, "es_warp_score_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_warp_score_at(ctx, corr_dev, rows, stride, row_dev, col_dev, nlag_dev, B, es_warp_tab{warp_dev, nwarp_dev, nslot_dev, D, Jw}, hyp_dev,
                                   H, hop_dev, K, HR, Ccols, hop_row_dev, n_origins, score_dev, origin_dev, rank_dev, scratch_dev, (hipStream_t)stream);
}

// ---- the coherent score over records anywhere in the three tables (include/echoseal_coherent_at.h) ----
int es_coherent_score_at_batch(es_ctx* ctx, const double* m_dev, const double* a_dev, const double* d_dev, int64_t rows, int64_t stride,
                               const int64_t* row_dev, const int64_t* col_dev, const int32_t* nslot_dev, int64_t B, int64_t Jw,
                               const int32_t* phase_dev, int P, const uint8_t* ring_dev, const uint8_t* hop_dev, int64_t K, int64_t HR,
                               int64_t Ccols, const int32_t* hop_row_dev, const uint32_t* lo_dev, int64_t n_origins, double* score_dev,
                               int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (const char* why = presence_table(rows, stride, B)) return fail(ctx, ES_EINVAL, (std::string("es_coherent_score_at_batch") + why).c_str());
    if (Jw < 0 || K < 0 || Ccols < 0 || n_origins < 0) return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: negative count");
    if (P < 1 || P > ES_FRAME_LEN) return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: P must be in 1 .. 1215");
    if (HR < 1 || HR > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: HR must be in 1 .. 2^31 - 1");
    const int64_t NB = n_origins / ES_HOP_ORIGINS + (n_origins % ES_HOP_ORIGINS != 0);
    if (Ccols - n_origins < Jw - 1)                                         // (the counts are >= 0 here: a difference cannot wrap, their sum could)
        return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: Ccols < n_origins + Jw - 1");
    if (B == 0 || K == 0) return ES_OK;
    if (K > 0x7FFFFFFFll / B || (NB > 0 && B * K > 0x7FFFFFFFll / NB))
        return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: more than 2^31 - 1 blocks of (record, key, 256 origins) in one call");
    const bool scored = NB > 0 && Jw > 0 && rows > 0 && stride >= ES_FRAME_LEN + 190;   // otherwise J == 0 everywhere: no block reads the tables or hop bytes
    if (!score_dev || !origin_dev || !rank_dev ||
        (NB > 0 && (!scratch_dev || !row_dev || !col_dev || !nslot_dev || !hop_row_dev || !lo_dev || !phase_dev || !ring_dev)) ||
        (scored && (!m_dev || !a_dev || !d_dev || !hop_dev)))
        return fail(ctx, ES_EINVAL, "es_coherent_score_at_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_coherent_score_at(ctx, m_dev, a_dev, d_dev, rows, stride, row_dev, col_dev, nslot_dev, B, Jw, phase_dev, P, ring_dev, hop_dev, K,
                                       HR, Ccols, hop_row_dev, lo_dev, n_origins, score_dev, origin_dev, rank_dev, scratch_dev, (hipStream_t)stream);
}

// ---- the hypothesis list picked on the device (include/echoseal_pick.h) ----
int es_fold_pick_batch(es_ctx* ctx, const double* fold_dev, int64_t B, int64_t D, const int32_t* nwarp_dev, int64_t H, int32_t* hyp_dev,
                       double* val_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (B < 0 || D < 0) return fail(ctx, ES_EINVAL, "es_fold_pick_batch: negative count");
    if (H < 1 || H > ES_PICK_MAX_H) return fail(ctx, ES_EINVAL, "es_fold_pick_batch: H must be in 1 .. ES_PICK_MAX_H");
    if (B > 0x7FFFFFFFll) return fail(ctx, ES_EINVAL, "es_fold_pick_batch: more than 2^31 - 1 records (a workgroup each) in one call");
    if (D > 0x7FFFFFFFll / ES_FRAME_LEN) return fail(ctx, ES_EINVAL, "es_fold_pick_batch: 1215 D above 2^31 - 1");
    if (B == 0 || D == 0) return ES_OK;
    if (!fold_dev || !hyp_dev) return fail(ctx, ES_EINVAL, "es_fold_pick_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_fold_pick(ctx, fold_dev, B, D, nwarp_dev, H, hyp_dev, val_dev, (hipStream_t)stream);
}

// What both acquisition calls refuse and when they have nothing to do: -> ES_EINVAL, ES_OK with *work = false, or ES_OK with *work = true
// and the exact grid of one wave per (record, tile of 64 high halves) within 2^31 - 1 blocks.
static int acquire_span(es_ctx* ctx, const char* who, int64_t P, int64_t ctr_lo, int64_t ctr_hi, bool* work)
{
    *work = false;
    const char* why = P < 0 ? ": negative count"
                      : (ctr_lo < 0 || ctr_hi > ((int64_t)1 << 32) || ctr_lo > ctr_hi) ? ": the span must lie in [0, 2^32] with ctr_lo <= ctr_hi" : nullptr;
    if (!why) {
        const int64_t H = ((ctr_hi + 65535) >> 16) - (ctr_lo >> 16), TW = ((H + 31) / 32 + 1) / 2;
        if (P == 0 || H == 0) return ES_OK;
        if (P > (((int64_t)1 << 33) - 4) / TW) why = ": more than 2^31 - 1 blocks of four (record, 64 high halves) tiles in one call";
    }
    if (why) {
        ctx->err = std::string(who) + why;
        return ES_EINVAL;
    }
    *work = true;
    return ES_OK;
}

int es_acquire_mask_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* ok_dev, const int32_t* lo16_dev,
                          const uint8_t* band_dev, int64_t P, int64_t ctr_lo, int64_t ctr_hi, uint32_t* mask_dev, int32_t* count_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (N < 0) return fail(ctx, ES_EINVAL, "es_acquire_mask_batch: negative count");
    bool work;
    if (acquire_span(ctx, "es_acquire_mask_batch", P, ctr_lo, ctr_hi, &work) != ES_OK) return ES_EINVAL;
    if (!work) return ES_OK;
    if (N < 1) return fail(ctx, ES_EINVAL, "es_acquire_mask_batch: records but an empty key ring");
    if (!ring_dev || !key_dev || !ok_dev || !lo16_dev || !band_dev || !mask_dev || !count_dev)
        return fail(ctx, ES_EINVAL, "es_acquire_mask_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_acquire_mask(ctx, ring_dev, N, key_dev, ok_dev, lo16_dev, band_dev, P, ctr_lo, ctr_hi, mask_dev, count_dev, (hipStream_t)stream);
}

int es_acquire_list_batch(es_ctx* ctx, const uint32_t* mask_dev, const int32_t* lo16_dev, int64_t P, int64_t ctr_lo, int64_t ctr_hi,
                          const int64_t* base_dev, int64_t total, int32_t* cand_rec_dev, uint32_t* cand_ctr_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (total < 0) return fail(ctx, ES_EINVAL, "es_acquire_list_batch: negative count");
    bool work;
    if (acquire_span(ctx, "es_acquire_list_batch", P, ctr_lo, ctr_hi, &work) != ES_OK) return ES_EINVAL;
    if (!work || total == 0) return ES_OK;
    if (!mask_dev || !lo16_dev || !base_dev || !cand_rec_dev || !cand_ctr_dev) return fail(ctx, ES_EINVAL, "es_acquire_list_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_acquire_list(ctx, mask_dev, lo16_dev, P, ctr_lo, ctr_hi, base_dev, total, cand_rec_dev, cand_ctr_dev, (hipStream_t)stream);
}

// what both memo calls refuse: a table that is not a power of two of entries, a count the uint32 claim words cannot index
static int memo_refusal(es_ctx* ctx, const char* who, int64_t slots, int64_t n)
{
    const char* why = (slots < 1 || (slots & (slots - 1)) != 0) ? ": slots must be a power of two, at least 1"
                      : (n < 0 || n >= (((int64_t)1 << 32) - 1)) ? ": n must be in [0, 2^32 - 1)" : nullptr;
    if (!why) return ES_OK;
    ctx->err = std::string(who) + why;
    return ES_EINVAL;
}

int es_memo_probe_batch(es_ctx* ctx, const uint64_t* table_dev, int64_t slots, const uint64_t* k0_dev, const uint64_t* k1_dev, int64_t n,
                        uint8_t* hit_dev, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (memo_refusal(ctx, "es_memo_probe_batch", slots, n) != ES_OK) return ES_EINVAL;
    if (n == 0) return ES_OK;
    if (!table_dev || !k0_dev || !k1_dev || !hit_dev) return fail(ctx, ES_EINVAL, "es_memo_probe_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_memo_probe(ctx, table_dev, slots, k0_dev, k1_dev, n, hit_dev, (hipStream_t)stream);
}

int es_memo_insert_batch(es_ctx* ctx, uint64_t* table_dev, uint32_t* claim_dev, int64_t slots, const uint64_t* k0_dev, const uint64_t* k1_dev,
                         int64_t n, void* stream)
{
    if (!ctx) return ES_EINVAL;
    if (memo_refusal(ctx, "es_memo_insert_batch", slots, n) != ES_OK) return ES_EINVAL;
    if (n == 0) return ES_OK;
    if (!table_dev || !claim_dev || !k0_dev || !k1_dev) return fail(ctx, ES_EINVAL, "es_memo_insert_batch: null pointer");
    DeviceGuard g(ctx->device);
    return es_launch_memo_insert(ctx, table_dev, claim_dev, slots, k0_dev, k1_dev, n, (hipStream_t)stream);
}

}  // extern "C"
