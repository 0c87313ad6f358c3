/* es_internal.h -- private declarations shared by the HIP translation units. */
#ifndef ES_INTERNAL_H
#define ES_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include <utility>

#include "../../include/echoseal_hip.h"
#include "../../include/echoseal_presence.h"
#include "../../include/echoseal_warp.h"
#include "../../include/echoseal_live_presence.h"
#include "../../include/echoseal_pick.h"
#include "../../include/echoseal_coherent.h"
#include "../../include/echoseal_coherent_at.h"

/* global memory by its address space: what the integer kernels (es_aead.hip, es_keyring.hip) read and write through */
typedef __attribute__((address_space(1))) const uint8_t g_cu8;
typedef __attribute__((address_space(1))) const uint32_t g_cu32;
typedef __attribute__((address_space(1))) const int32_t g_ci32;
typedef __attribute__((address_space(1))) const long long g_ci64;
typedef __attribute__((address_space(1))) uint8_t g_u8;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) int32_t g_i32;

struct es_frozen_mask { uint32_t w[32]; };            /* bit i set = index i frozen */

struct es_band_tables {
    double ba[ES_NBANDS][18];                         /* b[0..8], a[0..8] (already divided by a0) */
    double tpl[ES_NBANDS][64];                        /* 63 taps + pad */
    float  taps[ES_NBANDS][ES_MAX_TAPS];
    float  tpl32[ES_NBANDS][64];                      /* template rounded to float32 (screening kernel) */
    int32_t ntaps[ES_NBANDS];
};

struct es_ctx {
    int device = 0;
    int list_size_max = 8;
    int num_cu = 256;
    bool tables_ready = false;
    std::string err;

    es_frozen_mask frozen{};
    int n_info = 0;
    int max_ntaps = 0;                /* longest matched filter of the tables (picks the demodulator's instantiation) */
    double mf_norm[ES_NBANDS] = {};   /* c_b of include/echoseal_coherent.h: sqrt(191 * sum of the band's squared taps), formed by es_set_tables */

    /* device-resident tables */
    es_band_tables* d_tables = nullptr;
    uint16_t* d_data_pos = nullptr;                   /* [448] ascending information indices */
    uint64_t* d_exp_tab = nullptr;                    /* [256] */
    /* scratch */
    double* d_scl_scratch = nullptr;  size_t scl_scratch_bytes = 0;
    unsigned* d_slot_bits = nullptr;  /* bitmap of the slab slots of es_scl_multi_kernel (one bit per resident block) */
    double* d_ws_corr = nullptr;      size_t ws_corr_bytes = 0;
    void*   d_wide_scratch = nullptr; size_t wide_scratch_bytes = 0; long long wide_lanes = 0;   /* lane-per-path list decoder (es_scl_wide.hip): list sizes 64..1024, and shorter lists with scl_lanes = 1; its slab in lanes */
    bool    wide_enabled = false;
    unsigned* d_wide_slot_bits = nullptr; int wide_slot_words = 0;   /* its slab slot bitmap (>= 128 words: a slot per one-wave block of the slab, 3 072 / 4 096 on 256 CUs) */
    uint8_t* d_sbox = nullptr;        /* AES S-box (es_schedule_batch and the key-ring entry points), filled by es_create ... */
    uint8_t h_sbox[256] = {};         /* ... from this host copy, which es_launch_schedule expands its round keys with */
    /* Who is using a scratch slab (es_slab_enter).  Domain 0 = d_scl_scratch (es_scl.hip, es_scl_multi.hip),
       domain 1 = d_wide_scratch (es_scl_wide.hip).  `shape`: how the launch cuts the slab into slots; launches of one shareable shape on
       several streams share the slab through its slot bitmap, anything else is ordered behind the outstanding launches. */
    struct slab_use {
        struct user { hipStream_t st; hipEvent_t done; int shape; bool shareable; };   /* a stream's LAST launch on this slab: recorded after it (es_slab_leave) */
        std::vector<user> users;
    };
    slab_use slab[2];
    int* d_cursors = nullptr;         /* frame counters of the lane-per-path list decoder's launches (skip_if_hard_ok): a ring, one per launch */
    unsigned cursor_next = 0;         /* eager launches rotate over the first ES_CURSOR_RING - ES_CURSOR_CAPTURED counters */
    unsigned cursor_captured = 0;     /* launches recorded into a stream capture keep a counter of their own for the life of the context (the graph may replay at any time) */
    bool pick_attr_set = false;       /* per-device kernel attributes already raised for this context's device */
    unsigned wide_attr_mask = 0;      /* bit per instantiation of the lane-per-path list decoder (list capacity 1 .. 1024, kind of code): es_scl_wide.hip wide_attr_bit */
    /* tuning (es_set_option) */
    int scl_lanes = 0;                /* lanes per path of the multi-frame list decoder: 4 (16 paths per wave), 2 (32 paths per wave), 0 = by batch size */
    int scl_prio = 0;                 /* wave priority of the lane-per-path list decoder's launches (0..3) */
    int scl_multi = -1;               /* several frames per wave for list sizes <= 8: -1 auto (large batches), 0 never, 1 always */
};

#define ES_HIP_CHECK(ctx, expr)                                                         \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);             \
            return ES_EHIP;                                                             \
        }                                                                               \
    } while (0)

#if defined(__HIPCC__)
/* Grid of a launch whose blocks stride over the items: a block per `per_block` items, at most `cap_blocks` (each launcher's own multiple of
 * num_cu, chosen for its kernel). */
static inline unsigned es_grid(long long items, long long per_block, long long cap_blocks)
{
    const long long blocks = (items + per_block - 1) / per_block;
    return (unsigned)(blocks < cap_blocks ? blocks : cap_blocks);
}
/* The one way a kernel is launched and a failed launch reported (ctx->err as ES_HIP_CHECK words it). */
template <typename... P, typename... A>
__attribute__((always_inline)) static inline int es_launch(es_ctx* ctx, void (*kernel)(P...), unsigned grid, unsigned block, size_t lds,
                                                            hipStream_t st, A&&... args)
{
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, std::forward<A>(args)...);
    ES_HIP_CHECK(ctx, hipGetLastError());
    return ES_OK;
}

/* Inclusive prefix sum over the 64 lanes of a wave on the data-parallel primitives (row_shr 1, 2, 4, 8 inside the rows of 16, then the two
 * row broadcasts): six dependent vector adds of a few cycles each, where six __shfl_up were six LDS-crossbar round trips (~100 cycles each).
 * Lanes without a source keep the `old` operand, 0. */
__device__ __forceinline__ uint32_t es_wave_incl_scan_u32(uint32_t x)
{
    int v = (int)x;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     /* row_shr:1 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     /* row_shr:2 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     /* row_shr:4 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     /* row_shr:8 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     /* row_bcast:15 into rows 1 and 3 */
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     /* row_bcast:31 into rows 2 and 3 */
    return (uint32_t)v;
}
/* value of lane `src` (wave-uniform) in every lane: v_readlane instead of a ds_bpermute round trip */
__device__ __forceinline__ int es_wave_read_lane(int v, int src) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src)); }
#endif

/* Tiling of the sync correlation, shared by the float64 kernel (es_sync.hip) and the float32 screen (es_sync32.hip): a wave covers a segment
 * of 64 lanes x XC_R consecutive lags (19 is odd: a lane stride of 19 words is free of LDS bank conflicts), a block is XC_WAVES waves. */
constexpr int XC_R = 19;
constexpr int XC_SEG = 64 * XC_R;                  /* lags per wave */
static_assert(XC_SEG == ES_XC_SEG, "include/echoseal_hip.h states the correlation segment for the host");
constexpr int XC_WAVES = 4;

/* kernels exist for power-of-two list sizes; a context created for list_size_max serves every size up to the next one */
static inline int es_list_cap(int lmax) { int c = 1; while (c < lmax) c <<= 1; return c; }

/* Slab ownership (es_api.hip): es_slab_enter before a launch that uses a scratch slab, es_slab_leave right after it (same arguments).
 * Launches on ONE stream are ordered by the stream.  Launches of one shareable shape (the kernels that claim slots from the slab's bitmap)
 * on several streams run concurrently.  A launch of another shape -- or of a kernel that indexes the slab by block -- is ordered behind the
 * last launch of every other user ON THE DEVICE (hipStreamWaitEvent on the event es_slab_leave recorded): the host never blocks, and no
 * stream handle is used after its owner may have destroyed it (the events belong to the context).  Inside a stream capture both are no-ops:
 * a captured graph orders its own nodes, and graphs of different slot geometry must not be replayed concurrently on one context (header). */
int es_slab_enter(es_ctx* ctx, int domain, int shape, bool shareable, hipStream_t st);
int es_slab_leave(es_ctx* ctx, int domain, int shape, bool shareable, hipStream_t st);

/* What a list-decoder launch reads and writes: es_scl_batch fills it once, after validation (L = the caller's list size). */
struct es_scl_io {
    const void* llr; int dtype; int64_t B; int L; int skip_if_hard_ok;
    uint8_t* hard_info; uint8_t* hard_ok; uint8_t* cand_info; double* cand_metric; uint8_t* cand_ok; int32_t* ncand;
};
/* Which row and sample record i of a demodulator / header launch reads.  {nullptr, 0, 1}: plain, row i from start[i].  n_rows >= 1
 * (the *_at entry points): row row[i] (NULL = i) of n_rows, from start[i * start_stride]. */
struct es_rec_at { const int32_t* row; int64_t n_rows; int start_stride; };

/* launchers implemented in the kernel translation units */
size_t es_scl_scratch_bytes(const es_ctx* ctx);
size_t es_scl_wide_scratch_bytes(const es_ctx* ctx, long long* lanes_out);
size_t es_scl_multi_scratch_bytes(const es_ctx* ctx);
#define ES_CURSOR_RING 1024
#define ES_CURSOR_CAPTURED 256                                   /* of them: set aside for launches recorded into stream captures (never reused) */
int es_cursor_next(es_ctx* ctx, hipStream_t st, int** cursor);   /* a frame counter for one launch on `st` (es_api.hip) */
int es_launch_scl_multi(es_ctx* ctx, const es_scl_io& io, hipStream_t st);
int es_launch_scl_wide(es_ctx* ctx, const es_scl_io& io, hipStream_t st);
int es_launch_scl_wide_large(es_ctx* ctx, const es_scl_io& io, hipStream_t st);   /* L = 257..1024 (es_scl_wide_large.hip) */
int es_launch_scl(es_ctx* ctx, const es_scl_io& io, hipStream_t st);
int es_launch_softplus(es_ctx* ctx, const double* t, int64_t n, double* out, hipStream_t st);
int es_launch_polar_f_dev(es_ctx* ctx, const double* a, const double* b, int64_t n, double* out, int* bad, hipStream_t st);
int es_launch_polar_encode(es_ctx* ctx, const uint8_t* info, int64_t B, uint8_t* code, hipStream_t st);
int es_launch_bpf(es_ctx* ctx, const void* frames, int dtype, int64_t B, int T, const uint8_t* band,
                  double* y, float* y32, hipStream_t st);
int es_launch_xcorr32(es_ctx* ctx, const float* y32, int64_t B, int T, const uint8_t* band, float* corr32, hipStream_t st);
int es_launch_pick_exact(es_ctx* ctx, const float* corr32, const double* y, int64_t B, int T, const uint8_t* band,
                         double* thr, int32_t* peaks, int32_t* npeaks, uint8_t* flags, hipStream_t st);
int es_launch_sync_fused(es_ctx* ctx, const float* y32, const double* y, int64_t B, int T, const uint8_t* band, double* thr,
                         int32_t* peaks, int32_t* npeaks, uint8_t* flags, hipStream_t st);
int es_launch_xcorr(es_ctx* ctx, const double* y, int64_t B, int T, const uint8_t* band, double* corr,
                    hipStream_t st);
int es_launch_pick(es_ctx* ctx, const double* corr, int64_t B, int n_lags, double* thr, int32_t* peaks,
                   int32_t* npeaks, hipStream_t st);
/* records of unequal length in rows of T: len [B] samples of each record, clamped to [0, T] on the device (es_sync.hip) */
int es_launch_xcorr_ragged(es_ctx* ctx, const double* y, int64_t B, int T, const int32_t* len, const uint8_t* band, double* corr,
                           hipStream_t st);
int es_launch_pick_ragged(es_ctx* ctx, const double* corr, int64_t B, int T, const int32_t* len, double* thr, int32_t* peaks,
                          int32_t* npeaks, hipStream_t st);
/* a tick of a live monitor (es_bpf_stream_batch, es_xcorr_stream_batch; es_sync.hip): record r continues stream sid[r] of a table of S
 * streams, history rows of H columns; move / base / z / pos / any_move are the band-pass call's alone */
struct es_monitor_args {
    int64_t R; int64_t n_stride; const int64_t* sid; const int64_t* len; const int64_t* col; const int64_t* move; const int64_t* base;
    int64_t S; int H; const uint8_t* band; double* z; int64_t* pos; double* y_hist; double* corr_hist; bool any_move;
};
int es_launch_bpf_stream(es_ctx* ctx, const es_monitor_args& a, const void* x, int dtype, hipStream_t st);
int es_launch_xcorr_stream(es_ctx* ctx, const es_monitor_args& a, int nseg, hipStream_t st);
/* windows read in place: record i = nlag[i] lags from column col[i] of row row[i] (NULL = i) of corr [n_rows][stride] (es_sync.hip) */
int es_launch_pick_at(es_ctx* ctx, const double* corr, int64_t n_rows, int stride, int64_t B, const int32_t* row, const int32_t* col,
                      const int32_t* nlag, double* thr, int32_t* peaks, int32_t* npeaks, hipStream_t st);
int es_launch_llr(es_ctx* ctx, const double* y, int64_t B, int T, const int32_t* start, const es_rec_at& at,
                  const uint8_t* band, const uint8_t* pn, int variant, float* llr, int32_t* best_s,
                  float* score, hipStream_t st);

int es_launch_tx_frames(es_ctx* ctx, const uint8_t* code, const uint8_t* pn_rows, const uint8_t* band, const uint32_t* ctr,
                        unsigned long long pre_bits, const uint8_t* hdr_pn16, int64_t B, double* y_ws, float* frames, hipStream_t st);
int es_launch_mix(es_ctx* ctx, const float* x, int64_t R, int64_t n, int block, const float* chips, int64_t chips_stride,
                  const int64_t* chip_off, double alpha, double floor_lin, float* out, double* scale_out, hipStream_t st);
/* records of unequal length in rows of n_stride, chips from one flat pool (es_mix_ragged_batch; es_mix.hip) */
struct es_mix_ragged_args {
    const float* x; int64_t R; int64_t n_stride; const int64_t* len; int block;
    const float* chips; int64_t chips_total; const int64_t* chip_base; const int64_t* chip_cnt;
    double alpha; double floor_lin; float* out; double* scale_out;
};
int es_launch_mix_ragged(es_ctx* ctx, const es_mix_ragged_args& a, hipStream_t st);
/* chunks of live streams: record r continues stream sid[r] of a table of S (tail [S][1215], off [S]); its new frames lie in the pool
 * (es_mix_stream_batch; es_mix.hip) */
struct es_mix_stream_args {
    const float* x; int64_t R; int64_t n_stride; const int64_t* len; int block;
    const int64_t* sid; int64_t S; const float* tail; const int64_t* off;
    const float* chips; int64_t chips_total; const int64_t* chip_base; const int64_t* chip_cnt;
    double alpha; double floor_lin; float* out; double* scale_out;
};
int es_launch_mix_stream(es_ctx* ctx, const es_mix_stream_args& a, hipStream_t st);
/* ... and the state of the pushed streams after that mix (es_stream_commit_batch; es_mix.hip) */
struct es_stream_commit_args {
    int64_t R; int64_t n_stride; const int64_t* len; const int64_t* sid; int64_t S; float* tail; int64_t* ctr; int64_t* off;
    const float* chips; int64_t chips_total; const int64_t* chip_base; const int64_t* chip_cnt;
};
int es_launch_stream_commit(es_ctx* ctx, const es_stream_commit_args& a, hipStream_t st);
/* es_launch_tx_frames with the header PN of frame f read from ring row key[f] (es_tx.hip) */
int es_launch_tx_frames_keyed(es_ctx* ctx, const uint8_t* code, const uint8_t* pn_rows, const uint8_t* band, const uint32_t* ctr,
                              unsigned long long pre_bits, const uint8_t* ring, int64_t N, const int32_t* key, int64_t B, double* y_ws,
                              float* frames, hipStream_t st);
int es_launch_resample(es_ctx* ctx, const void* x, int dtype, int64_t B, int64_t n_x, const void* h_tf, int hpp, int up, int down,
                       int64_t y0, int64_t n_out, void* out, hipStream_t st);
/* clips of unequal length and rate from one flat pool, filters from another, a descriptor per record (es_resample_ragged_batch; es_resample.hip) */
struct es_resample_ragged_args {
    const void* pool; int dtype; int64_t pool_n; const void* filt; int64_t filt_n; const int64_t* desc; int64_t R; int rep;
    float* out; int64_t out_stride; int64_t max_out;
};
int es_launch_resample_ragged(es_ctx* ctx, const es_resample_ragged_args& a, hipStream_t st);
/* chunks of live streams at their own rates: record r continues stream sid[r] of a table of S (rate [S][5], tail [S][256], nin [S]);
 * max_out: the most outputs a record finalizes, from the host records (es_resample_stream_batch; es_resample.hip) */
struct es_resample_stream_args {
    const void* x; int dtype; int64_t R; int64_t n_stride; const int64_t* sid; const int64_t* len; int64_t S; const int64_t* rate;
    const float* filt; int64_t filt_n; float* tail; int64_t* nin; float* out; int64_t out_stride; int64_t max_out;
};
int es_launch_resample_stream(es_ctx* ctx, const es_resample_stream_args& a, hipStream_t st);
/* F(n): the outputs of resample_poly(X[:n], up, down) that no later sample changes -- those whose newest input sample has arrived
 * (DESIGN 4.16); n * up < 2^62 is the caller's to hold */
__host__ __device__ static inline long long es_rs_finalized(long long n, long long up, long long down, long long y0)
{
    if (n <= 0) return 0;
    const long long f = (n * up - 1) / down - y0 + 1;
    return f > 0 ? f : 0;
}
int es_launch_schedule(es_ctx* ctx, const uint8_t* aes_key16, const uint8_t* band_key32, const uint32_t* ctr_dev,
                       uint32_t ctr0, int64_t n, uint8_t* pn_rows, uint8_t* band, hipStream_t st);
int es_launch_aead_seal(es_ctx* ctx, const uint8_t* key32, const uint8_t* nonces, const uint8_t* plain, int64_t n, uint8_t* blobs,
                        hipStream_t st);
int es_launch_aead_check(es_ctx* ctx, const uint8_t* key32, const uint8_t* blobs, int64_t n, int group, const uint32_t* ctr,
                         uint8_t* ok, uint8_t* plain, hipStream_t st);
int es_launch_select(es_ctx* ctx, const uint8_t* key32, const uint32_t* ctr, int64_t B, int L, const uint8_t* hard_info,
                     const uint8_t* hard_ok, const uint8_t* cand_info, const double* cand_metric, const uint8_t* cand_ok,
                     const int32_t* ncand, uint8_t* payload, int8_t* ok, int32_t* which, hipStream_t st);
/* many keys at once (es_keyring.hip, es_aead.hip): ring rows of ES_KEYRING_BYTES, key = ring row of each record */
void es_host_sbox(uint8_t sb[256]);                              /* the AES S-box, computed (es_sched.hip): es_create fills h_sbox / d_sbox with it */
int es_launch_keyring_derive(es_ctx* ctx, const uint8_t* master32, int64_t N, uint8_t* ring, hipStream_t st);
int es_launch_schedule_keyed(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint32_t* ctr, int64_t n,
                             uint8_t* pn_rows, uint8_t* band, hipStream_t st);
int es_launch_aead_check_keyed(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint8_t* blobs, int64_t n, int group,
                               const uint32_t* ctr, uint8_t* ok, uint8_t* plain, hipStream_t st);
int es_launch_aead_seal_keyed(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint8_t* nonces, const uint8_t* plain,
                              int64_t n, uint8_t* blobs, hipStream_t st);
int es_launch_select_keyed(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint32_t* ctr, int64_t B, int L,
                           const uint8_t* hard_info, const uint8_t* hard_ok, const uint8_t* cand_info, const double* cand_metric,
                           const uint8_t* cand_ok, const int32_t* ncand, uint8_t* payload, int8_t* ok, int32_t* which, hipStream_t st);
int es_launch_plan(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base,
                   int64_t rows, int T, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop, int64_t N, int C,
                   uint8_t* cand_slot, uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st);
int es_launch_plan_ragged(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base,
                          int64_t rows, const int32_t* len, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop,
                          int64_t N, int C, uint8_t* cand_slot, uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st);
int es_launch_plan_at(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base, int64_t rows,
                      const int32_t* len, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop, int64_t N, int C,
                      const int64_t* pos0, const uint32_t* ctr0, const int32_t* hop_row, const uint32_t* hop_base, int HR, uint8_t* cand_slot,
                      uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st);
int es_launch_hop_window(es_ctx* ctx, const uint8_t* ring, int64_t N, const uint32_t* hop_base, int64_t HR, int64_t C, uint8_t* hop,
                         hipStream_t st);
/* acquisition (es_keyring.hip): the span is checked by the entry points, 0 <= ctr_lo <= ctr_hi <= 2^32, and so is the grid */
int es_launch_acquire_mask(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint8_t* ok, const int32_t* lo16,
                           const uint8_t* band, int64_t P, int64_t ctr_lo, int64_t ctr_hi, uint32_t* mask, int32_t* count, hipStream_t st);
int es_launch_acquire_list(es_ctx* ctx, const uint32_t* mask, const int32_t* lo16, int64_t P, int64_t ctr_lo, int64_t ctr_hi, const int64_t* base,
                           int64_t total, int32_t* cand_rec, uint32_t* cand_ctr, hipStream_t st);
/* presence (es_keyring.hip; include/echoseal_presence.h): counts, the hop table's width and both grids are checked by the entry points */
int es_launch_phase_fold(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, double* fold, hipStream_t st);
int es_launch_hop_score(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const int32_t* phase, int P,
                        const uint8_t* hop, int64_t K, int64_t Ccols, int64_t n_origins, double* score, int64_t* origin, int32_t* rank,
                        void* scratch, hipStream_t st);
/* the same along a table of per-slot offsets (include/echoseal_warp.h): one struct for what both launches read of it */
struct es_warp_tab { const int32_t* warp; const int32_t* nwarp; const int32_t* nslot; long long D, Jw; };
int es_launch_warp_fold(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const es_warp_tab& tab, double* fold,
                        hipStream_t st);
int es_launch_warp_score(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const es_warp_tab& tab,
                         const int32_t* hyp, int64_t H, const uint8_t* hop, int64_t K, int64_t Ccols, int64_t n_origins, double* score,
                         int64_t* origin, int32_t* rank, void* scratch, hipStream_t st);
/* the same over records that lie anywhere in a table of rows (include/echoseal_live_presence.h) */
int es_launch_warp_fold_at(es_ctx* ctx, const double* corr, int64_t rows, int64_t stride, const int64_t* row, const int64_t* col, const int32_t* nlag,
                           int64_t B, const es_warp_tab& tab, double* fold, hipStream_t st);
int es_launch_warp_score_at(es_ctx* ctx, const double* corr, int64_t rows, int64_t stride, const int64_t* row, const int64_t* col, const int32_t* nlag,
                            int64_t B, const es_warp_tab& tab, const int32_t* hyp, int64_t H, const uint8_t* hop, int64_t K, int64_t HR, int64_t Ccols,
                            const int32_t* hop_row, int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st);
/* the hypothesis list picked on the device (es_keyring.hip; include/echoseal_pick.h): a workgroup per record, B checked by the entry point */
int es_launch_fold_pick(es_ctx* ctx, const double* fold, int64_t B, int64_t D, const int32_t* nwarp, int64_t H, int32_t* hyp, double* val, hipStream_t st);
/* the coherent presence test (es_coherent_body.inc; include/echoseal_coherent.h): counts and both grids are checked by the entry points */
int es_launch_mf_rows(es_ctx* ctx, const double* y, int64_t rows, int64_t T, const int32_t* len, const uint8_t* band, double* m, double* a,
                      double* d, hipStream_t st);
int es_launch_coherent_score(es_ctx* ctx, const double* m, const double* a, const double* d, int64_t T, const int32_t* nslot, int64_t B,
                             const int32_t* phase, int P, const uint8_t* ring, const uint8_t* hop, int64_t K, int64_t Ccols, uint32_t lo,
                             int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st);
/* the same over records that lie anywhere in the three tables (include/echoseal_coherent_at.h): the same device body */
int es_launch_coherent_score_at(es_ctx* ctx, const double* m, const double* a, const double* d, int64_t rows, int64_t stride, const int64_t* row,
                                const int64_t* col, const int32_t* nslot, int64_t B, int64_t Jw, const int32_t* phase, int P, const uint8_t* ring,
                                const uint8_t* hop, int64_t K, int64_t HR, int64_t Ccols, const int32_t* hop_row, const uint32_t* lo,
                                int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st);
int es_launch_header(es_ctx* ctx, const double* y, int64_t B, int T, const int32_t* start, const es_rec_at& at, const uint8_t* band,
                     const uint8_t* hdr_pn, uint8_t* ok, int32_t* val, float* score, int32_t* best_s, hipStream_t st);
/* the verdict memo (es_memo.hip).  The slot of record (k0, k1) in a table of `slots` entries is es_memo_mix(k0, k1) & (slots - 1): the
 * splitmix64 finaliser over k0 * 0x9E3779B97F4A7C15 + k1, as include/echoseal_hip.h states it (host twin: echoseal_amd/memo.py slot) */
__host__ __device__ static inline unsigned long long es_memo_mix(unsigned long long k0, unsigned long long k1)
{
    unsigned long long z = k0 * 0x9E3779B97F4A7C15ull + k1;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
int es_launch_memo_probe(es_ctx* ctx, const uint64_t* table, int64_t slots, const uint64_t* k0, const uint64_t* k1, int64_t n, uint8_t* hit,
                         hipStream_t st);
int es_launch_memo_insert(es_ctx* ctx, uint64_t* table, uint32_t* claim, int64_t slots, const uint64_t* k0, const uint64_t* k1, int64_t n,
                          hipStream_t st);

#endif
