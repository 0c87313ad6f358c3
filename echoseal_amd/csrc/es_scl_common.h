// es_scl_common.h -- pieces shared by the list-decoder kernels (es_scl.hip: one frame per wave;
// es_scl_multi.hip: several frames per wave).
#ifndef ES_SCL_COMMON_H
#define ES_SCL_COMMON_H
#include "es_internal.h"
#include "es_math.h"
#include "es_wave.h"

namespace {

constexpr int N = ES_POLAR_N;
constexpr int NLEV = 10;
constexpr int KINFO = ES_POLAR_K;         // 448 data positions (440 info + 8 CRC)


struct SclArgs {
    unsigned long long* dbg;
    const void* llr; int is_f64; long long B;
    es_frozen_mask frozen;
    const uint16_t* data_pos;
    const uint64_t* exp_tab;
    double* scratch;
    unsigned* slot_bits; int n_slots, slot_words;   // multi-frame kernel: bitmap of slab slots (one per resident block)
    uint8_t* hard_info; uint8_t* hard_ok;
    uint8_t* cand_info; double* cand_metric; uint8_t* cand_ok; int32_t* ncand;
    int skip_if_hard_ok;
    int lsz;                                  // the caller's list size (<= the kernel's template capacity L): paths kept per sort, row stride of the outputs
};

// What every launch of es_scl.hip / es_scl_multi.hip passes alike; the launchers add their slab.
inline SclArgs scl_args(const es_ctx* ctx, const es_scl_io& io)
{
    SclArgs a{};
    a.llr = io.llr; a.is_f64 = (io.dtype == ES_DTYPE_F64); a.B = io.B;
    a.frozen = ctx->frozen; a.data_pos = ctx->d_data_pos; a.exp_tab = ctx->d_exp_tab;
    a.hard_info = io.hard_info; a.hard_ok = io.hard_ok; a.cand_info = io.cand_info;
    a.cand_metric = io.cand_metric; a.cand_ok = io.cand_ok; a.ncand = io.ncand;
    a.skip_if_hard_ok = io.skip_if_hard_ok;
    a.lsz = io.L;
    return a;
}

__device__ __forceinline__ uint64_t ptr_set(uint64_t p, int depth, int slot)
{
    const int sh = 6 * (depth - 1);
    return (p & ~(63ULL << sh)) | ((uint64_t)slot << sh);
}
__device__ __forceinline__ int ptr_get(uint64_t p, int depth) { return (int)((p >> (6 * (depth - 1))) & 63ULL); }

// S is a loop-unrolled constant at every call site, so the switch folds away.
__device__ __forceinline__ double xor_lanes_f64_sw(double x, int S, int lane)
{
    switch (S) {
        case 1: return xor_lanes_f64<1>(x, lane);
        case 2: return xor_lanes_f64<2>(x, lane);
        case 4: return xor_lanes_f64<4>(x, lane);
        case 8: return xor_lanes_f64<8>(x, lane);
        case 16: return xor_lanes_f64<16>(x, lane);
        default: return xor_lanes_f64<32>(x, lane);
    }
}

__device__ __forceinline__ uint8_t crc8_bytes(const uint8_t* b, int n)
{
    uint32_t reg = 0;
    for (int i = 0; i < n; ++i) {
        reg ^= b[i];
        #pragma unroll
        for (int k = 0; k < 8; ++k) reg = (reg & 0x80u) ? ((reg << 1) ^ 0x07u) & 0xffu : (reg << 1) & 0xffu;
    }
    return (uint8_t)reg;
}


}  // namespace
#endif
