// es_wave.h -- small wave-level helpers shared by the kernel translation units (device code only): fences between the
// lanes of one wave, order-preserving integer images of floats for the radix selects, lane exchanges.
#ifndef ES_WAVE_H
#define ES_WAVE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// The lanes of a wave run in lock step, but the compiler and the memory pipeline must still be told that what one lane
// wrote to LDS (wave_fence_lds) or to LDS and global memory (wave_fence_global) is what another lane of the wave reads next.
__device__ __forceinline__ void wave_fence_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ void wave_fence_global()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// Monotone unsigned image of a float / double (x < y <=> key(x) < key(y), -0.0 below +0.0) and back: what the radix selects sort by.
__device__ __forceinline__ uint32_t f32_key(float x)
{
    uint32_t b; __builtin_memcpy(&b, &x, 4);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k)
{
    const uint32_t b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    float x; __builtin_memcpy(&x, &b, 4); return x;
}
__device__ __forceinline__ uint64_t f64_key(double x)
{
    uint64_t b; __builtin_memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double key_f64(uint64_t k)
{
    const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
    double x; __builtin_memcpy(&x, &b, 8); return x;
}

// number of set bits of a ballot mask below this lane
__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// lane l <-> lane l ^ S for a compile-time S, through DPP where the data-parallel primitives reach
// (S = 1, 2: quad_perm; S = 4, 8: a row shift each way and a select); otherwise ds_bpermute.
template <int S>
__device__ __forceinline__ int xor_lanes_b32(int v, int lane)
{
    if constexpr (S == 1) return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);        // quad_perm [1,0,3,2]
    else if constexpr (S == 2) return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    else if constexpr (S == 4 || S == 8) {
        const int up = __builtin_amdgcn_mov_dpp(v, 0x100 + S, 0xf, 0xf, true);             // row_shl:S  (lane l gets l+S)
        const int dn = __builtin_amdgcn_mov_dpp(v, 0x110 + S, 0xf, 0xf, true);             // row_shr:S  (lane l gets l-S)
        return (lane & S) ? dn : up;
    } else return __shfl_xor(v, S);
}
template <int S>
__device__ __forceinline__ float xor_lanes_f32(float x, int lane)
{
    int v; __builtin_memcpy(&v, &x, 4);
    const int r = xor_lanes_b32<S>(v, lane);
    float o; __builtin_memcpy(&o, &r, 4); return o;
}
template <int S>
__device__ __forceinline__ double xor_lanes_f64(double x, int lane)
{
    uint64_t u; __builtin_memcpy(&u, &x, 8);
    const uint32_t lo = (uint32_t)xor_lanes_b32<S>((int)(uint32_t)u, lane);
    const uint32_t hi = (uint32_t)xor_lanes_b32<S>((int)(uint32_t)(u >> 32), lane);
    u = ((uint64_t)hi << 32) | lo;
    double r; __builtin_memcpy(&r, &u, 8); return r;
}

}  // namespace
#endif
