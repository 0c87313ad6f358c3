/* es_hop_best.h -- the end every presence score kernel shares (es_keyring.hip, es_coherent_body.inc): what a lane, a block or a (clip, key)
 * pair has found so far, the total order over it, and the reduction of a block's ES_HOP_ORIGINS lanes into the caller's scratch, which
 * es_hop_best_kernel (es_keyring.hip; es_launch_hop_best) then reduces chunk by chunk. */
#ifndef ES_HOP_BEST_H
#define ES_HOP_BEST_H

#include "es_internal.h"

// `a` is replaced by `b` where b is scored and a is not, or b's score is larger, or equal at a lower origin (an origin is owned by one
// lane, which keeps its earliest list entry itself)
struct hs_best { double score; long long origin; int rank; };
__device__ __forceinline__ bool hs_better(const hs_best& b, const hs_best& a)
{
    return b.origin >= 0 && (a.origin < 0 || b.score > a.score || (b.score == a.score && b.origin < a.origin));
}

// the best of a block's 256 lanes, to slot blockIdx.x of the scratch arrays: the end of every score kernel
__device__ __forceinline__ void hs_block_best(hs_best* red, const hs_best& best, int tid, double* __restrict__ sc_score,
        long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    red[tid] = best;
    __syncthreads();
    #pragma unroll 1
    for (int w = ES_HOP_ORIGINS / 2; w > 0; w >>= 1) {                                     // a maximum under a total order: any shape gives the same winner
        if (tid < w && hs_better(red[tid + w], red[tid])) red[tid] = red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        sc_score[blockIdx.x] = red[0].score; sc_origin[blockIdx.x] = red[0].origin; sc_rank[blockIdx.x] = red[0].rank;
    }
}

// the caller's scratch as the three arrays of the blocks' bests, one slot per (clip, key, chunk)
struct hs_scratch {
    long long NB, pairs, slots;
    double* score; long long* origin; long long* rank;
    hs_scratch(void* scratch, int64_t B, int64_t K, int64_t n_origins)
        : NB((n_origins + ES_HOP_ORIGINS - 1) / ES_HOP_ORIGINS), pairs((long long)B * K), slots(pairs * NB), score((double*)scratch),
          origin((long long*)scratch + slots), rank((long long*)scratch + 2 * slots) {}
};
// the launch that reduces them (es_keyring.hip)
int es_launch_hop_best(es_ctx* ctx, const hs_scratch& sc, double* score, int64_t* origin, int32_t* rank, hipStream_t st);

#endif
