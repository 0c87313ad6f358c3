// es_memo.hip -- the verdict memo of live identification: a direct-mapped table of exact 128-bit records in HBM.
//
// An entry is two uint64 words (k0, k1), all ones when empty; record (k0, k1) lives at slot es_memo_slot(k0, k1, slots) or nowhere.
// Probe compares both words.  Insert is two kernels without a wait of any kind: es_memo_claim_kernel takes each contested slot for the
// lowest record index that maps to it (one atomic min on a uint32 claim word that rests at 0xFFFFFFFF), es_memo_write_kernel lets that
// record alone write both words and put the claim word back.  Two records of one call never write the same entry, so no entry is ever a
// mixture of two records, and the table after a call is a function of the table before it and the records (echoseal_amd/memo.py is
// that function on the host).  No kernel here loops on memory another thread writes.
#include "es_internal.h"

constexpr int MEMO_BLOCK = 256;

// record i of n, or -1: a thread per record
__device__ __forceinline__ long long memo_record(long long n)
{
    const long long i = (long long)blockIdx.x * MEMO_BLOCK + threadIdx.x;
    return i < n ? i : -1;
}

__global__ __launch_bounds__(MEMO_BLOCK) void es_memo_probe_kernel(const ulonglong2* __restrict__ table, unsigned long long mask,
                                                                   const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1,
                                                                   long long n, uint8_t* __restrict__ hit)
{
    const long long i = memo_record(n);
    if (i < 0) return;
    const unsigned long long a = k0[i], b = k1[i];
    const ulonglong2 e = table[es_memo_mix(a, b) & mask];                 // one 16-byte load: slot <= mask < slots
    hit[i] = (uint8_t)(e.x == a && e.y == b);
}

__global__ __launch_bounds__(MEMO_BLOCK) void es_memo_claim_kernel(unsigned* __restrict__ claim, unsigned long long mask,
                                                                   const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1,
                                                                   long long n)
{
    const long long i = memo_record(n);
    if (i < 0) return;
    const unsigned long long a = k0[i];
    if (a == ES_MEMO_EMPTY) return;                                       // a masked record
    atomicMin(&claim[es_memo_mix(a, k1[i]) & mask], (unsigned)i);         // i < 2^32 - 1: never the resting value
}

__global__ __launch_bounds__(MEMO_BLOCK) void es_memo_write_kernel(ulonglong2* __restrict__ table, unsigned* __restrict__ claim, unsigned long long mask,
                                                                   const unsigned long long* __restrict__ k0, const unsigned long long* __restrict__ k1,
                                                                   long long n)
{
    const long long i = memo_record(n);
    if (i < 0) return;
    const unsigned long long a = k0[i], b = k1[i];
    if (a == ES_MEMO_EMPTY) return;
    const unsigned long long s = es_memo_mix(a, b) & mask;
    // the claim word holds the winner's index until the winner itself puts 0xFFFFFFFF back: a loser reads one or the other, never its own
    if (claim[s] != (unsigned)i) return;
    table[s] = make_ulonglong2(a, b);
    claim[s] = 0xFFFFFFFFu;
}

static unsigned memo_grid(int64_t n) { return (unsigned)((n + MEMO_BLOCK - 1) / MEMO_BLOCK); }     // n < 2^32: fewer than 2^24 blocks

int es_launch_memo_probe(es_ctx* ctx, const uint64_t* table, int64_t slots, const uint64_t* k0, const uint64_t* k1, int64_t n, uint8_t* hit,
                         hipStream_t st)
{
    return es_launch(ctx, es_memo_probe_kernel, memo_grid(n), MEMO_BLOCK, 0, st, (const ulonglong2*)table, (unsigned long long)(slots - 1),
                     (const unsigned long long*)k0, (const unsigned long long*)k1, (long long)n, hit);
}

int es_launch_memo_insert(es_ctx* ctx, uint64_t* table, uint32_t* claim, int64_t slots, const uint64_t* k0, const uint64_t* k1, int64_t n,
                          hipStream_t st)
{
    const unsigned long long mask = (unsigned long long)(slots - 1);
    const int rc = es_launch(ctx, es_memo_claim_kernel, memo_grid(n), MEMO_BLOCK, 0, st, (unsigned*)claim, mask, (const unsigned long long*)k0,
                             (const unsigned long long*)k1, (long long)n);
    if (rc != ES_OK) return rc;
    return es_launch(ctx, es_memo_write_kernel, memo_grid(n), MEMO_BLOCK, 0, st, (ulonglong2*)table, (unsigned*)claim, mask,
                     (const unsigned long long*)k0, (const unsigned long long*)k1, (long long)n);
}
