// es_keyring.hip -- many keys at once: the key ring (everything the keyed kernels need of a 32-byte master key, derived on the
// device), the key / PN / hop schedule of (key, counter) records, and the counter-candidate planning of the detector's scan for
// every (key, clip, band).  Replaces, per key, SecureChannel.__init__ (rtwm/crypto.py:19-30: HKDF-SHA256), StreamPRNG.__init__
// (rtwm/utils.py:86-88: BLAKE2s), the host-side expansion of es_sched.hip, and _scan_band_multi_frame's candidate loop
// (rtwm/detector.py:105-142) -- also for rows that lie somewhere in a stream marked from any counter (es_plan_at_kernel: line 117 with the
// row's absolute position and the stream's counter origin), over hop windows filled here (es_hop_window_kernel: rtwm/utils.py:27-36).
// Where nobody knows the origin, the low-16 gate of lines 122-127 is taken over a span of the whole counter range instead of an estimate's
// window (es_acquire_mask_kernel, es_acquire_count_kernel, es_acquire_list_kernel).
//
// Last, the presence test, which reads the same hop rows: the keyless fold of a clip's correlation rows over the 1215-sample frame grid and
// the score of every (key, counter origin, phase) against them (es_phase_fold_kernel, es_hop_score_kernel), and both again
// on a grid that follows clock drift, a table of per-slot offsets (es_warp_fold_kernel, es_warp_score_kernel), and those two
// over records that lie anywhere in a table of rows, such as the windows of live streams in a monitor's history (es_warp_fold_at_kernel,
// es_warp_score_at_kernel) -- the only float64 work in this file, every sum in one lane from its first slot to its last --
// and the pick of the hypothesis list from a fold (es_fold_pick_kernel), which compares float64 values as integers.
//
// Integer work otherwise.  Ring and schedule: one lane per key / per record, the S-box in LDS, round keys and hash states in
// registers (every index a constant after unrolling: no private memory).  Plan: one wave per (key, row), peaks serially, the
// counter window across the lanes, order kept by ballot + count of lower lanes.  Global memory is reached through
// address_space(1) pointers only.
#include "es_internal.h"
#include "es_crypto_dev.h"
#include "es_wave.h"
#include "es_hop_best.h"

namespace {

// ring row, in 32-bit words (include/echoseal_hip.h): AEAD key | AES round keys | HMAC inner state | HMAC outer state | header PN | hop0
constexpr int RW_AEAD = 0, RW_RK = 8, RW_IPAD = 52, RW_OPAD = 60, RW_HDR = 68, RW_HOP0 = 72, RW_WORDS = ES_KEYRING_BYTES / 4;
static_assert(RW_WORDS == 76 && ES_KEYRING_BYTES % 16 == 0, "ring row layout");

__device__ __forceinline__ void load_sbox(uint8_t* sbox, const uint8_t* sbox_g)
{
    sbox[threadIdx.x] = ((g_cu8*)sbox_g)[threadIdx.x];
    __syncthreads();
}

// states after the 64-byte HMAC pad blocks of a key of eight big-endian words
__device__ __forceinline__ void hmac256_pads(const uint32_t key[8], uint32_t ipad[8], uint32_t opad[8])
{
    uint32_t w[16];
    #pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = 0x36363636u ^ (t < 8 ? key[t] : 0u);
    #pragma unroll
    for (int t = 0; t < 8; ++t) ipad[t] = c_IV256[t];
    sha256_compress(ipad, w);
    #pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = 0x5c5c5c5cu ^ (t < 8 ? key[t] : 0u);
    #pragma unroll
    for (int t = 0; t < 8; ++t) opad[t] = c_IV256[t];
    sha256_compress(opad, w);
}

__global__ __launch_bounds__(256) void es_keyring_derive_kernel(const uint8_t* __restrict__ master_p, long long N,
        const uint8_t* __restrict__ sbox_g, uint8_t* __restrict__ ring_p)
{
    __shared__ uint8_t sbox[256];
    load_sbox(sbox, sbox_g);
    es_lds_cu8* sb = (es_lds_cu8*)sbox;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < N; k += stride) {
        g_cu8* mk = (g_cu8*)master_p + k * 32;
        g_u32* row = (g_u32*)(ring_p + k * ES_KEYRING_BYTES);
        uint32_t master[8];
        #pragma unroll
        for (int t = 0; t < 8; ++t)
            master[t] = ((uint32_t)mk[4 * t] << 24) | ((uint32_t)mk[4 * t + 1] << 16) | ((uint32_t)mk[4 * t + 2] << 8) | mk[4 * t + 3];
        uint32_t ip[8], op[8], w[16], prk[8], t1[8], t2[8];
        // HKDF-Extract: PRK = HMAC(salt = 32 zero bytes, master)
        #pragma unroll
        for (int t = 0; t < 8; ++t) prk[t] = 0;
        hmac256_pads(prk, ip, op);
        #pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = master[t];
        hmac256_short(ip, op, w, 8, prk);
        // HKDF-Expand: T1 = HMAC(PRK, info | 01), T2 = HMAC(PRK, T1 | info | 02); info = "EchoSeal:KDF:v1" (15 bytes)
        hmac256_pads(prk, ip, op);
        w[0] = 0x4563686fu; w[1] = 0x5365616cu; w[2] = 0x3a4b4446u; w[3] = 0x3a763101u;
        hmac256_short(ip, op, w, 4, t1);
        #pragma unroll
        for (int t = 0; t < 8; ++t) w[t] = t1[t];
        w[8] = 0x4563686fu; w[9] = 0x5365616cu; w[10] = 0x3a4b4446u; w[11] = 0x3a763102u;
        hmac256_short(ip, op, w, 12, t2);
        #pragma unroll
        for (int t = 0; t < 8; ++t) row[RW_AEAD + t] = __builtin_bswap32(t1[t]);        // ChaCha20 reads its key as little-endian words
        // AES sub-key = BLAKE2s-128(PRNG seed = T2, person "EchoSeal"), then the 44 round-key words
        uint32_t seed[8], sub[4], rk[44];
        #pragma unroll
        for (int t = 0; t < 8; ++t) seed[t] = __builtin_bswap32(t2[t]);
        blake2s_sub_key(seed, sub);
        #pragma unroll
        for (int t = 0; t < 4; ++t) rk[t] = __builtin_bswap32(sub[t]);
        aes128_expand(rk, sb);
        #pragma unroll
        for (int t = 0; t < 44; ++t) row[RW_RK + t] = rk[t];
        // hop key = the master key itself: HMAC pad states, and the band of counter 0
        hmac256_pads(master, ip, op);
        #pragma unroll
        for (int t = 0; t < 8; ++t) { row[RW_IPAD + t] = ip[t]; row[RW_OPAD + t] = op[t]; }
        w[0] = 0;
        hmac256_short(ip, op, w, 1, t1);
        // header PN = the first AES block of counter 0, bytes in stream order
        uint32_t s[4] = {0u, 0u, 0u, 0u};
        aes128_encrypt<10>(rk, sb, s);
        #pragma unroll
        for (int c = 0; c < 4; ++c) row[RW_HDR + c] = __builtin_bswap32(s[c]);
        row[RW_HOP0] = (t1[0] >> 24) & 3u;
        row[RW_HOP0 + 1] = 0; row[RW_HOP0 + 2] = 0; row[RW_HOP0 + 3] = 0;
    }
}

// b = band index of counter ctr under the hop key of ring row `row`: HMAC-SHA256(master, ctr_be32)[0] % 4 from the row's pad states.
// The one statement of it, for es_schedule_keyed_kernel and es_hop_window_kernel.  A macro and not a device function: the compiler
// orders the sums of the two compressions by where their operands are defined in the function it simplifies first, and through any
// wrapper function, however thin, es_schedule_keyed_kernel came out with a dozen instructions in another order (tools/asm_diff.sh).
#define ES_HOP_BAND(b, row, ctr)                                                                                                      \
    do {                                                                                                                              \
        uint32_t ip[8], op[8], w[16], tag[8];                                                                                         \
        _Pragma("unroll")                                                                                                             \
        for (int t = 0; t < 8; ++t) { ip[t] = (row)[RW_IPAD + t]; op[t] = (row)[RW_OPAD + t]; }                                       \
        w[0] = (ctr);                                                                 /* message = ctr_be32 */                        \
        hmac256_short(ip, op, w, 1, tag);                                                                                             \
        (b) = (tag[0] >> 24) & 3u;                                                    /* tag[0] % 4 */                                \
    } while (0)

// es_schedule_kernel (es_sched.hip) with the key material of record i read from ring row key[i]
__global__ __launch_bounds__(256) void es_schedule_keyed_kernel(const uint8_t* __restrict__ ring_p, long long N,
        const int32_t* __restrict__ key_p, const uint32_t* __restrict__ ctr_p, long long n, const uint8_t* __restrict__ sbox_g,
        uint8_t* __restrict__ pn_p, uint8_t* __restrict__ band_p)
{
    __shared__ uint8_t sbox[256];
    load_sbox(sbox, sbox_g);
    es_lds_cu8* sb = (es_lds_cu8*)sbox;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long key = ((g_ci32*)key_p)[i];
        const uint32_t ctr = ((g_cu32*)ctr_p)[i];
        const bool have = key >= 0 && key < N;
        g_cu32* row = (g_cu32*)(ring_p + (have ? key : 0) * ES_KEYRING_BYTES);
        if (pn_p) {
            g_u32* out = (g_u32*)(pn_p + i * ES_PN_BYTES);                            // 152-byte rows are 8-byte aligned
            if (have) {
                uint32_t rk[44];                                                      // once per record, not once per block
                #pragma unroll
                for (int t = 0; t < 44; ++t) rk[t] = row[RW_RK + t];
                #pragma unroll 1
                for (int j = 0; j < 10; ++j) {
                    uint32_t s[4] = {0u, ctr, 0u, (uint32_t)j};                       // (ctr << 64 | j), big endian
                    aes128_encrypt<10>(rk, sb, s);
                    out[4 * j] = __builtin_bswap32(s[0]); out[4 * j + 1] = __builtin_bswap32(s[1]);
                    if (j < 9) { out[4 * j + 2] = __builtin_bswap32(s[2]); out[4 * j + 3] = __builtin_bswap32(s[3]); }   // 152 = 9 * 16 + 8
                }
            } else {
                #pragma unroll 1
                for (int t = 0; t < ES_PN_BYTES / 4; ++t) out[t] = 0;
            }
        }
        if (band_p) {
            uint32_t b = 0;
            if (have) ES_HOP_BAND(b, row, ctr);
            ((g_u8*)band_p)[i] = (uint8_t)b;
        }
    }
}

// The hop windows of es_plan_at_batch: one lane per (key k, hop row h, column col) of the [N][HR][C] table, counter = base[h] + col.
// A counter past 2^32 - 1 does not exist and gets 0xFF, which matches no band.
__global__ __launch_bounds__(256) void es_hop_window_kernel(const uint8_t* __restrict__ ring_p, long long N, const uint32_t* __restrict__ base_p,
        long long HR, long long C, uint8_t* __restrict__ hop_p)
{
    const long long n = N * HR * C, stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long kh = i / C, col = i - kh * C, k = kh / HR, h = kh - k * HR;
        const unsigned long long ctr = (unsigned long long)((g_cu32*)base_p)[h] + (unsigned long long)col;
        g_cu32* row = (g_cu32*)(ring_p + k * ES_KEYRING_BYTES);
        uint32_t b = 0xFFu;
        if (ctr <= 0xFFFFFFFFull) ES_HOP_BAND(b, row, (uint32_t)ctr);
        ((g_u8*)hop_p)[i] = (uint8_t)b;
    }
}

// The candidate (peak slot, counter) pairs of _scan_band_multi_frame in try order, for key k and row `row` = item `pair` of the
// launch, by one wave.  T: the row's sample count, against which a peak is judged to hold a frame or not.
// AT (es_plan_at_kernel): the row's first sample is absolute sample pos0 of a stream whose frame k carries counter ctr0 + k, so counters
// are 64-bit here and end at 2^32 - 1, and column 0 of the hop row read is counter hbase.  Without AT the hop row is the key's and starts
// at counter 0; pos0, ctr0, hbase and hrow are not read.
template <bool AT>
__device__ __forceinline__ void plan_row(long long pair, long long k, long long row, int T, const int32_t* __restrict__ peaks_p,
        const int32_t* __restrict__ npeaks_p, const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p, int C,
        uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p, int32_t* __restrict__ count_p, int32_t* __restrict__ looked_p,
        long long pos0 = 0, long long ctr0 = 0, long long hbase = 0, long long hrow = 0)
{
    using ctr_t = typename std::conditional<AT, long long, int>::type;
    const int lane = threadIdx.x & 63;
    g_ci32* peaks = (g_ci32*)peaks_p + row * ES_MAX_PEAKS;
    g_cu8* hop = (g_cu8*)hop_p + (AT ? hrow : k) * (long long)C;
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
        ctr_t est;
        if constexpr (AT) est = ctr0 + (2 * (pos0 + start) + ES_FRAME_LEN) / (2 * ES_FRAME_LEN);     // the frame the absolute sample lies in
        else est = (int)((2LL * start + ES_FRAME_LEN) / (2 * ES_FRAME_LEN));          // round(start / 1215): 1215 is odd, no ties
        bool wide = true;
        if (!hok) {                                                                   // the +-3 window, gated by the hop alone
            const ctr_t c = est - 3 + lane;
            bool v;                                                                   // (every hop read is guarded by the hop row's width)
            if constexpr (AT) v = lane < 7 && c >= 0 && c <= 0xFFFFFFFFLL && c - hbase >= 0 && c - hbase < C && hop[c - hbase] == band;
            else v = lane < 7 && c >= 0 && c < C && hop[c] == band;
            const unsigned long long m = __ballot(v);
            if (m) {
                const int pos = tried + lanes_below(m);
                if (v && pos < ES_MAX_TRIES) { slot_out[pos] = (uint8_t)s; ctr_out[pos] = (uint32_t)c; }
                tried += __popcll(m);
                wide = false;
            }
        }
        if (wide) {                                                                   // the +-200 window; with a header also gated by lo16
            const ctr_t lo = est - 200 > 0 ? est - 200 : 0, hi = est + 200;
            #pragma unroll 1
            for (ctr_t c0 = lo; c0 <= hi && tried < ES_MAX_TRIES; c0 += 64) {
                const ctr_t c = c0 + lane;
                bool v;
                if constexpr (AT) v = c <= hi && c <= 0xFFFFFFFFLL && c - hbase >= 0 && c - hbase < C && hop[c - hbase] == band &&
                                      (!hok || (int)(c & 0xFFFF) == lo16);
                else v = c <= hi && c < C && hop[c] == band && (!hok || (c & 0xFFFF) == lo16);
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

// one wave per (key, row), four waves per workgroup; every row T samples
__global__ __launch_bounds__(256) void es_plan_kernel(const int32_t* __restrict__ peaks_p, const int32_t* __restrict__ npeaks_p,
        const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p, long long rows, int T,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p,
        long long N, int C, uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p, int32_t* __restrict__ count_p,
        int32_t* __restrict__ looked_p)
{
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // wave-uniform
    if (pair >= N * rows) return;
    const long long k = pair / rows, row = pair - k * rows;
    plan_row<false>(pair, k, row, T, peaks_p, npeaks_p, rowband_p, base_p, hok_p, hlo_p, P, hop_p, C, slot_p, cctr_p, count_p, looked_p);
}

// the same with row r of len_p[r] samples
__global__ __launch_bounds__(256) void es_plan_ragged_kernel(const int32_t* __restrict__ peaks_p, const int32_t* __restrict__ npeaks_p,
        const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p, long long rows, const int32_t* __restrict__ len_p,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p,
        long long N, int C, uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p, int32_t* __restrict__ count_p,
        int32_t* __restrict__ looked_p)
{
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // wave-uniform
    if (pair >= N * rows) return;
    const long long k = pair / rows, row = pair - k * rows;
    plan_row<false>(pair, k, row, ((g_ci32*)len_p)[row], peaks_p, npeaks_p, rowband_p, base_p, hok_p, hlo_p, P, hop_p, C, slot_p, cctr_p, count_p,
             looked_p);
}

// es_plan_ragged_kernel for rows that lie somewhere in a stream: row r starts at absolute sample pos0[r] of a stream whose counters
// start at ctr0[r], and the pair (k, r) reads hop row hrow[r] of key k's HR hop rows, whose column 0 is counter hbase[hrow[r]].
// A hop row index outside [0, HR) plans nothing.
__global__ __launch_bounds__(256) void es_plan_at_kernel(const int32_t* __restrict__ peaks_p, const int32_t* __restrict__ npeaks_p,
        const uint8_t* __restrict__ rowband_p, const int32_t* __restrict__ base_p, long long rows, const int32_t* __restrict__ len_p,
        const uint8_t* __restrict__ hok_p, const int32_t* __restrict__ hlo_p, long long P, const uint8_t* __restrict__ hop_p,
        long long N, int C, const long long* __restrict__ pos0_p, const uint32_t* __restrict__ ctr0_p, const int32_t* __restrict__ hrow_p,
        const uint32_t* __restrict__ hbase_p, int HR, uint8_t* __restrict__ slot_p, uint32_t* __restrict__ cctr_p,
        int32_t* __restrict__ count_p, int32_t* __restrict__ looked_p)
{
    const long long pair = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);      // wave-uniform
    if (pair >= N * rows) return;
    const long long k = pair / rows, row = pair - k * rows;
    const int h = ((g_ci32*)hrow_p)[row];
    if (h < 0 || h >= HR) {
        if ((threadIdx.x & 63) == 0) {
            ((g_i32*)count_p)[pair] = 0;
            if (looked_p) ((g_i32*)looked_p)[pair] = 0;
        }
        return;
    }
    plan_row<true>(pair, k, row, ((g_ci32*)len_p)[row], peaks_p, npeaks_p, rowband_p, base_p, hok_p, hlo_p, P, hop_p, C, slot_p, cctr_p, count_p,
                   looked_p, ((g_ci64*)pos0_p)[row], (long long)((g_cu32*)ctr0_p)[row], (long long)((g_cu32*)hbase_p)[h], k * HR + h);
}

// ---- acquisition: every counter of a 32-bit span a decoded header may belong to (es_acquire_mask_batch, es_acquire_list_batch) ----
// A record p is one (key, fitting peak) with its header decode; its candidates are the counters (h << 16) | lo16[p] of the span that hop to
// the band the peak was found in.  Row p of the mask has one bit per high half h, bit h - h0 of [W] words; a wave covers one tile of 64 high
// halves (two words) of one record, TW = ceil(W / 2) tiles per record, four waves per workgroup.

// One lane per (record, h): the HMAC of its counter where the record is live and the counter lies in [ctr_lo, ctr_hi).  Both words of the
// tile are written whatever they hold.
__global__ __launch_bounds__(256) void es_acquire_mask_kernel(const uint8_t* __restrict__ ring_p, long long N, const int32_t* __restrict__ key_p,
        const uint8_t* __restrict__ ok_p, const int32_t* __restrict__ lo16_p, const uint8_t* __restrict__ band_p, long long P, long long ctr_lo,
        long long ctr_hi, long long h0, int H, int W, int TW, uint32_t* __restrict__ mask_p)
{
    const long long g = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);         // wave-uniform
    if (g >= P * TW) return;
    const long long p = g / TW;
    const int tile = (int)(g - p * TW), lane = threadIdx.x & 63, j = tile * 64 + lane;
    const long long key = ((g_ci32*)key_p)[p];
    const int lo16 = ((g_ci32*)lo16_p)[p];
    const bool live = ((g_cu8*)ok_p)[p] != 0 && key >= 0 && key < N && lo16 >= 0 && lo16 <= 0xFFFF;
    const long long c = ((h0 + j) << 16) | (long long)(lo16 & 0xFFFF);
    bool v = live && j < H && c >= ctr_lo && c < ctr_hi;                                        // (ctr_hi <= 2^32: c is a 32-bit counter)
    if (v) {
        g_cu32* row = (g_cu32*)(ring_p + key * ES_KEYRING_BYTES);
        uint32_t b = 0;
        ES_HOP_BAND(b, row, (uint32_t)c);
        v = b == ((g_cu8*)band_p)[p];
    }
    const unsigned long long m = __ballot(v);
    g_u32* out = (g_u32*)mask_p + p * W;
    if (lane == 0) out[2 * tile] = (uint32_t)m;                                                 // (2 * tile < W by TW = ceil(W / 2))
    if (lane == 32 && 2 * tile + 1 < W) out[2 * tile + 1] = (uint32_t)(m >> 32);
}

// count[p] = set bits of mask row p: one wave per record over the words the launch before wrote (integer sums: the same in any order)
__global__ __launch_bounds__(256) void es_acquire_count_kernel(const uint32_t* __restrict__ mask_p, long long P, int W, int32_t* __restrict__ count_p)
{
    const long long p = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);         // wave-uniform
    if (p >= P) return;
    const int lane = threadIdx.x & 63;
    g_cu32* row = (g_cu32*)mask_p + p * W;
    uint32_t n = 0;
    #pragma unroll 1
    for (int w = lane; w < W; w += 64) n += (uint32_t)__popc(row[w]);
    n = es_wave_incl_scan_u32(n);
    if (lane == 63) ((g_i32*)count_p)[p] = (int32_t)n;
}

// The set bits of every record with base[p] >= 0 as (record, counter) entries base[p] + i, i ascending with h.  A wave owns one tile: its
// offset in the record's list is the popcount of the row's words before the tile, which it sums itself (no wave waits for another); inside
// the tile the order comes from the ballot.  An entry at or past `total` is not written.
__global__ __launch_bounds__(256) void es_acquire_list_kernel(const uint32_t* __restrict__ mask_p, const int32_t* __restrict__ lo16_p, long long P,
        long long h0, int W, int TW, const long long* __restrict__ base_p, long long total, int32_t* __restrict__ rec_p, uint32_t* __restrict__ ctr_p)
{
    const long long g = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);         // wave-uniform
    if (g >= P * TW) return;
    const long long p = g / TW;
    const int tile = (int)(g - p * TW), lane = threadIdx.x & 63;
    const long long base = ((g_ci64*)base_p)[p];
    if (base < 0) return;
    g_cu32* row = (g_cu32*)mask_p + p * W;
    uint32_t before = 0;
    #pragma unroll 1
    for (int w = lane; w < 2 * tile; w += 64) before += (uint32_t)__popc(row[w]);
    before = (uint32_t)es_wave_read_lane((int)es_wave_incl_scan_u32(before), 63);
    const int wi = 2 * tile + (lane >> 5);
    const bool v = wi < W && ((row[wi < W ? wi : 0] >> (lane & 31)) & 1u) != 0;
    const unsigned long long m = __ballot(v);
    const long long at = base + before + lanes_below(m);
    if (v && at < total) {
        ((g_i32*)rec_p)[at] = (int32_t)p;
        ((g_u32*)ctr_p)[at] = (uint32_t)(((h0 + tile * 64 + lane) << 16) | (long long)(((g_ci32*)lo16_p)[p] & 0xFFFF));
    }
}

// ---- presence: the preamble peaks of a clip against a key's hop sequence (include/echoseal_presence.h; host twin: echoseal_amd/presence.py) ----
// Clip b owns rows 4 b .. 4 b + 3 of corr [rows][stride], row 4 b + band the correlation row of BAND_PLAN index `band`, lags [0, nlag[b]);
// J = nlag / 1215 whole slots.  Every sum is float64, added slot by slot from +0.0 in ascending slot order by ONE lane (no FMA: the unit
// is built with -ffp-contract=off), so a plain host loop gives the same bits.  No column at or past nlag is read.
constexpr int HS_TILE = ES_HOP_TILE, HS_ORIGINS = ES_HOP_ORIGINS;
static_assert(HS_ORIGINS == 256 && HS_TILE * 4 == HS_ORIGINS, "one lane loads one (slot, band) value of a tile");

__device__ __forceinline__ long long clip_nlag(const int32_t* __restrict__ nlag_p, long long b, long long stride)
{
    const long long n = ((g_ci32*)nlag_p)[b];
    return n < 0 ? 0 : (n > stride ? stride : n);
}

// the largest of the four band rows at one lag: band 0 first, a later band only where strictly larger
__device__ __forceinline__ double band_max(const double* __restrict__ v, long long stride)
{
    double m = v[0];
    #pragma unroll
    for (int band = 1; band < 4; ++band) {
        const double c = v[band * stride];
        m = c > m ? c : m;
    }
    return m;
}

// the same for a record whose four band rows lie anywhere: o[band] = the element offset of the row of BAND_PLAN band `band` from v
struct band_rows { long long o[4]; };
__device__ __forceinline__ double band_max(const double* __restrict__ v, const band_rows& r)
{
    double m = v[r.o[0]];
    #pragma unroll
    for (int band = 1; band < 4; ++band) {
        const double c = v[r.o[band]];
        m = c > m ? c : m;
    }
    return m;
}

// fold[b][phi] = sum over slots j of the largest of the four band rows at lag phi + 1215 j: one lane per (clip, phase), five blocks per clip
__global__ __launch_bounds__(256) void es_phase_fold_kernel(const double* __restrict__ corr_p, long long stride, const int32_t* __restrict__ nlag_p,
        double* __restrict__ fold_p)
{
    const long long b = blockIdx.x / 5;
    const int phi = (int)(blockIdx.x - b * 5) * 256 + (int)threadIdx.x;
    if (phi >= ES_FRAME_LEN) return;
    const long long J = clip_nlag(nlag_p, b, stride) / ES_FRAME_LEN;
    const double* row = corr_p + 4 * b * stride + phi;
    double acc = 0.0;
    #pragma unroll 1
    for (long long j = 0; j < J; ++j)
        acc = acc + band_max(row + j * ES_FRAME_LEN, stride);
    fold_p[b * ES_FRAME_LEN + phi] = acc;
}

// hs_best, hs_better, hs_block_best: what a lane, a block or a (clip, key) pair has found so far (es_hop_best.h)

// One block per (clip b, key k, chunk of 256 origins), one lane per origin.  Per list entry the [J][4] values of its phase pass through
// LDS in tiles of HS_TILE slots; the lane adds vals[j][hop[k][origin + j]] slot by slot, so neighbouring lanes read neighbouring hop bytes.
// An origin whose window holds a byte above 3 (0xFF: a counter that does not exist) is not scored.  The block's best goes to slot
// (b K + k) NB + chunk of the scratch arrays.
__global__ __launch_bounds__(256) void es_hop_score_kernel(const double* __restrict__ corr_p, long long stride, const int32_t* __restrict__ nlag_p,
        const int32_t* __restrict__ phase_p, int P, const uint8_t* __restrict__ hop_p, long long K, long long Ccols, long long n_origins,
        long long NB, double* __restrict__ sc_score, long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    __shared__ double vals[HS_TILE * 4];
    __shared__ hs_best red[HS_ORIGINS];
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x % NB, bk = blockIdx.x / NB, k = bk % K, b = bk / K;
    const long long origin = chunk * HS_ORIGINS + tid;
    const bool live = origin < n_origins;
    const long long J = clip_nlag(nlag_p, b, stride) / ES_FRAME_LEN;
    g_cu8* hop = (g_cu8*)hop_p + k * Ccols + (live ? origin : 0);                         // columns origin .. origin + J - 1 < Ccols (the entry point's check)
    const double* rows = corr_p + 4 * b * stride;
    hs_best best = {-__builtin_inf(), -1, -1};
    #pragma unroll 1
    for (int p = 0; p < P; ++p) {
        const int phi = ((g_ci32*)phase_p)[b * P + p];
        if (phi < 0 || phi >= ES_FRAME_LEN || J == 0) continue;                           // (block-uniform) an entry that is no phase is not scored
        double acc = 0.0;
        bool ok = live;
        #pragma unroll 1
        for (long long j0 = 0; j0 < J; j0 += HS_TILE) {
            const int nt = (int)(J - j0 < HS_TILE ? J - j0 : HS_TILE);
            __syncthreads();                                                              // the tile before has been read
            if ((tid >> 2) < nt) vals[tid] = rows[(tid & 3) * stride + phi + (j0 + (tid >> 2)) * ES_FRAME_LEN];
            __syncthreads();
            if (live) {
                #pragma unroll 1
                for (int j = 0; j < nt; ++j) {
                    const unsigned h = hop[j0 + j];
                    ok = ok && h < 4u;
                    acc = acc + vals[4 * j + (int)(h & 3u)];
                }
            }
        }
        const double s = acc / (double)J;
        if (ok && (best.origin < 0 || s > best.score)) { best.score = s; best.origin = origin; best.rank = p; }
    }
    hs_block_best(red, best, tid, sc_score, sc_origin, sc_rank);
}

// the best of the NB chunks of each (clip, key), chunks ascending (ties keep the lower origin): one lane per pair
__global__ __launch_bounds__(256) void es_hop_best_kernel(const double* __restrict__ sc_score, const long long* __restrict__ sc_origin,
        const long long* __restrict__ sc_rank, long long pairs, long long NB, double* __restrict__ score_p, long long* __restrict__ origin_p,
        int32_t* __restrict__ rank_p)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pairs) return;
    hs_best best = {-__builtin_inf(), -1, -1};
    #pragma unroll 1
    for (long long c = 0; c < NB; ++c) {
        const hs_best cand = {sc_score[i * NB + c], sc_origin[i * NB + c], (int)sc_rank[i * NB + c]};
        if (hs_better(cand, best)) best = cand;
    }
    score_p[i] = best.score; origin_p[i] = best.origin; rank_p[i] = best.rank;
}

// ---- presence along a table of per-slot offsets (include/echoseal_warp.h) ----
// Slot j of row d of clip b starts at lag 1215 j + warp[b][d][j].  A row is usable where d < nwarp[b] and every one of its J slots lies
// whole inside [0, nlag): both kernels judge each slot from the table before they read it, so no table can make them read past a row.
constexpr int WS_HB = ES_WARP_HB;

// J of clip b: nslot[b] clamped to [0, min(Jw, nlag / 1215)]
__device__ __forceinline__ long long warp_slots(const es_warp_tab& tab, long long b, long long n)
{
    const long long most = n / ES_FRAME_LEN < tab.Jw ? n / ES_FRAME_LEN : tab.Jw, J = ((g_ci32*)tab.nslot)[b];
    return J < 0 ? 0 : (J > most ? most : J);
}

// the first lag of slot j under offset w, or -1 where the slot does not lie whole inside [0, n)
__device__ __forceinline__ long long warp_lag(long long j, int w, long long n)
{
    const long long c = j * ES_FRAME_LEN + w;
    return (c >= 0 && c + (ES_FRAME_LEN - 1) < n) ? c : -1;
}

// fold[b][d][phi] = sum over slots j of band_max at lag phi + 1215 j + warp[b][d][j], -inf for an unusable row: one lane per (record, row,
// phase), five blocks per (record, row) = item bd of the launch; the row's offsets pass through LDS 256 slots at a time, already turned into
// first lags.  The one body of es_warp_fold_kernel and es_warp_fold_at_kernel: corr_p + lag0 + phi is lag 0 of phase phi, r says where the four
// band rows lie from there (ROWS: a clip's stride, its rows being 4 b .. 4 b + 3, or the band_rows of a record anywhere), n is the record's
// lag count -- nothing but lags [0, n) of those rows is read.
template <typename ROWS>
__device__ __forceinline__ void warp_fold_body(const double* __restrict__ corr_p, long long lag0, const ROWS& r, long long n, long long b, long long d,
        long long bd, int phi, const es_warp_tab& tab, double* __restrict__ fold_p)
{
    __shared__ long long lag[256];
    const int tid = threadIdx.x;
    const long long J = warp_slots(tab, b, n);
    g_ci32* wrow = (g_ci32*)tab.warp + bd * tab.Jw;
    const double* row = corr_p + lag0 + phi;
    bool usable = d < ((g_ci32*)tab.nwarp)[b];                                            // block-uniform, like everything the loop branches on
    double acc = 0.0;
    #pragma unroll 1
    for (long long j0 = 0; usable && j0 < J; j0 += 256) {
        const int nt = (int)(J - j0 < 256 ? J - j0 : 256);
        __syncthreads();                                                                  // the tile before has been read
        if (tid < nt) lag[tid] = warp_lag(j0 + tid, wrow[j0 + tid], n);
        usable = __syncthreads_and(tid >= nt || lag[tid] >= 0) != 0;
        if (usable && phi < ES_FRAME_LEN) {
            #pragma unroll 1
            for (int j = 0; j < nt; ++j)
                acc = acc + band_max(row + lag[j], r);
        }
    }
    if (phi < ES_FRAME_LEN) fold_p[bd * ES_FRAME_LEN + phi] = usable ? acc : -__builtin_inf();
}

__global__ __launch_bounds__(256) void es_warp_fold_kernel(const double* __restrict__ corr_p, long long stride, const int32_t* __restrict__ nlag_p,
        es_warp_tab tab, double* __restrict__ fold_p)
{
    const long long bd = blockIdx.x / 5, b = bd / tab.D, d = bd - b * tab.D;
    const int phi = (int)(blockIdx.x - bd * 5) * 256 + (int)threadIdx.x;
    warp_fold_body(corr_p, 4 * b * stride, stride, clip_nlag(nlag_p, b, stride), b, d, bd, phi, tab, fold_p);
}

// Record b of an _at call (include/echoseal_live_presence.h): its four rows are row[b][0 .. 3] of corr [rows][stride], its lag 0 column col[b].
// -> its lag count, nlag[b] clamped to [0, stride - col], and r.o[band] = row[b][band] * stride + col; 0 and zeros for a record that is not
// addressable (a row outside [0, rows) or a column outside [0, stride]).  Decided here, from the three arrays alone, before any row is read.
struct es_at_rec { const long long* row; const long long* col; const int32_t* nlag; long long rows, stride; };
__device__ __forceinline__ long long at_record(const es_at_rec& at, long long b, band_rows& r)
{
    const long long col = ((g_ci64*)at.col)[b];
    bool ok = col >= 0 && col <= at.stride;
    long long q[4];
    #pragma unroll
    for (int band = 0; band < 4; ++band) {
        q[band] = ((g_ci64*)at.row)[4 * b + band];
        ok = ok && q[band] >= 0 && q[band] < at.rows;
    }
    #pragma unroll
    for (int band = 0; band < 4; ++band) r.o[band] = ok ? q[band] * at.stride + col : 0;   // (rows * stride < 2^62: the entry point's check)
    const long long n = ((g_ci32*)at.nlag)[b], most = ok ? at.stride - col : 0;
    return n < 0 ? 0 : (n > most ? most : n);
}

// es_warp_fold_kernel over records that lie anywhere in the table of rows
__global__ __launch_bounds__(256) void es_warp_fold_at_kernel(const double* __restrict__ corr_p, es_at_rec at, es_warp_tab tab, double* __restrict__ fold_p)
{
    const long long bd = blockIdx.x / 5, b = bd / tab.D, d = bd - b * tab.D;
    const int phi = (int)(blockIdx.x - bd * 5) * 256 + (int)threadIdx.x;
    band_rows r;
    const long long n = at_record(at, b, r);
    warp_fold_body(corr_p, 0, r, n, b, d, bd, phi, tab, fold_p);
}

// es_hop_score_kernel along the table, the list taken HB entries at a time.  A lane's hop window is the same for every entry, so the slot
// tile is the outer loop and the block of entries the inner one: per tile the block's [HS_TILE][4][HB] values pass through LDS (the HB
// values of one (slot, band) side by side), a hop byte is read once per block, and acc[e] still takes its terms in ascending slot order.
// An entry is dropped where it names no usable row or no phase: e_bad is raised by whichever lane finds a slot of its row outside the
// clip, and that slot is not read.  HB = 1 is the loop of es_hop_score_kernel itself.
// The one body of es_warp_score_kernel and es_warp_score_at_kernel.  The staging lane tid & 3 owns one band.  Without AT `rows` stands on
// row 4 b of a clip and the lane's row is (tid & 3) * stride further; with AT `rows` stands on lag 0 of the lane's own row, wherever the
// record has it, and stride is not read.  n and J are the record's lags and slots, hop the lane's window (column 0 = its origin).
template <int HB, bool AT>
__device__ __forceinline__ void warp_score_body(const double* __restrict__ rows, long long stride, long long n, long long J, g_cu8* hop, bool live, long long origin,
        long long b, const es_warp_tab& tab, const int32_t* __restrict__ hyp_p, int H, double* __restrict__ sc_score, long long* __restrict__ sc_origin,
        long long* __restrict__ sc_rank)
{
    __shared__ __attribute__((aligned(16))) double vals[HS_TILE * 4 * HB];
    __shared__ hs_best red[HS_ORIGINS];
    __shared__ int e_row[HB], e_phi[HB], e_bad[HB];
    const int tid = threadIdx.x;
    hs_best best = {-__builtin_inf(), -1, -1};
    #pragma unroll 1
    for (int h0 = 0; h0 < H && J > 0; h0 += HB) {
        __syncthreads();                                                                  // the block before has been judged
        if (tid < HB) {
            int d = -1, phi = -1;
            if (h0 + tid < H) { d = ((g_ci32*)hyp_p)[(b * H + h0 + tid) * 2]; phi = ((g_ci32*)hyp_p)[(b * H + h0 + tid) * 2 + 1]; }
            const bool named = d >= 0 && d < tab.D && d < ((g_ci32*)tab.nwarp)[b] && phi >= 0 && phi < ES_FRAME_LEN;
            e_row[tid] = named ? d : -1; e_phi[tid] = phi; e_bad[tid] = !named;
        }
        __syncthreads();
        double acc[HB];
        #pragma unroll
        for (int e = 0; e < HB; ++e) acc[e] = 0.0;
        bool ok = live;
        #pragma unroll 1
        for (long long j0 = 0; j0 < J; j0 += HS_TILE) {
            const int nt = (int)(J - j0 < HS_TILE ? J - j0 : HS_TILE);
            __syncthreads();                                                              // the tile before has been read
            if ((tid >> 2) < nt) {
                const long long j = j0 + (tid >> 2);
                #pragma unroll
                for (int e = 0; e < HB; ++e) {
                    const int d = e_row[e];
                    const long long c = d < 0 ? -1 : warp_lag(j, ((g_ci32*)tab.warp)[(b * tab.D + d) * tab.Jw + j], n);
                    if (c >= 0) vals[tid * HB + e] = AT ? rows[c + e_phi[e]] : rows[(tid & 3) * stride + c + e_phi[e]];
                    else if (d >= 0) e_bad[e] = 1;
                }
            }
            __syncthreads();
            if (live) {
                #pragma unroll 1
                for (int j = 0; j < nt; ++j) {
                    const unsigned h = hop[j0 + j];
                    ok = ok && h < 4u;
                    const double* v = vals + (4 * j + (int)(h & 3u)) * HB;
                    #pragma unroll
                    for (int e = 0; e < HB; ++e) acc[e] = acc[e] + v[e];
                }
            }
        }
        #pragma unroll
        for (int e = 0; e < HB; ++e) {                                                    // entries ascending: of equal scores the earliest stays
            const double s = acc[e] / (double)J;
            if (ok && !e_bad[e] && (best.origin < 0 || s > best.score)) { best.score = s; best.origin = origin; best.rank = h0 + e; }
        }
    }
    hs_block_best(red, best, tid, sc_score, sc_origin, sc_rank);
}

template <int HB>
__global__ __launch_bounds__(256) void es_warp_score_kernel(const double* __restrict__ corr_p, long long stride, const int32_t* __restrict__ nlag_p,
        es_warp_tab tab, const int32_t* __restrict__ hyp_p, int H, const uint8_t* __restrict__ hop_p, long long K, long long Ccols,
        long long n_origins, long long NB, double* __restrict__ sc_score, long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x % NB, bk = blockIdx.x / NB, k = bk % K, b = bk / K;
    const long long origin = chunk * HS_ORIGINS + tid;
    const bool live = origin < n_origins;
    const long long n = clip_nlag(nlag_p, b, stride), J = warp_slots(tab, b, n);
    g_cu8* hop = (g_cu8*)hop_p + k * Ccols + (live ? origin : 0);                         // columns origin .. origin + J - 1 < Ccols: J <= Jw
    warp_score_body<HB, false>(corr_p + 4 * b * stride, stride, n, J, hop, live, origin, b, tab, hyp_p, H, sc_score, sc_origin, sc_rank);
}

// es_warp_score_kernel over records that lie anywhere in the table of rows; the pair (b, k) reads hop row hop_row[b] of key k's HR hop rows.
// A hop row index outside [0, HR) leaves the record no slot: nothing of it is read, nothing is scored.
template <int HB>
__global__ __launch_bounds__(256) void es_warp_score_at_kernel(const double* __restrict__ corr_p, es_at_rec at, es_warp_tab tab,
        const int32_t* __restrict__ hyp_p, int H, const uint8_t* __restrict__ hop_p, long long K, long long HR, long long Ccols,
        const int32_t* __restrict__ hop_row_p, long long n_origins, long long NB, double* __restrict__ sc_score, long long* __restrict__ sc_origin,
        long long* __restrict__ sc_rank)
{
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x % NB, bk = blockIdx.x / NB, k = bk % K, b = bk / K;
    const long long origin = chunk * HS_ORIGINS + tid;
    const bool live = origin < n_origins;
    band_rows r;
    const long long n = at_record(at, b, r);
    long long mine = r.o[0];                                                              // the staging lane tid & 3 owns one band: one row base per lane
    #pragma unroll
    for (int band = 1; band < 4; ++band) mine = (tid & 3) == band ? r.o[band] : mine;
    const long long hr = ((g_ci32*)hop_row_p)[b];
    const bool hashop = hr >= 0 && hr < HR;
    const long long J = hashop ? warp_slots(tab, b, n) : 0;
    g_cu8* hop = (g_cu8*)hop_p + (k * HR + (hashop ? hr : 0)) * Ccols + (live ? origin : 0); // columns origin .. origin + J - 1 < Ccols: J <= Jw
    warp_score_body<HB, true>(corr_p + mine, 0, n, J, hop, live, origin, b, tab, hyp_p, H, sc_score, sc_origin, sc_rank);
}

// ---- the hypothesis list of a presence test picked on the device (include/echoseal_pick.h) ----
// Per record the H candidates of largest fold value, equal values by the lower row and then the lower phase.
//
// One workgroup of four waves per record.  A value becomes a 96-bit key (hi, lo): hi the order-preserving integer image of the value
// (f64_key of es_wave.h after -0.0 has become +0.0; 0 for what is no candidate, -inf and every NaN -- no candidate's image is 0), lo the
// complement of its index d 1215 + phi, so that of equal values the lower index has the larger key.  The keys of a record are distinct,
// and entry h is the largest key strictly below entry h - 1's: H rounds of a maximum under a total order, which any reduction shape
// gives alike -- lanes stride over the record's nwarp 1215 values (coalesced 8-byte reads), the wave reduces through cross-lane moves,
// the four waves through four LDS slots that every lane then reads, so each lane knows the winner and no second barrier is needed
// (the slots alternate between two sets from round to round).  The first round without a candidate ends the list; the rest is filled.
constexpr int FP_BLOCK = 256, FP_WAVES = FP_BLOCK / 64;

struct fp_key { uint64_t hi; uint32_t lo; };

__device__ __forceinline__ bool fp_above(const fp_key& a, const fp_key& b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }

// the image of a candidate's value, 0 for -inf and NaN
__device__ __forceinline__ uint64_t fp_image(double v)
{
    uint64_t b; __builtin_memcpy(&b, &v, 8);
    const uint64_t mag = b & 0x7fffffffffffffffULL;
    if (mag > 0x7ff0000000000000ULL || b == 0xfff0000000000000ULL) return 0;
    double x = v;
    if (mag == 0) x = 0.0;                                                                // -0.0 == +0.0
    return f64_key(x);
}

template <int S>
__device__ __forceinline__ fp_key fp_max_xor(const fp_key& k, int lane)
{
    fp_key o;
    const uint32_t l = (uint32_t)xor_lanes_b32<S>((int)(uint32_t)k.hi, lane), h = (uint32_t)xor_lanes_b32<S>((int)(uint32_t)(k.hi >> 32), lane);
    o.hi = ((uint64_t)h << 32) | l;
    o.lo = (uint32_t)xor_lanes_b32<S>((int)k.lo, lane);
    return fp_above(o, k) ? o : k;
}

__global__ __launch_bounds__(FP_BLOCK) void es_fold_pick_kernel(const double* __restrict__ fold_p, long long D, const int32_t* __restrict__ nwarp_p, int H,
        int32_t* __restrict__ hyp_p, double* __restrict__ val_p)
{
    __shared__ fp_key red[2][FP_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    long long nw = nwarp_p ? (long long)((g_ci32*)nwarp_p)[b] : D;
    nw = nw < 0 ? 0 : (nw > D ? D : nw);
    const unsigned n = (unsigned)(nw * ES_FRAME_LEN);                                     // 1215 D < 2^31: the entry point's check
    const double* f = fold_p + b * D * ES_FRAME_LEN;                                      // values [0, n) of it are read, nothing else
    fp_key prev = {~0ull, ~0u};                                                           // above every key: no image is all ones
    int h = 0;
    #pragma unroll 1
    for (; h < H; ++h) {
        fp_key best = {0, 0};
        #pragma unroll 4
        for (unsigned i = tid; i < n; i += FP_BLOCK) {
            const fp_key k = {fp_image(f[i]), ~i};
            if (k.hi != 0 && fp_above(prev, k) && fp_above(k, best)) best = k;
        }
        best = fp_max_xor<1>(best, lane); best = fp_max_xor<2>(best, lane); best = fp_max_xor<4>(best, lane);
        best = fp_max_xor<8>(best, lane); best = fp_max_xor<16>(best, lane); best = fp_max_xor<32>(best, lane);
        if (lane == 0) red[h & 1][wave] = best;
        __syncthreads();
        best = red[h & 1][0];
        #pragma unroll
        for (int w = 1; w < FP_WAVES; ++w)
            if (fp_above(red[h & 1][w], best)) best = red[h & 1][w];
        if (best.hi == 0) break;                                                          // (block-uniform) the record has no further candidate
        if (tid == 0) {
            const unsigned i = ~best.lo;
            hyp_p[(b * H + h) * 2] = (int32_t)(i / ES_FRAME_LEN);
            hyp_p[(b * H + h) * 2 + 1] = (int32_t)(i % ES_FRAME_LEN);
            if (val_p) val_p[b * H + h] = f[i];
        }
        prev = best;
    }
    for (int e = h + tid; e < H; e += FP_BLOCK) {                                         // entries that name nothing
        hyp_p[(b * H + e) * 2] = -1;
        hyp_p[(b * H + e) * 2 + 1] = -1;
        if (val_p) val_p[b * H + e] = -__builtin_inf();
    }
}

}  // namespace

int es_launch_keyring_derive(es_ctx* ctx, const uint8_t* master32, int64_t N, uint8_t* ring, hipStream_t st)
{
    return es_launch(ctx, es_keyring_derive_kernel, es_grid(N, 256, ctx->num_cu * 8), 256, 0, st, master32, (long long)N,
                     (const uint8_t*)ctx->d_sbox, ring);
}

int es_launch_schedule_keyed(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint32_t* ctr, int64_t n,
                             uint8_t* pn_rows, uint8_t* band, hipStream_t st)
{
    return es_launch(ctx, es_schedule_keyed_kernel, es_grid(n, 256, ctx->num_cu * 8), 256, 0, st, ring, (long long)N, key, ctr,
                     (long long)n, (const uint8_t*)ctx->d_sbox, pn_rows, band);
}

int es_launch_plan(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base,
                   int64_t rows, int T, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop, int64_t N, int C,
                   uint8_t* cand_slot, uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st)
{
    const long long pairs = (long long)N * rows;                                      // one wave each, four waves per block
    return es_launch(ctx, es_plan_kernel, (unsigned)((pairs + 3) / 4), 256, 0, st, peaks, npeaks, rowband, hdr_base,
                     (long long)rows, T, hdr_ok, hdr_lo16, (long long)P, hop, (long long)N, C, cand_slot, cand_ctr, count, looked);
}

int es_launch_plan_ragged(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base,
                          int64_t rows, const int32_t* len, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop,
                          int64_t N, int C, uint8_t* cand_slot, uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st)
{
    const long long pairs = (long long)N * rows;                                      // one wave each, four waves per block
    return es_launch(ctx, es_plan_ragged_kernel, (unsigned)((pairs + 3) / 4), 256, 0, st, peaks, npeaks, rowband, hdr_base,
                     (long long)rows, len, hdr_ok, hdr_lo16, (long long)P, hop, (long long)N, C, cand_slot, cand_ctr, count, looked);
}

int es_launch_plan_at(es_ctx* ctx, const int32_t* peaks, const int32_t* npeaks, const uint8_t* rowband, const int32_t* hdr_base, int64_t rows,
                      const int32_t* len, const uint8_t* hdr_ok, const int32_t* hdr_lo16, int64_t P, const uint8_t* hop, int64_t N, int C,
                      const int64_t* pos0, const uint32_t* ctr0, const int32_t* hop_row, const uint32_t* hop_base, int HR, uint8_t* cand_slot,
                      uint32_t* cand_ctr, int32_t* count, int32_t* looked, hipStream_t st)
{
    const long long pairs = (long long)N * rows;                                      // one wave each, four waves per block
    return es_launch(ctx, es_plan_at_kernel, (unsigned)((pairs + 3) / 4), 256, 0, st, peaks, npeaks, rowband, hdr_base, (long long)rows, len,
                     hdr_ok, hdr_lo16, (long long)P, hop, (long long)N, C, (const long long*)pos0, ctr0, hop_row, hop_base, HR, cand_slot,
                     cand_ctr, count, looked);
}

int es_launch_hop_window(es_ctx* ctx, const uint8_t* ring, int64_t N, const uint32_t* hop_base, int64_t HR, int64_t C, uint8_t* hop,
                         hipStream_t st)
{
    return es_launch(ctx, es_hop_window_kernel, es_grid((long long)N * HR * C, 256, ctx->num_cu * 8), 256, 0, st, ring, (long long)N, hop_base,
                     (long long)HR, (long long)C, hop);
}

// the exact grids of the acquisition kernels (one wave per tile of 64 high halves, four waves per block): no cap, the entry points refuse a
// call whose grid would pass 2^31 - 1 blocks
int es_launch_acquire_mask(es_ctx* ctx, const uint8_t* ring, int64_t N, const int32_t* key, const uint8_t* ok, const int32_t* lo16,
                           const uint8_t* band, int64_t P, int64_t ctr_lo, int64_t ctr_hi, uint32_t* mask, int32_t* count, hipStream_t st)
{
    const long long h0 = ctr_lo >> 16, H = ((ctr_hi + 65535) >> 16) - h0, W = (H + 31) / 32, TW = (W + 1) / 2;
    if (const int rc = es_launch(ctx, es_acquire_mask_kernel, (unsigned)((P * TW + 3) / 4), 256, 0, st, ring, (long long)N, key, ok, lo16, band,
                                 (long long)P, (long long)ctr_lo, (long long)ctr_hi, h0, (int)H, (int)W, (int)TW, mask)) return rc;
    return es_launch(ctx, es_acquire_count_kernel, (unsigned)((P + 3) / 4), 256, 0, st, (const uint32_t*)mask, (long long)P, (int)W, count);
}

int es_launch_acquire_list(es_ctx* ctx, const uint32_t* mask, const int32_t* lo16, int64_t P, int64_t ctr_lo, int64_t ctr_hi, const int64_t* base,
                           int64_t total, int32_t* cand_rec, uint32_t* cand_ctr, hipStream_t st)
{
    const long long h0 = ctr_lo >> 16, H = ((ctr_hi + 65535) >> 16) - h0, W = (H + 31) / 32, TW = (W + 1) / 2;
    return es_launch(ctx, es_acquire_list_kernel, (unsigned)((P * TW + 3) / 4), 256, 0, st, mask, lo16, (long long)P, h0, (int)W, (int)TW,
                     (const long long*)base, (long long)total, cand_rec, cand_ctr);
}

// the exact grids of the presence kernels: the entry points refuse a call whose grid would pass 2^31 - 1 blocks
int es_launch_phase_fold(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, double* fold, hipStream_t st)
{
    return es_launch(ctx, es_phase_fold_kernel, (unsigned)(B * 5), 256, 0, st, corr, (long long)stride, nlag, fold);
}

// the launch that reduces the blocks' bests in the caller's scratch (hs_scratch: es_hop_best.h), for the score kernels here and in es_coherent_body.inc
int es_launch_hop_best(es_ctx* ctx, const hs_scratch& sc, double* score, int64_t* origin, int32_t* rank, hipStream_t st)
{
    return es_launch(ctx, es_hop_best_kernel, (unsigned)((sc.pairs + 255) / 256), 256, 0, st, (const double*)sc.score, (const long long*)sc.origin,
                     (const long long*)sc.rank, sc.pairs, sc.NB, score, (long long*)origin, rank);
}

int es_launch_hop_score(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const int32_t* phase, int P,
                        const uint8_t* hop, int64_t K, int64_t Ccols, int64_t n_origins, double* score, int64_t* origin, int32_t* rank,
                        void* scratch, hipStream_t st)
{
    const hs_scratch sc(scratch, B, K, n_origins);
    if (sc.slots > 0)
        if (const int rc = es_launch(ctx, es_hop_score_kernel, (unsigned)sc.slots, 256, 0, st, corr, (long long)stride, nlag, phase, P, hop, (long long)K,
                                     (long long)Ccols, (long long)n_origins, sc.NB, sc.score, sc.origin, sc.rank)) return rc;
    return es_launch_hop_best(ctx, sc, score, origin, rank, st);
}

// the same along a table of per-slot offsets (include/echoseal_warp.h): exact grids again, checked by the entry points
int es_launch_warp_fold(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const es_warp_tab& tab, double* fold,
                        hipStream_t st)
{
    return es_launch(ctx, es_warp_fold_kernel, (unsigned)(B * tab.D * 5), 256, 0, st, corr, (long long)stride, nlag, tab, fold);
}

int es_launch_warp_score(es_ctx* ctx, const double* corr, int64_t stride, const int32_t* nlag, int64_t B, const es_warp_tab& tab,
                         const int32_t* hyp, int64_t H, const uint8_t* hop, int64_t K, int64_t Ccols, int64_t n_origins, double* score,
                         int64_t* origin, int32_t* rank, void* scratch, hipStream_t st)
{
    const hs_scratch sc(scratch, B, K, n_origins);
    if (sc.slots > 0)
        if (const int rc = es_launch(ctx, es_warp_score_kernel<WS_HB>, (unsigned)sc.slots, 256, 0, st, corr, (long long)stride, nlag, tab, hyp, (int)H,
                                     hop, (long long)K, (long long)Ccols, (long long)n_origins, sc.NB, sc.score, sc.origin, sc.rank)) return rc;
    return es_launch_hop_best(ctx, sc, score, origin, rank, st);
}

// the same over records that lie anywhere in a table of rows (include/echoseal_live_presence.h): exact grids, checked by the entry points
int es_launch_warp_fold_at(es_ctx* ctx, const double* corr, int64_t rows, int64_t stride, const int64_t* row, const int64_t* col, const int32_t* nlag,
                           int64_t B, const es_warp_tab& tab, double* fold, hipStream_t st)
{
    return es_launch(ctx, es_warp_fold_at_kernel, (unsigned)(B * tab.D * 5), 256, 0, st, corr,
                     es_at_rec{(const long long*)row, (const long long*)col, nlag, (long long)rows, (long long)stride}, tab, fold);
}

int es_launch_warp_score_at(es_ctx* ctx, const double* corr, int64_t rows, int64_t stride, const int64_t* row, const int64_t* col, const int32_t* nlag,
                            int64_t B, const es_warp_tab& tab, const int32_t* hyp, int64_t H, const uint8_t* hop, int64_t K, int64_t HR, int64_t Ccols,
                            const int32_t* hop_row, int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st)
{
    const hs_scratch sc(scratch, B, K, n_origins);
    if (sc.slots > 0)
        if (const int rc = es_launch(ctx, es_warp_score_at_kernel<WS_HB>, (unsigned)sc.slots, 256, 0, st, corr,
                                     es_at_rec{(const long long*)row, (const long long*)col, nlag, (long long)rows, (long long)stride}, tab, hyp, (int)H,
                                     hop, (long long)K, (long long)HR, (long long)Ccols, hop_row, (long long)n_origins, sc.NB, sc.score, sc.origin,
                                     sc.rank)) return rc;
    return es_launch_hop_best(ctx, sc, score, origin, rank, st);
}

// the exact grid, a workgroup per record: the entry point refuses B > 2^31 - 1
int es_launch_fold_pick(es_ctx* ctx, const double* fold, int64_t B, int64_t D, const int32_t* nwarp, int64_t H, int32_t* hyp, double* val, hipStream_t st)
{
    return es_launch(ctx, es_fold_pick_kernel, (unsigned)B, FP_BLOCK, 0, st, fold, (long long)D, nwarp, (int)H, hyp, val);
}

// the coherent presence test (include/echoseal_coherent.h): its two kernels and launchers, a file of their own in this unit
#include "es_coherent_body.inc"
