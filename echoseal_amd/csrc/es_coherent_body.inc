// es_coherent_body.inc -- the coherent presence test (include/echoseal_coherent.h; DESIGN 4.27; host twin: echoseal_amd/presence.py
// mf_rows_model, coherent_score_model).  Where the presence test of es_keyring.hip sums normalised preamble correlations (63 chips per
// frame), this one sums, per hypothesised (key, counter) and frame start, the 63 preamble chips and the 128 header chips -- the counter's
// low 16 bits, each over 8 chips, times the key's header PN -- on matched-filter rows, over every phase of the 1215-sample grid.
//
// Two kernels.  es_mf_rows_kernel: the keyless rows of a band-passed record, a tiled FIR with the taps and a tile of samples in LDS, one
// lane per output.  es_coherent_score_kernel: one lane per counter origin, as es_hop_score_kernel; what the lanes of a (list entry, slot)
// share -- the preamble sum, the normaliser and the sixteen 8-chip header sums of each band -- passes through LDS in tiles of slots.
// es_coherent_score_at_kernel (include/echoseal_coherent_at.h; DESIGN 4.28) is the same device body over records that name their rows,
// column, hop row and counter base: the windows of a clip's timeline on the clip's own rows.
//
// Float64 throughout; every sum is added term by term in ascending order from +0.0 by ONE lane, a product formed and then added (the unit
// is built with -ffp-contract=off), so a plain host loop gives the same bits.  No atomic, no workspace of the context.
// Compiled into es_keyring.hip, whose last lines include this file: the score kernel here ends in that unit's reduction (es_hop_best.h,
// es_hop_best_kernel) and reads the same ring and hop rows.

namespace {

constexpr int MF_TILE = ES_MF_TILE;
constexpr int COH_PRE = ES_PRE_L, COH_HDR = 128, COH_SPAN = COH_PRE + COH_HDR - 1;       // 190: the last known chip of a frame start, from its first
constexpr int MF_MEXT = MF_TILE + COH_PRE - 1;                                             // m values a tile's preamble sums read
constexpr unsigned long long PRE_BITS = 0x8218A7A392DD9ABEull;                             // the 63-chip MLS, chip q = bit 63 - q (utils.mseq_63)
static_assert(MF_TILE == 256 && COH_PRE == 63 && COH_SPAN == 190, "one lane per output of a tile");

struct mf_norm { double c[ES_NBANDS]; };

// One block per (record r, tile of 256 outputs from t0).  LDS: the band's taps in forward order, samples [t0, t0 + 256 + 189 + L) of the
// record (0.0 at or past its length: nothing there is read from memory, and no value that depends on it is stored), and m over
// [t0, t0 + 256 + 62).  MAXT: the longest filter this instantiation holds.
template <int MAXT>
__global__ __launch_bounds__(256) void es_mf_rows_kernel(const double* __restrict__ y_p, long long T, const int32_t* __restrict__ len_p,
        const uint8_t* __restrict__ band_p, const es_band_tables* __restrict__ tab, mf_norm norm, long long tiles, double* __restrict__ m_p,
        double* __restrict__ a_p, double* __restrict__ d_p)
{
    constexpr int YT = MF_TILE + COH_SPAN - 1 + MAXT;
    __shared__ double g[MAXT];
    __shared__ double ys[YT];
    __shared__ double ms[MF_MEXT + 1];
    const int tid = threadIdx.x;
    const long long r = blockIdx.x / tiles, t0 = (blockIdx.x - r * tiles) * MF_TILE;
    const unsigned band = ((g_cu8*)band_p)[r];
    long long n = ((g_ci32*)len_p)[r];
    n = n < 0 ? 0 : (n > T ? T : n);
    if (band >= (unsigned)ES_NBANDS) return;                                               // (block-uniform)
    int L = tab->ntaps[band];
    L = L < 1 ? 1 : (L > MAXT ? MAXT : L);                                                 // es_set_tables and the launcher hold 1 <= L <= MAXT
    const int W = COH_SPAN + L;
    if (t0 + L > n) return;                                                                // (block-uniform) no output of this tile is defined
    const double* y = y_p + r * T;
    for (int i = tid; i < L; i += 256) g[i] = (double)tab->taps[band][L - 1 - i];
    for (int i = tid; i < MF_TILE + W - 1; i += 256) ys[i] = t0 + i < n ? y[t0 + i] : 0.0;
    __syncthreads();
    #pragma unroll 1
    for (int t = tid; t < MF_MEXT; t += 256) {                                             // m over the tile and the 62 values past it
        double acc = 0.0;
        #pragma unroll 4
        for (int i = 0; i < L; ++i) acc = acc + ys[t + i] * g[i];
        ms[t] = acc;
    }
    __syncthreads();
    const long long t = t0 + tid;
    if (t + L <= n) m_p[r * T + t] = ms[tid];
    if (t + W > n) return;
    double a = 0.0, q = 0.0;
    #pragma unroll 7
    for (int k = 0; k < COH_PRE; ++k) {
        const double v = ms[tid + k];
        a = a + (((PRE_BITS >> (63 - k)) & 1ull) ? v : -v);
    }
    #pragma unroll 4
    for (int k = 0; k < W; ++k) q = q + ys[tid + k] * ys[tid + k];
    a_p[r * T + t] = a;
    d_p[r * T + t] = __builtin_sqrt(q) * norm.c[band];
}

// ---- the score ----
constexpr int CT = ES_COH_TILE, CO = ES_HOP_ORIGINS;
// per (slot of the tile, band): a, d, Z_0 .. Z_15, and (a + H) for the two high bytes the block's 256 consecutive counters can hold
constexpr int CS_A = 0, CS_D = 1, CS_Z = 2, CS_AH = 18, CS_REC = 20;
static_assert(CO == 256 && CT * ES_NBANDS * 16 == 4 * CO, "four header sums per lane and tile");

// J of clip b: nslot[b] clamped to [0, max(0, T - 190) / 1215] -- index phi + 1215 j + 190 of a row stays below T for phi <= 1214, j < J
__device__ __forceinline__ long long coh_slots(const int32_t* __restrict__ nslot_p, long long b, long long T)
{
    const long long most = T > COH_SPAN ? (T - COH_SPAN) / ES_FRAME_LEN : 0, J = ((g_ci32*)nslot_p)[b];
    return J < 0 ? 0 : (J > most ? most : J);
}

// the signed sum of eight header sums under one byte of the counter, MSB first, from +0.0
__device__ __forceinline__ double byte_sum(const double* z, unsigned byte)
{
    double s = 0.0;
    #pragma unroll
    for (int i = 0; i < 8; ++i) s = s + (((byte >> (7 - i)) & 1u) ? z[i] : -z[i]);
    return s;
}

// The one body of es_coherent_score_kernel and es_coherent_score_at_kernel (DESIGN 4.14, 4.28): a block serves (record, key, chunk of 256
// origins), one lane per origin; the kernels differ only in where a record's rows, hop bytes and counters start, which they hand over as
//   mine   the index in m, a, d of sample 0 of the record's row of band (tid >> 4) & 3 -- the one band this lane stages (64-bit: a row
//          base may pass 2^31)
//   J      the record's slots, decided by the kernel before any read;  phase_p its P list entries
//   hop    column 0 of the chunk's hop bytes under this key, hop_n how many of them exist;  ctr0 lane 0's counter at slot 0
//   pn     the eight PN bits of header bit tid & 15 under this key, MSB first
// Its counter at slot j is ctr0 + tid + j.  Per list entry and tile of CT slots: (1) every lane forms four of the tile's CT x 4 x 16 header
// sums Z from m and the key's header PN, and the tile's hop bytes and a, d go to LDS; (2) STRAIGHT false: (a + H) is tabulated per (slot,
// band, high byte) -- the block's counters at one slot are 256 consecutive values, so two high bytes whatever ctr0 is; (3) the lane adds
// its slot terms in ascending slot order.  STRAIGHT true is the definition written out, 17 signed adds per (origin, slot); both give the
// same bits, because a table entry is summed in the defined order.
template <bool STRAIGHT>
__device__ __forceinline__ void coherent_score_body(const double* __restrict__ m_p, const double* __restrict__ a_p, const double* __restrict__ d_p,
        long long mine, long long J, g_cu8* hop, long long hop_n, uint32_t ctr0, unsigned pn, const int32_t* __restrict__ phase_p, int P, bool live,
        long long origin, double* __restrict__ sc_score, long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    __shared__ double sh[CT * ES_NBANDS * CS_REC];
    __shared__ uint8_t hops[CO + CT];
    __shared__ hs_best red[CO];
    const int tid = threadIdx.x;
    __builtin_assume(J >= 0 && J <= 0x7FFFFFFFll / ES_FRAME_LEN);                          // both kernels clamp J so: the body is compiled before it is inlined
    // this lane's header sums of a tile: (slot, band) pair tid >> 4 and pair 16 .. 48 further on (the same band), header bit i = tid & 15
    const int zi = tid & 15;
    hs_best best = {-__builtin_inf(), -1, -1};
    #pragma unroll 1
    for (int p = 0; p < P; ++p) {
        const int phi = ((g_ci32*)phase_p)[p];
        if (phi < 0 || phi >= ES_FRAME_LEN || J == 0) continue;                           // (block-uniform) an entry that is no phase is not scored
        double acc = 0.0;
        bool ok = live;
        #pragma unroll 1
        for (long long j0 = 0; j0 < J; j0 += CT) {
            const int nt = (int)(J - j0 < CT ? J - j0 : CT);
            __syncthreads();                                                              // the tile before has been read
            #pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pair = (tid >> 4) + 16 * e, j = pair >> 2;                      // 64 pairs: slot j of the tile, band pair & 3 = (tid >> 4) & 3
                if (j < nt) {
                    const long long s = mine + phi + (j0 + j) * ES_FRAME_LEN;
                    const double* mm = m_p + s + COH_PRE + 8 * zi;
                    double z = 0.0;
                    #pragma unroll
                    for (int m = 0; m < 8; ++m) z = z + (((pn >> (7 - m)) & 1u) ? mm[m] : -mm[m]);
                    double* rec = sh + pair * CS_REC;
                    rec[CS_Z + zi] = z;
                    if (zi == 0) rec[CS_A] = a_p[s];
                    if (zi == 1) rec[CS_D] = d_p[s];
                }
            }
            for (int i = tid; i < CO + nt - 1; i += 256) hops[i] = j0 + i < hop_n ? hop[j0 + i] : (uint8_t)0xFF;
            __syncthreads();
            if (!STRAIGHT) {
                if (tid < 2 * 4 * nt) {                                                   // (slot, band, which of the two high bytes)
                    const int pair = tid >> 1, e = tid & 1;
                    double* rec = sh + pair * CS_REC;
                    const unsigned hi = (((ctr0 + (uint32_t)(j0 + (pair >> 2))) >> 8) + (unsigned)e) & 0xFFu;
                    rec[CS_AH + e] = rec[CS_A] + byte_sum(rec + CS_Z, hi);
                }
                __syncthreads();
            }
            if (live) {
                #pragma unroll 4                                                          // the terms of four slots in flight; acc still takes them in slot order
                for (int j = 0; j < nt; ++j) {
                    const unsigned h = hops[tid + j];
                    ok = ok && h < 4u;
                    const double* rec = sh + (4 * j + (int)(h & 3u)) * CS_REC;
                    const uint32_t base = ctr0 + (uint32_t)(j0 + j), c = base + (uint32_t)tid;
                    double num;
                    if (STRAIGHT) num = (rec[CS_A] + byte_sum(rec + CS_Z, (c >> 8) & 0xFFu)) + byte_sum(rec + CS_Z + 8, c & 0xFFu);
                    else num = rec[CS_AH + (int)(((c >> 8) - (base >> 8)) & 1u)] + byte_sum(rec + CS_Z + 8, c & 0xFFu);
                    const double den = rec[CS_D];
                    acc = acc + (den == 0.0 ? 0.0 : num / den);
                }
            }
        }
        const double s = acc / (double)J;
        if (ok && (best.origin < 0 || s > best.score)) { best.score = s; best.origin = origin; best.rank = p; }
    }
    hs_block_best(red, best, tid, sc_score, sc_origin, sc_rank);
}

// Clip b owns rows 4 b .. 4 b + 3 from column 0; one lo and one hop row per key serve the whole call.
template <bool STRAIGHT>
__global__ __launch_bounds__(256) void es_coherent_score_kernel(const double* __restrict__ m_p, const double* __restrict__ a_p,
        const double* __restrict__ d_p, long long T, const int32_t* __restrict__ nslot_p, const int32_t* __restrict__ phase_p, int P,
        const uint8_t* __restrict__ ring_p, const uint8_t* __restrict__ hop_p, long long K, long long Ccols, uint32_t lo, long long n_origins,
        long long NB, double* __restrict__ sc_score, long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x % NB, bk = blockIdx.x / NB, k = bk % K, b = bk / K;
    const long long origin = chunk * CO + tid;
    const long long J = coh_slots(nslot_p, b, T);
    g_cu8* hop = (g_cu8*)hop_p + k * Ccols + chunk * CO;                                   // columns chunk 256 + i, i < 256 + J - 1, exist where i < n_origins - chunk 256 + J - 1
    const long long hop_n = n_origins - chunk * CO + J - 1;                                // ... of them (<= Ccols - chunk 256: the entry point's check)
    const unsigned pn = ((g_cu8*)ring_p)[k * ES_KEYRING_BYTES + ES_COH_HDR_PN + (tid & 15)];
    coherent_score_body<STRAIGHT>(m_p, a_p, d_p, (4 * b + ((tid >> 4) & 3)) * T, J, hop, hop_n, lo + (uint32_t)(chunk * CO), pn, phase_p + b * P, P,
                                  origin < n_origins, origin, sc_score, sc_origin, sc_rank);
}

// The same over records that lie anywhere in the three tables (include/echoseal_coherent_at.h): record b names its four rows, its column,
// its hop row and the counter of that hop row's column 0.  Whether it is addressable, its J and its hop row are decided here, from the
// arrays alone and alike for the whole block, before anything of the tables or the hop bytes is read; J == 0 reads none of them.
struct es_coh_at { const long long* row; const long long* col; const int32_t* nslot; const int32_t* hop_row; const uint32_t* lo; long long rows, stride, Jw, HR; };

template <bool STRAIGHT>
__global__ __launch_bounds__(256) void es_coherent_score_at_kernel(const double* __restrict__ m_p, const double* __restrict__ a_p,
        const double* __restrict__ d_p, es_coh_at at, const int32_t* __restrict__ phase_p, int P, const uint8_t* __restrict__ ring_p,
        const uint8_t* __restrict__ hop_p, long long K, long long Ccols, long long n_origins, long long NB, double* __restrict__ sc_score,
        long long* __restrict__ sc_origin, long long* __restrict__ sc_rank)
{
    const int tid = threadIdx.x;
    const long long chunk = blockIdx.x % NB, bk = blockIdx.x / NB, k = bk % K, b = bk / K;
    const long long origin = chunk * CO + tid;
    const long long col = ((g_ci64*)at.col)[b], hr = ((g_ci32*)at.hop_row)[b];
    bool ok = col >= 0 && col <= at.stride && hr >= 0 && hr < at.HR;
    long long mine = 0;                                                                    // the row of the one band this lane stages
    #pragma unroll
    for (int band = 0; band < 4; ++band) {
        const long long q = ((g_ci64*)at.row)[4 * b + band];
        ok = ok && q >= 0 && q < at.rows;
        mine = ((tid >> 4) & 3) == band ? q : mine;
    }
    long long most = ok && at.stride - col > COH_SPAN ? (at.stride - col - COH_SPAN) / ES_FRAME_LEN : 0, J = ((g_ci32*)at.nslot)[b];
    most = most > at.Jw ? at.Jw : most;
    J = J < 0 ? 0 : (J > most ? most : J);
    mine = ok ? mine * at.stride + col : 0;                                               // (rows, stride < 2^31: the entry point's check)
    g_cu8* hop = (g_cu8*)hop_p + (k * at.HR + (ok ? hr : 0)) * Ccols + chunk * CO;         // hop_n <= Ccols - chunk 256: J <= Jw
    const long long hop_n = n_origins - chunk * CO + J - 1;
    const unsigned pn = ((g_cu8*)ring_p)[k * ES_KEYRING_BYTES + ES_COH_HDR_PN + (tid & 15)];
    coherent_score_body<STRAIGHT>(m_p, a_p, d_p, mine, J, hop, hop_n, ((g_cu32*)at.lo)[b] + (uint32_t)(chunk * CO), pn, phase_p + b * P, P,
                                  origin < n_origins, origin, sc_score, sc_origin, sc_rank);
}

}  // namespace

// the exact grids: the entry points refuse a call whose grid would pass 2^31 - 1 blocks, and hold tables_ready
int es_launch_mf_rows(es_ctx* ctx, const double* y, int64_t rows, int64_t T, const int32_t* len, const uint8_t* band, double* m, double* a,
                      double* d, hipStream_t st)
{
    const long long tiles = (T + MF_TILE - 1) / MF_TILE;
    mf_norm norm;
    for (int b = 0; b < ES_NBANDS; ++b) norm.c[b] = ctx->mf_norm[b];
    if (ctx->max_ntaps <= ES_MAX_TAPS_FAST)
        return es_launch(ctx, es_mf_rows_kernel<ES_MAX_TAPS_FAST>, (unsigned)(rows * tiles), 256, 0, st, y, (long long)T, len, band,
                         (const es_band_tables*)ctx->d_tables, norm, tiles, m, a, d);
    return es_launch(ctx, es_mf_rows_kernel<ES_MAX_TAPS>, (unsigned)(rows * tiles), 256, 0, st, y, (long long)T, len, band,
                     (const es_band_tables*)ctx->d_tables, norm, tiles, m, a, d);
}

#ifdef ES_COHERENT_STRAIGHT
constexpr bool COH_STRAIGHT = true;                                                        // A/B build (tools/build_variant.sh): the 17-add form
#else
constexpr bool COH_STRAIGHT = false;
#endif

int es_launch_coherent_score(es_ctx* ctx, const double* m, const double* a, const double* d, int64_t T, const int32_t* nslot, int64_t B,
                             const int32_t* phase, int P, const uint8_t* ring, const uint8_t* hop, int64_t K, int64_t Ccols, uint32_t lo,
                             int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st)
{
    const hs_scratch sc(scratch, B, K, n_origins);
    if (sc.slots > 0)
        if (const int rc = es_launch(ctx, es_coherent_score_kernel<COH_STRAIGHT>, (unsigned)sc.slots, 256, 0, st, m, a, d, (long long)T, nslot, phase,
                                     P, ring, hop, (long long)K, (long long)Ccols, lo, (long long)n_origins, sc.NB, sc.score, sc.origin, sc.rank))
            return rc;
    return es_launch_hop_best(ctx, sc, score, origin, rank, st);
}

int es_launch_coherent_score_at(es_ctx* ctx, const double* m, const double* a, const double* d, int64_t rows, int64_t stride, const int64_t* row,
                                const int64_t* col, const int32_t* nslot, int64_t B, int64_t Jw, const int32_t* phase, int P, const uint8_t* ring,
                                const uint8_t* hop, int64_t K, int64_t HR, int64_t Ccols, const int32_t* hop_row, const uint32_t* lo,
                                int64_t n_origins, double* score, int64_t* origin, int32_t* rank, void* scratch, hipStream_t st)
{
    const hs_scratch sc(scratch, B, K, n_origins);
    if (sc.slots > 0)
        if (const int rc = es_launch(ctx, es_coherent_score_at_kernel<COH_STRAIGHT>, (unsigned)sc.slots, 256, 0, st, m, a, d,
                                     es_coh_at{(const long long*)row, (const long long*)col, nslot, hop_row, lo, (long long)rows, (long long)stride,
                                               (long long)Jw, (long long)HR},
                                     phase, P, ring, hop, (long long)K, (long long)Ccols, (long long)n_origins, sc.NB, sc.score, sc.origin, sc.rank))
            return rc;
    return es_launch_hop_best(ctx, sc, score, origin, rank, st);
}
