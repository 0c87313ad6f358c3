/* echoseal_warp.h -- companion of echoseal_presence.h: the presence test on a frame grid that follows sample-clock drift.
 * Same library, same conventions, same ES_ABI_VERSION (nothing of echoseal_hip.h or echoseal_presence.h changes); written in the
 * vocabulary echoseal_amd/_native.py binds (bind_header), which reads this file into tables of its own (WARP_DECLARATIONS,
 * WARP_SIGNATURES, WARP_CONSTANTS).
 *
 * Definition.  The rows, nlag and the summation rule are those of echoseal_presence.h: clip b owns rows 4 b .. 4 b + 3 of corr_dev
 * [rows][stride] float64, lags [0, nlag), nlag = nlag_dev[b] clamped to [0, stride]; every sum is float64, added one term after the other
 * in ascending slot order starting from +0.0, by one lane from its first term to its last, without FMA and without any tree shape
 * (echoseal_amd/presence.py warp_fold_model, warp_score_model give the same bits).  What is new is a table of per-slot sample offsets:
 *     warp_dev [B][D][Jw] int32      row d of clip b: slot j of the frame grid starts warp[b][d][j] samples after 1215 j
 *     nwarp_dev [B] int32            the rows of clip b (rows at or past it are unusable)
 *     nslot_dev [B] int32            J, the slots of clip b that are summed, clamped to [0, min(Jw, nlag / 1215)]
 * Row d of clip b is USABLE iff d < nwarp[b] and, for every j < J, 0 <= 1215 j + warp[b][d][j] and 1215 j + warp[b][d][j] + 1214 < nlag.
 * The kernels decide that from the table themselves, slot by slot before the slot is read: whatever the table holds, no column outside
 * [0, nlag) is ever read, and columns at or past nlag may hold anything, NaN included.  Entries of a row at or past J are not read.
 * With D = 1, a table of zeros and nslot = nlag / 1215 both calls give the bits of es_phase_fold_batch / es_hop_score_batch.
 * No atomic decides an order; two runs give the same bits.  Both calls need no tables and no context workspace, only enqueue, and can
 * be captured. */
#ifndef ECHOSEAL_WARP_H
#define ECHOSEAL_WARP_H

#include "echoseal_presence.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The keyless fold along every row of the table: fold_dev [B][D][1215] float64,
 *     fold[b][d][phi] = sum_{j < J} max_band corr[4 b + band][phi + 1215 j + warp[b][d][j]],       phi in 0 .. 1214
 * (the maximum taken band 0 first, a later band replacing it only where strictly larger).  An unusable row is all -inf; J == 0 writes
 * zeros to the usable rows.  One lane per (clip, row, phase), five workgroups per (clip, row); the row of offsets passes through LDS.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows < 4 B, stride > 2^31 - 1, 5 B D > 2^31 - 1 workgroups
 * (the grid is exact), a null pointer with work to do.  B * D == 0: ES_OK, nothing enqueued. */
int es_warp_fold_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                       const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev, int64_t D, int64_t Jw,
                       double* fold_dev, void* stream);

/* The keyed score along a list of hypotheses.  hyp_dev [B][H][2] int32: entry h of clip b is (d, phi), a row of the table and a phase;
 * hop_dev [K][Ccols] uint8 as for es_hop_score_batch.  For key row k, origin i in [0, n_origins) and entry h:
 *     S(k, i, h) = (sum_{j < J} corr[4 b + hop[k][i + j]][phi_h + 1215 j + warp[b][d_h][j]]) / J
 * Not scored: an entry whose row is unusable (d outside 0 .. D - 1 included) or whose phi lies outside 0 .. 1214; an origin whose window
 * hop[k][i .. i + J - 1] holds a byte above 3; anything where J == 0.  Out, per (clip, key): score_dev [B][K] float64 the largest S,
 * origin_dev [B][K] int64 its origin and rank_dev [B][K] int32 its list entry h; of equal scores the lowest origin wins, then the
 * earliest entry.  Nothing scored: -inf, -1, -1.
 * One workgroup per (clip, key, ES_HOP_ORIGINS origins), one lane per origin.  The list is taken ES_WARP_HB entries at a time: per
 * tile of ES_HOP_TILE slots the block's [ES_WARP_HB][ES_HOP_TILE][4] values pass through LDS and a lane reads each hop byte of its
 * window once for the whole block, one accumulator per entry in registers; each (origin, entry) sum still runs in ascending slot
 * order.  The workgroups' bests are reduced by the second launch of es_hop_score_batch through scratch_dev, under that call's
 * contract: caller-provided, 8-byte aligned, 24 * B * K * ceil(n_origins / ES_HOP_ORIGINS) bytes (may be NULL where that is 0),
 * contents unspecified afterwards.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows < 4 B, stride > 2^31 - 1, H < 1, H or D above
 * 2^31 - 1, Ccols < n_origins + Jw - 1, B * K * ceil(n_origins / ES_HOP_ORIGINS) > 2^31 - 1 workgroups (the grid is exact), a null
 * pointer with work to do.  B * K == 0: ES_OK, nothing enqueued.
 * (ES_WARP_HB may be given on the compiler's command line for an A/B build of es_keyring.hip: 1 is the loop of es_hop_score_batch
 * along the table, which the blocked form was measured against.  The bits do not depend on it.) */
#ifndef ES_WARP_HB
#define ES_WARP_HB  8
#endif
int es_warp_score_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                        const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev, int64_t D, int64_t Jw,
                        const int32_t* hyp_dev, int64_t H, const uint8_t* hop_dev, int64_t K, int64_t Ccols, int64_t n_origins,
                        double* score_dev, int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_WARP_H */
