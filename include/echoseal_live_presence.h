/* echoseal_live_presence.h -- companion of echoseal_warp.h: the presence test over records that lie anywhere in a table of correlation
 * rows, such as the windows of live streams in a monitor table's corr_hist.  Same library, same conventions, same
 * ES_ABI_VERSION (nothing of echoseal_hip.h, echoseal_presence.h or echoseal_warp.h changes); written in the vocabulary
 * echoseal_amd/_native.py binds (bind_header), which reads this file into tables of its own (LIVE_PRESENCE_DECLARATIONS,
 * LIVE_PRESENCE_SIGNATURES, LIVE_PRESENCE_CONSTANTS).
 *
 * Definition.  es_warp_fold_at_batch / es_warp_score_at_batch are es_warp_fold_batch / es_warp_score_batch with the rows of record b
 * named instead of implied.  corr_dev [rows][stride] float64 is a table of rows, and per record b
 *     row_dev [B][4] int64           row_dev[b][band]: the row that holds BAND_PLAN band `band` of the record
 *     col_dev [B] int64              the column of the record's lag 0
 *     nlag_dev [B] int32             its lags
 * Record b is ADDRESSABLE iff all four rows lie in [0, rows) and 0 <= col <= stride.  Its nlag is nlag_dev[b] clamped to
 * [0, stride - col]; a record that is not addressable has nlag = 0.  The kernels decide this from the three arrays before any read:
 * whatever they hold, no element outside columns [col, col + nlag) of the record's own four rows is read -- columns before col are not
 * read either -- and everything else of the table may hold anything, NaN included.  Two records may share rows and overlap.  Lag i of band
 * `band` of record b is corr[row[b][band]][col[b] + i]; with that, the warp table (warp_dev, nwarp_dev, nslot_dev, D, Jw), the rule by
 * which a row of it is usable, "judged slot by slot before the slot is read", and the summation rule are those of echoseal_warp.h: every
 * sum is float64, added one term after the other in ascending slot order starting from +0.0, by one lane from its first term to its
 * last, without FMA and without any tree shape (echoseal_amd/presence.py: window_rows, then warp_fold_model / warp_score_model, give
 * the same bits).
 * Identities.  With row[b][band] = 4 b + band, col = 0, HR = 1 and hop_row = 0 both calls give the bits of es_warp_fold_batch /
 * es_warp_score_batch; with additionally D = 1, a table of zeros and nslot = nlag / 1215, the bits of es_phase_fold_batch /
 * es_hop_score_batch.
 * No atomic decides an order; two runs give the same bits.  Both calls need no tables and no context workspace, only enqueue, and can
 * be captured. */
#ifndef ECHOSEAL_LIVE_PRESENCE_H
#define ECHOSEAL_LIVE_PRESENCE_H

#include "echoseal_warp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The keyless fold along every row of the table: fold_dev [B][D][1215] float64,
 *     fold[b][d][phi] = sum_{j < J} max_band corr[row[b][band]][col[b] + phi + 1215 j + warp[b][d][j]],       phi in 0 .. 1214
 * (the maximum taken band 0 first, a later band replacing it only where strictly larger).  An unusable row is all -inf; J == 0 (a record
 * that is not addressable included) writes zeros to the usable rows.  One lane per (record, row, phase), five workgroups per (record,
 * row); the row of offsets passes through LDS.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows or stride > 2^31 - 1, 5 B D > 2^31 - 1 workgroups (the
 * grid is exact), a null pointer with work to do.  B * D == 0: ES_OK, nothing enqueued. */
int es_warp_fold_at_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int64_t* row_dev, const int64_t* col_dev,
                          const int32_t* nlag_dev, int64_t B, const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev,
                          int64_t D, int64_t Jw, double* fold_dev, void* stream);

/* The keyed score along a list of hypotheses.  hyp_dev [B][H][2] int32 as for es_warp_score_batch.  hop_dev [K][HR][Ccols] uint8 as
 * es_hop_window_batch writes it, and hop_row_dev [B] int32: record b reads hop row hop_row[b] of every key,
 *     hop(k, b, i) = hop_dev[(k HR + hop_row[b]) Ccols + i]
 *     S(k, i, h)   = (sum_{j < J} corr[row[b][hop(k, b, i + j)]][col[b] + phi_h + 1215 j + warp[b][d_h][j]]) / J
 * so streams at different counters share one launch, each with the hop row of its own span base.  A hop_row outside [0, HR) scores
 * nothing for the record (-inf, -1, -1), and nothing of the record is read.  What is not scored otherwise, the three outputs
 * (score_dev [B][K] float64, origin_dev [B][K] int64, rank_dev [B][K] int32), the tie rules, the blocking by ES_WARP_HB entries and
 * the scratch contract (caller-provided, 8-byte aligned, 24 * B * K * ceil(n_origins / ES_HOP_ORIGINS) bytes, reduced by the second
 * launch of es_hop_score_batch, contents unspecified afterwards) are es_warp_score_batch's.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows or stride > 2^31 - 1, H < 1, H or D above 2^31 - 1,
 * HR < 1, HR above 2^31 - 1, Ccols < n_origins + Jw - 1, B * K * ceil(n_origins / ES_HOP_ORIGINS) > 2^31 - 1 workgroups (the grid is
 * exact), a null pointer with work to do.  B * K == 0: ES_OK, nothing enqueued. */
int es_warp_score_at_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int64_t* row_dev, const int64_t* col_dev,
                           const int32_t* nlag_dev, int64_t B, const int32_t* warp_dev, const int32_t* nwarp_dev, const int32_t* nslot_dev,
                           int64_t D, int64_t Jw, const int32_t* hyp_dev, int64_t H, const uint8_t* hop_dev, int64_t K, int64_t HR,
                           int64_t Ccols, const int32_t* hop_row_dev, int64_t n_origins, double* score_dev, int64_t* origin_dev,
                           int32_t* rank_dev, void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_LIVE_PRESENCE_H */
