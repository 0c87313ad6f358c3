/* echoseal_coherent_at.h -- companion of echoseal_hip.h: the keyed score of the coherent presence test (echoseal_coherent.h)
 * over records that lie anywhere in a table of rows -- the windows of a clip's presence timeline, each on its own columns of
 * the clip's four matched-filter rows, each with its own counters.  Same library, same conventions, same ES_ABI_VERSION (nothing of
 * echoseal_hip.h or of another companion changes); written in the vocabulary echoseal_amd/_native.py binds (bind_header), which reads this
 * file into tables of its own (COHERENT_AT_DECLARATIONS, COHERENT_AT_SIGNATURES, COHERENT_AT_CONSTANTS).
 *
 * Conventions: those of echoseal_coherent.h.  Everything is float64.  Every sum is added one term after the other in ascending order
 * starting from +0.0, by one lane from its first term to its last; a product is formed and then added; the counter's high and low byte
 * are summed apart.  A plain loop on the host gives the same bits (echoseal_amd/presence.py coherent_score_at_model).  No atomic decides
 * an order; two runs give the same bits.  The call only enqueues, takes no context workspace and can be captured. */
#ifndef ECHOSEAL_COHERENT_AT_H
#define ECHOSEAL_COHERENT_AT_H

#include "echoseal_coherent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* es_coherent_score_batch with the rows of each record named instead of implied, as es_warp_score_at_batch relates to
 * es_warp_score_batch.  m_dev, a_dev, d_dev [rows][stride] float64: the three tables es_mf_rows_batch writes.  Record b: row_dev[b][band]
 * (int64 [B][4]) the row that holds BAND_PLAN band `band`, col_dev[b] (int64 [B]) the column of its sample 0, nslot_dev[b] (int32 [B])
 * its slots.  The record is addressable iff all four rows lie in [0, rows) and 0 <= col <= stride.  Its J is nslot[b] clamped to
 * [0, min(Jw, max(0, stride - col - 190) / 1215)], and 0 where the record is not addressable or hop_row_dev[b] (int32 [B]) lies outside
 * [0, HR).  Both are decided from the arrays before any read: whatever the arrays hold, nothing outside columns
 * [col, col + 1215 J + 190) of the record's own four rows is read, and everything else of the three tables may hold anything, NaN
 * included.  Records may share rows and overlap.
 * phase_dev [B][P] int32, ring_dev: as for es_coherent_score_batch.  hop_dev [K][HR][Ccols] uint8 as es_hop_window_batch writes it: record b
 * reads hop row hop_row[b] of every key; lo_dev[b] (uint32 [B]) must be the counter of column 0 of that hop row -- the caller keeps the
 * two consistent, the call does not check it.  For key row k, origin o in [0, n_origins), list entry p with phi = phase[b][p], slot j < J:
 *     c = lo[b] + o + j (uint32),  band = hop[k][hop_row[b]][o + j],  s = col[b] + phi + 1215 j in the rows row[b][band]
 * and Z_i, N, R, S exactly as in echoseal_coherent.h.  What is not scored (a hop byte above 3 in the origin's window, an entry outside
 * 0 .. 1214, J == 0), the outputs score_dev [B][K], origin_dev [B][K], rank_dev [B][K], the tie rules (lowest origin, then earliest
 * entry), (-inf, -1, -1), the scratch contract (24 * B * K * ceil(n_origins / ES_HOP_ORIGINS) bytes, 8-byte aligned) and the second
 * launch that reduces the workgroups' bests are that header's.  One workgroup per (record, key, ES_HOP_ORIGINS origins), the same device
 * body as es_coherent_score_batch: with row[b][band] = 4 b + band, col = 0, HR = 1, hop_row = 0, lo_dev[b] = lo and Jw >= every J the
 * outputs are its bits.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows or stride > 2^31 - 1, P outside 1 .. 1215, HR < 1 or
 * HR > 2^31 - 1, Jw < 0, Ccols < n_origins + Jw - 1, B * K * ceil(n_origins / ES_HOP_ORIGINS) > 2^31 - 1 workgroups (the grid is exact),
 * a null pointer with work to do.  B * K == 0: ES_OK, nothing enqueued, nothing written. */
int es_coherent_score_at_batch(es_ctx* ctx, const double* m_dev, const double* a_dev, const double* d_dev, int64_t rows, int64_t stride,
                               const int64_t* row_dev, const int64_t* col_dev, const int32_t* nslot_dev, int64_t B, int64_t Jw,
                               const int32_t* phase_dev, int P, const uint8_t* ring_dev, const uint8_t* hop_dev, int64_t K, int64_t HR,
                               int64_t Ccols, const int32_t* hop_row_dev, const uint32_t* lo_dev, int64_t n_origins, double* score_dev,
                               int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_COHERENT_AT_H */
