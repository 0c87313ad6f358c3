/* echoseal_presence.h -- companion of echoseal_hip.h: the C ABI of the presence test, "do the preamble peaks of this clip
 * sit on one 1215-sample grid and follow this key's band-hop sequence from some counter?".  Same library, same conventions, same
 * ES_ABI_VERSION (nothing of echoseal_hip.h changes); written in the vocabulary echoseal_amd/_native.py binds (bind_header), which reads
 * this file into tables of its own (PRESENCE_DECLARATIONS, PRESENCE_SIGNATURES, PRESENCE_CONSTANTS).
 *
 * Definition.  Clip b of a call owns rows 4 b .. 4 b + 3 of corr_dev [rows][stride] float64: row 4 b + band holds the es_xcorr_batch
 * (or es_sync_ragged_batch) correlation row of the band with BAND_PLAN index `band`, lags [0, nlag), nlag = nlag_dev[b] clamped to
 * [0, stride] (int32 [B]: the clip's samples - 62).  J = nlag / 1215 is the clip's number of whole slots.  Columns at or past nlag may hold
 * anything, NaN included: they are never read.  Finite values only in the columns that are.  Every sum below is float64, added one term
 * after the other in ascending slot order starting from +0.0, by one lane from its first term to its last, without FMA and without any
 * pairwise or tree shape: a plain loop on the host gives the same bits (echoseal_amd/presence.py fold_model, score_model).  No atomic
 * decides an order; two runs give the same bits.  Both calls need no tables and no context workspace, only enqueue, and can be captured. */
#ifndef ECHOSEAL_PRESENCE_H
#define ECHOSEAL_PRESENCE_H

#include "echoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The keyless fold: fold_dev [B][1215] float64,
 *     fold[b][phi] = sum_{j < J} max_band corr[4 b + band][phi + 1215 j],       phi in 0 .. 1214
 * (the maximum taken band 0 first, a later band replacing it only where strictly larger).  J == 0 writes a row of zeros.  Picking the
 * phases of largest fold is host work.
 * ES_EINVAL, with nothing enqueued: a negative count, rows < 4 B, stride > 2^31 - 1, 5 B > 2^31 - 1 (five workgroups per clip: the grid is
 * exact), a null pointer with B > 0.  B == 0: ES_OK, nothing enqueued. */
int es_phase_fold_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                        double* fold_dev, void* stream);

/* The keyed score.  phase_dev [B][P] int32: the phase list of each clip, 1 <= P <= 1215; hop_dev [K][Ccols] uint8: column i of row k is
 * the band of counter lo + i under key row k, as es_hop_window_batch writes it with HR = 1 and hop_base = lo (0xFF: the counter does not
 * exist).  For key row k, origin i in [0, n_origins) and list entry p with phi = phase[b][p]:
 *     S(k, i, p) = (sum_{j < J} corr[4 b + hop[k][i + j]][phi + 1215 j]) / J
 * An origin whose window hop[k][i .. i + J - 1] holds a byte above 3 is not scored, nor is a list entry outside 0 .. 1214.  Out, per
 * (clip, key): score_dev [B][K] float64 the largest S, origin_dev [B][K] int64 its origin i and rank_dev [B][K] int32 its list entry p;
 * of equal scores the lowest origin wins, then the earliest list entry.  Nothing scored (J == 0 among the reasons): -inf, -1, -1.
 * One workgroup per (clip, key, ES_HOP_ORIGINS origins), one lane per origin; the [J][4] values of one phase pass through LDS in tiles
 * of ES_HOP_TILE slots.  The workgroups' bests are reduced by a second launch, chunks ascending, through scratch_dev: caller-provided,
 * 8-byte aligned, 24 * B * K * ceil(n_origins / ES_HOP_ORIGINS) bytes (may be NULL where that is 0), contents unspecified afterwards.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows < 4 B, stride > 2^31 - 1, P outside 1 .. 1215,
 * Ccols < n_origins + Jmax - 1 with Jmax = stride / 1215 (the most slots a clamped nlag can give), B * K * ceil(n_origins /
 * ES_HOP_ORIGINS) > 2^31 - 1 workgroups (the grid is exact), a null pointer with work to do.  B * K == 0: ES_OK, nothing enqueued. */
#define ES_HOP_TILE      64
#define ES_HOP_ORIGINS  256
int es_hop_score_batch(es_ctx* ctx, const double* corr_dev, int64_t rows, int64_t stride, const int32_t* nlag_dev, int64_t B,
                       const int32_t* phase_dev, int P, const uint8_t* hop_dev, int64_t K, int64_t Ccols, int64_t n_origins,
                       double* score_dev, int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_PRESENCE_H */
