/* echoseal_coherent.h -- companion of echoseal_hip.h: the C ABI of the coherent presence test, "does this clip carry, on one
 * 1215-sample grid, frame starts whose 63 preamble chips AND 128 keyed header chips are those of this key from some counter?".  Same
 * library, same conventions, same ES_ABI_VERSION (nothing of echoseal_hip.h changes); written in the vocabulary echoseal_amd/_native.py
 * binds (bind_header), which reads this file into tables of its own (COHERENT_DECLARATIONS, COHERENT_SIGNATURES, COHERENT_CONSTANTS).
 *
 * Conventions (those of echoseal_presence.h).  Everything is float64.  Every sum is added one term after the other in the stated ascending
 * order starting from +0.0, by one lane from its first term to its last; a product is formed and then added: no FMA, no pairwise or tree
 * shape.  A plain loop on the host gives the same bits (echoseal_amd/presence.py mf_rows_model, coherent_score_model).  No atomic decides
 * an order; two runs give the same bits.  Both calls only enqueue, take no context workspace and can be captured.
 *
 * Tables: the context's (es_set_tables).  For band b: L_b = ntaps[b], g_b[i] = (double)taps[b][L_b - 1 - i] the matched filter in forward
 * order, c_b = sqrt(191 * sum_{i < L_b} g_b[i]^2) (the sum in ascending i), W_b = 190 + L_b. */
#ifndef ECHOSEAL_COHERENT_H
#define ECHOSEAL_COHERENT_H

#include "echoseal_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The keyless rows.  Record r = the first n samples of row r of y_dev [rows][T] float64 (a band-passed record, as es_bpf_batch or
 * es_sync_ragged_batch writes it), n = len_dev[r] clamped to [0, T] (int32 [rows]), on band band_dev[r] (uint8 [rows], 0 .. 3: its
 * BAND_PLAN index).  Nothing of y at or past n is read; it may hold anything, NaN included.  Out, rows of T float64 each:
 *     m[r][t] = sum_{i < L} y[r][t + i] g[i]                          for t + L <= n
 *     a[r][s] = sum_{q < 63} p_q m[r][s + q]                          for s + W <= n      (p_q = +-1: the preamble symbols)
 *     d[r][s] = sqrt(sum_{k < W} y[r][s + k]^2) c                     for s + W <= n
 * and nothing anywhere else: an element that is not defined keeps what it held.  A record whose band byte is above 3 writes nothing.
 * One workgroup per (record, tile of ES_MF_TILE outputs), one lane per output, adjacent lanes on adjacent lags; the taps and the tile's
 * samples pass through LDS.  Serves every tap count es_set_tables admits (the small instantiation up to ES_MAX_TAPS_FAST taps, the large
 * one up to ES_MAX_TAPS).
 * ES_ENOTREADY before es_set_tables.  ES_EINVAL, with nothing enqueued and nothing written: a negative count, T > 2^31 - 1,
 * rows * ceil(T / ES_MF_TILE) > 2^31 - 1 workgroups (the grid is exact), a null pointer with work to do.  rows == 0 or T == 0: ES_OK,
 * nothing enqueued. */
#define ES_MF_TILE     256
int es_mf_rows_batch(es_ctx* ctx, const double* y_dev, int64_t rows, int64_t T, const int32_t* len_dev, const uint8_t* band_dev,
                     double* m_dev, double* a_dev, double* d_dev, void* stream);

/* The keyed score.  Clip b of a call owns rows 4 b .. 4 b + 3 of m_dev, a_dev, d_dev [rows][T], row 4 b + band the rows of BAND_PLAN
 * index `band`; J = nslot_dev[b] (int32 [B]) clamped to [0, max(0, T - 190) / 1215], so that no index below can pass a row -- the caller
 * names a J whose starts are all defined, J = max(0, n - 189 - L_max) / 1215 for a clip of n samples.  phase_dev [B][P] int32: the phase
 * list of each clip, 1 <= P <= 1215.  ring_dev: K key-ring rows (es_keyring_derive_batch); u_k[q] = +-1 from bit q (MSB first) of the
 * 128 header PN bits at byte ES_COH_HDR_PN of row k.  hop_dev [K][Ccols] uint8: column i of row k is the band of counter lo + i under
 * key row k, as es_hop_window_batch writes it with HR = 1 and hop_base = lo (0xFF: the counter does not exist); lo is the counter of
 * column 0.  For key row k, origin o in [0, n_origins), list entry p with phi = phase[b][p], and slot j < J:
 *     c = lo + o + j,  band = hop[k][o + j],  s = phi + 1215 j,  v = c & 0xFFFF,  sigma_i = 2 ((v >> (15 - i)) & 1) - 1
 *     Z_i = sum_{m < 8} u_k[8 i + m] m[4 b + band][s + 63 + 8 i + m]                                   i = 0 .. 15
 *     N   = (a[4 b + band][s] + sum_{i < 8} sigma_i Z_i) + sum_{i = 8 .. 15} sigma_i Z_i
 *     R   = N / d[4 b + band][s],  +0.0 where d is 0
 *     S(k, o, p) = (sum_{j < J} R) / J
 * (the counter's high and low byte are summed apart so that either sum may be tabulated per byte without changing a bit).  An origin
 * whose window hop[k][o .. o + J - 1] holds a byte above 3 is not scored, nor is a list entry outside 0 .. 1214.  Out, per (clip, key):
 * score_dev [B][K] float64 the largest S, origin_dev [B][K] int64 its origin o and rank_dev [B][K] int32 its list entry p; of equal
 * scores the lowest origin wins, then the earliest list entry.  Nothing scored (J == 0 among the reasons): -inf, -1, -1.
 * One workgroup per (clip, key, ES_HOP_ORIGINS origins), one lane per origin; what the lanes of a list entry share passes through LDS in
 * tiles of ES_COH_TILE slots.  The workgroups' bests are reduced by a second launch, chunks ascending, through scratch_dev: the contract
 * of es_hop_score_batch -- caller-provided, 8-byte aligned, 24 * B * K * ceil(n_origins / ES_HOP_ORIGINS) bytes (may be NULL where that
 * is 0), contents unspecified afterwards.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, rows < 4 B, T > 2^31 - 1, P outside 1 .. 1215,
 * Ccols < n_origins + Jmax - 1 with Jmax = max(0, T - 190) / 1215 (the most slots a clamped nslot can give),
 * B * K * ceil(n_origins / ES_HOP_ORIGINS) > 2^31 - 1 workgroups (the grid is exact), a null pointer with work to do.  B * K == 0: ES_OK,
 * nothing enqueued. */
#define ES_COH_TILE      16
#define ES_COH_HDR_PN   272
int es_coherent_score_batch(es_ctx* ctx, const double* m_dev, const double* a_dev, const double* d_dev, int64_t rows, int64_t T,
                            const int32_t* nslot_dev, int64_t B, const int32_t* phase_dev, int P, const uint8_t* ring_dev,
                            const uint8_t* hop_dev, int64_t K, int64_t Ccols, uint32_t lo, int64_t n_origins, double* score_dev,
                            int64_t* origin_dev, int32_t* rank_dev, void* scratch_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_COHERENT_H */
