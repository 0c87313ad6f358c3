/* echoseal_pick.h -- companion of echoseal_live_presence.h: the pick of a presence test's hypotheses on the device, what
 * presence.pick_hypotheses does on the host after a download of the whole fold.  Same library, same conventions, same ES_ABI_VERSION
 * (nothing of echoseal_hip.h, echoseal_presence.h, echoseal_warp.h or echoseal_live_presence.h changes); written in the vocabulary
 * echoseal_amd/_native.py binds (bind_header), which reads this file into tables of its own (PICK_DECLARATIONS, PICK_SIGNATURES,
 * PICK_CONSTANTS).
 *
 * Definition.  fold_dev [B][D][1215] float64 is what es_warp_fold_batch / es_warp_fold_at_batch write (with D = 1 also what
 * es_phase_fold_batch writes).  nwarp_dev [B] int32 says how many of a record's D rows are its own: null means D for every record,
 * otherwise the value is clamped to [0, D].  Rows at or past nwarp[b] are never read and may hold anything.
 * The CANDIDATES of record b are the pairs (d, phi), d < nwarp[b], phi in 0 .. 1214, whose value fold[b][d][phi] is neither -inf nor a
 * NaN: a NaN is never picked, whatever its sign or payload (a fold of finite samples holds none).  +inf is a candidate like any other
 * value.  Entry h of the record's list is the candidate of h-th largest value; candidates of equal value are ordered by the lower d,
 * then the lower phi, and -0.0 == +0.0 counts as equal.  The list is H entries long:
 *     hyp_dev [B][H][2] int32     entry h = (d, phi); (-1, -1) from the first entry past the record's last candidate
 *     val_dev [B][H] float64      the value of entry h as the fold holds it (a -0.0 stays -0.0); -inf beside (-1, -1).  May be null.
 * For a fold whose rows are each all -inf or wholly finite -- every fold of the public calls -- the list is
 * presence.pick_hypotheses(fold[b, :nwarp[b]], H), padded with (-1, -1): the form es_warp_score_batch / es_warp_score_at_batch take as
 * "an entry that names nothing".  presence.pick_model is the host twin for any fold.
 * One workgroup per record.  Each value becomes a 96-bit key, its order-preserving integer image above the complement of
 * d 1215 + phi, so the keys of a record are distinct and entry h is the largest key strictly below entry h - 1's: H rounds of a pure
 * maximum, whose reduction shape does not matter.  No atomic, no sort; two runs give the same bits.  The call needs no tables and no
 * context workspace, only enqueues, and can be captured. */
#ifndef ECHOSEAL_PICK_H
#define ECHOSEAL_PICK_H

#include "echoseal_live_presence.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ES_PICK_MAX_H 64                /* the longest list of one call */

/* ES_EINVAL, with nothing enqueued and nothing written: a negative count, H outside 1 .. ES_PICK_MAX_H, B > 2^31 - 1 (a workgroup per
 * record, the grid is exact), 1215 D > 2^31 - 1 (d 1215 + phi is a 32-bit word of the key), a null fold_dev or hyp_dev with work to do.
 * B * D == 0: ES_OK, nothing enqueued and NOTHING WRITTEN -- also for D == 0 with B > 0, where every list would be empty: a call
 * without work touches no memory, as for the folds; RxEngine.fold_pick fills the outputs of such a call itself. */
int es_fold_pick_batch(es_ctx* ctx, const double* fold_dev, int64_t B, int64_t D, const int32_t* nwarp_dev, int64_t H, int32_t* hyp_dev,
                       double* val_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_PICK_H */
