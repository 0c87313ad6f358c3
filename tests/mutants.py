"""Value-only mutants of the device code, and the GPU tests expected to fail on each.

An entry replaces `old`, a text that occurs exactly once in `file` (under echoseal_amd/csrc/), by `new`; tools/mutant_audit.py builds a
library per entry (echoseal_amd/libechoseal_hip_<id>.so, loaded through ES_LIB_VARIANT) and runs the `killers` against it: they must fail.
`why` is the one-sentence argument that the change is value-only: the mutated expression changes a value, or a choice among values the
unmutated code already proves in range, and feeds no subscript, pointer, trip count, barrier, launch geometry or LDS size, removes no
guard of a memory access and touches no atomic's address -- so the mutant can neither fault nor hang nor run longer than the original.
`equivalent` (at most three entries) is the written argument that no input changes any output; such an entry is built and run but is
allowed to survive.  tests/test_mutants_listed.py holds the table to the sources and to the suite.  SCL_MUTANTS, further down, is a second
table of the same kind for the list decoders.

An entry in a header or body file counts for every translation unit that includes it (kernel_units in test_mutants_listed.py).

A plain helper module: no fixtures, nothing pytest collects."""
from collections import namedtuple

Mutant = namedtuple("Mutant", "id file old new killers why equivalent", defaults=(None,))

_SCREEN = "tests/test_gpu_sync_screen.py"
_FRONT = "tests/test_gpu_front_edges.py"
_EDGES = "tests/test_gpu_decision_edges.py"
_PARITY = "tests/test_gpu_parity.py"

# killer sets, shared so that the runner measures each set once on the unmutated library
PICK = (_SCREEN + "::test_float64_path", _PARITY + "::test_pick_threshold_saturation_shortcut",
        _PARITY + "::test_edge_records")
S32 = (_SCREEN + "::test_worst_case_screens", _SCREEN + "::test_non_finite_screens",
       _SCREEN + "::test_own_screens")
XCORR = (_SCREEN + "::test_float64_path",)
BPF = (_PARITY + "::test_bandpass_bits_all_kernels", "tests/test_gpu_ragged.py::test_sync_ragged_equals_per_record_sync_and_oracle")
LLR = (_FRONT + "::test_every_payload_length", _FRONT + "::test_degenerate_content",
       _PARITY + "::test_llr_shift_search_screen_is_exact")
HDR = (_EDGES + "::test_header_margin_of_exactly_one_half", _EDGES + "::test_header_guard_floor_decides_the_shift",
       _FRONT + "::test_header_device_filling", _FRONT + "::test_every_payload_length",
       _FRONT + "::test_degenerate_content")
PLAN = (_EDGES + "::test_plan_header_gate_above_0x7fff", "tests/test_gpu_identify.py::test_plan_kernel_equals_reference_on_random_scans",
        "tests/test_gpu_ragged.py::test_plan_ragged_equals_reference_and_per_row_plan")
PLAN_AT = (_EDGES + "::test_plan_at_last_counter_in_the_narrow_window", "tests/test_gpu_counters.py::test_plan_at_equals_the_twin",)
HOP = ("tests/test_gpu_counters.py::test_hop_window_equals_band_index", "tests/test_gpu_grid_stride.py::test_hop_window_past_the_cap")
ACQ = (_EDGES + "::test_acquire_span_ends", "tests/test_gpu_acquire.py::test_mask_and_list_equal_the_twin",)
AEAD = (_EDGES + "::test_validator_rejects_every_single_bit_of_the_counter", "tests/test_gpu_aead_edges.py::test_validator_edges", "tests/test_gpu_aead_edges.py::test_select_edges",
        _PARITY + "::test_select_kernel_vs_oracle_and_host_rules")
MEMO = ("tests/test_gpu_memo.py::test_three_inserts_with_probes_between_equal_the_twin",)
SCHED = (_PARITY + "::test_schedule_kernel_vs_oracle",)
TX = (_EDGES + "::test_frame_generator_peak_of_exactly_three", "tests/test_gpu_grid_stride.py::test_frame_generator_rescale_branch",
      _PARITY + "::test_frame_generator_equals_host_embedder")
MIX = ("tests/test_gpu_embed.py::test_mix_equals_fixture_and_host_process",
       "tests/test_gpu_embed.py::test_mix_random_sweep_against_host",
       "tests/test_gpu_embed.py::test_mix_many_recordings_in_place_and_special_values")
RES = ("tests/test_gpu_resample_ragged.py::test_kernel_equals_scipy_bit_for_bit",
       "tests/test_gpu_resample_arms.py::test_resample_batches_of_other_sample_types_equal_scipy")
SCL = ("tests/test_gpu_scl_leaf_pairs.py::test_lists_equal_oracle",
       _PARITY + "::test_scl_all_list_sizes_vs_oracle", _PARITY + "::test_scl_multi_frames_per_wave",
       _PARITY + "::test_scl_wide_lists_vs_oracle")

_V = "A comparison or constant inside a value computation: "

MUTANTS = [
    # ---- es_pick_body.inc: the float64 threshold / peak kernel (three forms, compiled into es_sync.hip)
    Mutant("pick_cand_strict", "es_pick_body.inc", "(i < n) && !(c[i] < thr);", "(i < n) && (c[i] > thr);", PICK,
           _V + "the candidate flag of a lag already inside the row; candidates are stored under the untouched total < ES_MAX_PEAKS guard."),
    Mutant("pick_suppress_ge", "es_pick_body.inc", "bigger |= (c[j] > cv);", "bigger |= (c[j] >= cv);", PICK,
           _V + "the rival flag read over the same clamped lag window; it only decides whether a candidate is kept."),
    Mutant("pick_fallback_tie_lane", "es_pick_body.inc", "(ci == bv && i > bidx)", "(ci == bv && i < bidx)", PICK,
           _V + "which of two equal lags of the row a lane keeps; both indices are lags of the row and are stored, never used as subscripts beyond the equality test with s_taken."),
    Mutant("pick_fallback_tie_lds", "es_pick_body.inc", "(ov == mv && oi > mi)", "(ov == mv && oi < mi)", PICK,
           _V + "which of two equal (value, lag) pairs survives a reduction step; the LDS indices of the reduction are untouched."),
    Mutant("pick_cap", "es_pick_body.inc", "if (0.95 < thr) thr = 0.95;", "if (0.96 < thr) thr = 0.96;", PICK,
           _V + "the cap of the threshold, a float64 that is only compared with correlations and stored."),
    Mutant("pick_mad_scale", "es_pick_body.inc", "4.5 * 1.4826 * mad", "4.5 * 1.4827 * mad", PICK,
           _V + "the MAD's factor in the threshold, a float64 that is only compared with correlations and stored."),
    Mutant("pick_mad_eps", "es_pick_body.inc", "&s_pref, &s_k) + 1e-12;", "&s_pref, &s_k) + 1e-11;", PICK,
           _V + "the addend of the MAD, which enters the threshold alone."),
    # ---- es_llr.hip: the demodulator
    Mutant("llr_tail_guard", "es_llr.hip", "(n > guard + 8) ? guard : 0;", "(n >= guard + 8) ? guard : 0;", LLR,
           "Chooses between the two tail offsets 0 and guard, both of which the unmutated code uses with guard < n, so the tail "
           "[toff, n) stays inside the despread row and no longer than n."),
    Mutant("llr_mad_scale", "es_llr.hip", "const double sigma_mad = 1.4826 * mad;", "const double sigma_mad = 1.4827 * mad;", LLR,
           _V + "sigma, which only scales the stored LLRs."),
    Mutant("llr_sigma_floor", "es_llr.hip", "if (0.1 > sigma) sigma = 0.1;", "if (0.11 > sigma) sigma = 0.11;", LLR,
           _V + "the floor of sigma, which only scales the stored LLRs.",
           equivalent="The floor enters the output through scale = 2 / sigma^2 alone, and the next statement clamps the scale to 30: a sigma "
                      "at or below 0.11 gives 2 / sigma^2 >= 165 under either floor, hence the scale 30.0 under both; a sigma above 0.11 "
                      "is not touched by either; a NaN fails both comparisons.  Any floor below sqrt(2 / 30) = 0.258 computes the same LLRs."),
    Mutant("llr_scale_lo", "es_llr.hip", "if (scale < 0.5) scale = 0.5;", "if (scale < 0.6) scale = 0.6;", LLR,
           _V + "the lower clamp of the LLR scale."),
    Mutant("llr_scale_hi", "es_llr.hip", "if (scale > 30.0) scale = 30.0;", "if (scale > 31.0) scale = 31.0;", LLR,
           _V + "the upper clamp of the LLR scale."),
    Mutant("llr_clip", "es_llr.hip", "if (v > 12.0f) v = 12.0f;", "if (v > 13.0f) v = 13.0f;", LLR,
           _V + "the upper clip of a stored LLR."),
    Mutant("llr_clip_lo", "es_llr.hip", "if (v < -12.0f) v = -12.0f;", "if (v < -13.0f) v = -13.0f;", LLR,
           _V + "the lower clip of a stored LLR."),
    Mutant("llr_screen_r", "es_llr.hip", "constexpr double SCREEN_R = 4e-6;", "constexpr double SCREEN_R = 4e-9;", LLR,
           "Narrows the band of shifts that get the float32 evaluation; the two largest exact scores always pass their own test, so the "
           "candidate list stays non-empty and inside its nshift slots, and fewer candidates mean fewer trips of the candidate loop."),
    # ---- es_llr.hip: the header decoder
    Mutant("hdr_npos", "es_llr.hip", "(npos >= 10) &&", "(npos > 10) &&", HDR, _V + "one term of the stored ok flag."),
    Mutant("hdr_margin", "es_llr.hip", "&& (margin > 0.5f));", "&& (margin >= 0.5f));", HDR, _V + "one term of the stored ok flag."),
    Mutant("hdr_guard_hi", "es_llr.hip", "int guard = ntaps / 8 < 32 ? ntaps / 8 : 32;", "int guard = ntaps / 8 < 31 ? ntaps / 8 : 31;", HDR,
           "The guard stays inside [8, 32], the range the unmutated code proves for it, so the scored part [guard, 128) of the header "
           "stays a pairwise leaf of 96 to 120 terms inside the window."),
    Mutant("hdr_guard_lo", "es_llr.hip", "if (guard < 8) guard = 8;", "if (guard < 9) guard = 9;", HDR,
           "The guard stays inside [8, 32], the range the unmutated code proves for it, so the scored part [guard, 128) of the header "
           "stays a pairwise leaf of 96 to 120 terms inside the window."),
    Mutant("hdr_bit_strict", "es_llr.hip", "(s_sums[b] < 0.0f ? 1u : 0u)", "(s_sums[b] <= 0.0f ? 1u : 0u)", HDR,
           _V + "one bit of the stored header value."),
    # ---- es_keyring.hip: plan_row
    Mutant("plan_round", "es_keyring.hip", "est = (int)((2LL * start + ES_FRAME_LEN) / (2 * ES_FRAME_LEN));", "est = (int)(start / ES_FRAME_LEN);", PLAN,
           "The estimate only centres the counter windows; every hop read stays guarded by 0 <= c < C and every store by the untouched "
           "pos < ES_MAX_TRIES."),
    Mutant("plan_pm3_origin", "es_keyring.hip", "const ctr_t c = est - 3 + lane;", "const ctr_t c = est - 2 + lane;", PLAN,
           "Shifts the seven counters of the narrow window; every hop read stays guarded by 0 <= c < C and every store by the untouched "
           "pos < ES_MAX_TRIES."),
    Mutant("plan_pm3_width", "es_keyring.hip", "else v = lane < 7 && c >= 0 && c < C", "else v = lane < 6 && c >= 0 && c < C", PLAN,
           "Drops one lane from the narrow window: fewer candidates, the same guards, the output position still under the untouched "
           "pos < ES_MAX_TRIES."),
    Mutant("plan_wide_lo", "es_keyring.hip", "est - 200 > 0 ? est - 200 : 0,", "est - 199 > 0 ? est - 199 : 0,",
           PLAN + ("tests/test_gpu_search_traces.py::test_identifier_follows_the_reference_under_every_key",),
           "Moves the wide window's first counter by one; its 400 to 402 counters take the same seven trips of 64, every hop read "
           "stays guarded by c < C and every store by the untouched pos < ES_MAX_TRIES."),
    Mutant("plan_wide_hi", "es_keyring.hip", "hi = est + 200;", "hi = est + 201;", PLAN,
           "Moves the wide window's last counter by one; its 400 to 402 counters take the same seven trips of 64, every hop read "
           "stays guarded by c < C and every store by the untouched pos < ES_MAX_TRIES."),
    Mutant("plan_lo16_mask", "es_keyring.hip", "(!hok || (c & 0xFFFF) == lo16);", "(!hok || (c & 0x7FFF) == lo16);", PLAN,
           _V + "the header gate of a candidate, stored under the untouched pos < ES_MAX_TRIES."),
    Mutant("plan_at_ctr_max", "es_keyring.hip", "v = lane < 7 && c >= 0 && c <= 0xFFFFFFFFLL", "v = lane < 7 && c >= 0 && c < 0xFFFFFFFFLL", PLAN_AT,
           "Refuses the last 32-bit counter in the narrow window: fewer candidates, the hop read keeps its c - hbase guards and the "
           "store the untouched pos < ES_MAX_TRIES."),
    # ---- es_keyring.hip: the other kernels
    Mutant("hop_ctr_max", "es_keyring.hip", "if (ctr <= 0xFFFFFFFFull)", "if (ctr < 0xFFFFFFFFull)", HOP,
           _V + "whether a table cell holds a band or 0xFF; the cell's index is untouched."),
    Mutant("acq_ctr_hi", "es_keyring.hip", "c >= ctr_lo && c < ctr_hi;", "c >= ctr_lo && c <= ctr_hi;", ACQ,
           _V + "one bit of a mask word whose index is untouched; the extra counter is hashed, never used as an address."),
    Mutant("acq_ctr_lo", "es_keyring.hip", "j < H && c >= ctr_lo", "j < H && c > ctr_lo", ACQ,
           _V + "one bit of a mask word whose index is untouched."),
    # ---- es_aead.hip
    Mutant("aead_ctr_24", "es_aead.hip", "&& be_ctr == ctr;", "&& (be_ctr & 0xFFFFFFu) == (ctr & 0xFFFFFFu);", AEAD,
           _V + "one term of the validator's verdict."),
    Mutant("aead_magic", "es_aead.hip", "pt[0] == 0x4c415345u", "pt[0] == 0x4c415344u", AEAD, _V + "one term of the validator's verdict."),
    Mutant("aead_fallback_arms", "es_aead.hip", "which = best_crc >= 0 ? best_crc : best_any;", "which = best_any >= 0 ? best_any : best_crc;", AEAD,
           "Both arms are -1 or a candidate row below n, and the untouched which >= 0 guard stands before the row is read."),
    Mutant("aead_crc_tie", "es_aead.hip", "best_crc < 0 || cm[r] < cm[best_crc]", "best_crc < 0 || cm[r] <= cm[best_crc]", AEAD,
           "Chooses between two candidate rows below n that the loop has already read."),
    Mutant("aead_hard_first", "es_aead.hip", "else if (hard_ok[f] && (!use_key", "else if (n == 0 && hard_ok[f] && (!use_key", AEAD,
           "Sends a frame whose hard decision passes to the list loop the unmutated code runs whenever it fails: the same rows below "
           "n <= L of arrays allocated for L rows per frame."),
    # ---- es_memo.hip
    Mutant("memo_claim_max", "es_memo.hip", "atomicMin(&claim[", "atomicMax(&claim[", MEMO,
           "The claim word rests at all ones, so a maximum never changes it and no record writes; the atomic's address is unchanged."),
    Mutant("memo_probe_one_word", "es_memo.hip", "(uint8_t)(e.x == a && e.y == b);", "(uint8_t)(e.x == a);", MEMO,
           _V + "the stored hit flag, from the entry already loaded."),
    # ---- es_sched.hip
    Mutant("sched_band_mask", "es_sched.hip", "& 3u);", "& 1u);", SCHED, _V + "the stored band byte."),
    Mutant("sched_hmac_len", "es_sched.hip", "w[15] = (64 + 4) * 8;", "w[15] = (64 + 3) * 8;", SCHED,
           _V + "one word of the hashed message block, a register array with a constant index."),
    # ---- es_tx.hip
    Mutant("tx_peak_strict", "es_tx.hip", "const bool scale = peak > 3.0;", "const bool scale = peak >= 3.0;", TX,
           _V + "whether the stored chips are multiplied by 1 / peak."),
    Mutant("tx_peak_eps", "es_tx.hip", "const double peak = m + 1e-12;", "const double peak = m + 1e-11;", TX,
           _V + "the addend of the peak the chips are divided by."),
    # ---- es_mix.hip: the gain rule (the kernels are es_mix_body.inc, compiled into es_mix.hip)
    Mutant("mix_floor_max", "es_mix.hip", "if (floor_lin > scale) scale = floor_lin;", "if (floor_lin < scale) scale = floor_lin;", MIX,
           _V + "the gain of a block, a float64 the chips are multiplied by."),
    Mutant("mix_head_min", "es_mix.hip", "if (q < scale) scale = q;", "if (q > scale) scale = q;", MIX,
           _V + "the gain of a block, a float64 the chips are multiplied by."),
    Mutant("mix_headroom", "es_mix.hip", "double head = 0.98 - (double)mx;", "double head = 0.97 - (double)mx;", MIX,
           _V + "the headroom that limits the gain of a block."),
    Mutant("mix_peak_pos", "es_mix.hip", "if (peak > 0.0) {", "if (peak >= 0.0) {", MIX, _V + "which arm sets the gain of a block.",
           equivalent="peak = (double)mc + 1e-12 where mc is a maximum of float32 absolute values: it is either at least 1e-12, and "
                      "then both comparisons hold, or a NaN, and then both fail; it is never zero, the one value that separates them."),
    # ---- es_resample.hip
    Mutant("resample_i16_scale", "es_resample.hip", "return (float)*p / 32768.0f;", "return (float)*p / 32767.0f;", RES,
           _V + "the value of an int16 sample after its load."),
    Mutant("resample_fused_add", "es_resample.hip", "const T p = (T)rs_load(xw + m) * hp[m]; acc = acc + p;",
           "const T p = (T)rs_load(xw + m); acc = sizeof(T) == 4 ? (T)__builtin_fmaf((float)p, (float)hp[m], (float)acc) : (T)__builtin_fma((double)p, (double)hp[m], (double)acc);", RES,
           "Rounds product and sum once where the original rounds each: the same one load per tap from the same window and table "
           "positions, one instruction for two, the same trip count.  (Every phase and offset rounding of this file feeds a subscript, so none of them is a mutant.)"),
    # ---- es_sync32.hip.  Not listed: the saturation shortcut's margin, `MARG = 2.5 * DELTA` made 1.5 * DELTA.  It survived the first run
    # and cannot change a threshold or a peak: the shortcut answers 0.95 when X / 128 - (1 + 6.6717) MARG >= 0.95 + 1e-6 for the integers
    # X = bl - 128 + 6.6717 j of the histogram, while the bins prove thr >= X / 128 - (1 + 2 * 6.6717) DELTA; no (bl, j) lies between the two
    # (tests/test_mutants_listed.py::test_the_saturation_margin_cannot_move_a_threshold enumerates them, DESIGN 2.2 has the argument).  The
    # three equivalent slots being taken, it was replaced by the fallback's slack below, which can matter.
    Mutant("s32_fallback_slack", "es_sync32.hip", "lo = (double)t5 - 2.0 * DELTA;", "lo = (double)t5 - 1.0 * DELTA;", S32,
           "Raises the bound below which the fallback ignores screen values: fewer lags enter a list whose store keeps its untouched "
           "pos < PW_CAP guard, and the ranks are stored under the untouched before < kmax."),
    Mutant("s32_fused_fallback_tie", "es_sync32.hip", "(vj == v && ij > ii);", "(vj == v && ij < ii);", S32,
           "Reverses the order of equal values in the fallback's rank; the ranks stay a permutation and the store keeps its untouched "
           "before < kmax guard."),
    Mutant("s32_rival_ge", "es_sync32.hip", "beats |= jv > cv; });", "beats |= jv >= cv; });", S32,
           _V + "whether an exactly evaluated rival suppresses a candidate; peaks are stored under the untouched total < ES_MAX_PEAKS."),
    Mutant("s32_exact_row_tie", "es_sync32.hip", "(v == bv && i > bi)", "(v == bv && i < bi)", S32,
           _V + "which of two equal lags of the row the exact fallback keeps; the lag is stored and compared, never a subscript."),
    # ---- es_sync.hip
    Mutant("xcorr_energy_eps", "es_sync.hip", "num[r] / (__builtin_sqrt(en[r]) + 1e-12);", "num[r] / (__builtin_sqrt(en[r]) + 1e-11);", XCORR,
           _V + "the addend of a correlation's denominator."),
    Mutant("bpf_i16_scale", "es_sync.hip", "if (t < T) v0 = (float)f[t] * (1.0f / 32768.0f);", "if (t < T) v0 = (float)f[t] * (1.0f / 32767.0f);", BPF,
           _V + "the value of an int16 sample after its guarded load."),
    # ---- the list decoders: arithmetic on LLRs and metrics only
    Mutant("scl_hard_strict", "es_scl.hip", "(lam >= 0.0) ? 1u : 0u;", "(lam > 0.0) ? 1u : 0u;", SCL,
           "The preferred bit of a leaf only selects which of the two penalties lp and lp + al a path metric receives.",
           equivalent="The two forms differ for lam == +-0.0 alone (a NaN fails both).  The preferred bit is used for one thing, to choose "
                      "between the penalties lp and lp + al, and there al = |lam| = 0.0 and lp = log 2 > 0, so lp + al == lp bit for bit: "
                      "every metric, and with it every decision and output, is the same.  The same holds for the same line of "
                      "es_scl_multi.hip and es_scl_wide.hip, and for `x >= 0.0` in the leaf blocks, which are therefore not listed."),
    Mutant("scl_multi_frozen_penalty_sign", "es_scl_multi.hip", "if (pref != 0u) pen = lp + al;", "if (pref != 0u) pen = lp - al;", SCL,
           "Changes the penalty a frozen leaf adds to a path metric: a float64 that is only added, compared and stored."),
    Mutant("scl_leaf_penalty_sign", "es_softplus_dev.h", "(bit != pref) ? lp + al : lp;", "(bit != pref) ? lp - al : lp;", SCL,
           "Changes the penalty a leaf adds to a path metric in the lane-per-path decoder: a float64 that is only added, compared and stored."),
    Mutant("scl_g_sign", "es_math.h", "((uint64_t)(u & 1u) << 63)", "((uint64_t)(~u & 1u) << 63)", SCL,
           "Flips the sign g gives its first operand: an LLR value, in every list decoder, with no index derived from it."),
]

# ---------------------------------------------------------------------------------------------------------------------------------
# The list decoders: the fine-grained decisions of es_scl.hip, es_scl_multi.hip, es_scl_wide.hip (es_scl_wide_large.hip
# compiles the same kernel) and of the arithmetic they share, es_math.h and es_softplus_dev.h.  The same tuple and the same rules, with one
# more: the decoders spin on slots and barriers, so no entry feeds a subscript, a slab, LDS or slot address (p8_get / p8_set, ptr_get, fp0,
# myr, holder, parent, src, any W.sel / TBW / TBA / CB index), cnt, keep, nc, a trip count, the slot claim or release, a barrier or fence,
# launch geometry, the ki & 127 table index, a DPP or swizzle control or an asm block; a tie rule is reversed (`<` -> `>`: still a strict
# total order, the ranks stay a permutation), never made non-strict.  At most four entries are declared equivalent.
# tests/test_mutants_listed.py holds the table to these rules.  `tools/mutant_audit.py --table scl` builds and runs it.
_SL = "tests/test_softplus_sl_gpu.py"
_SEDGE = "tests/test_gpu_scl_decision_edges.py"
SCL_K = SCL + (_PARITY + "::test_scl_other_codes_vs_oracle",)                      # the run-time-K arms of the lane-per-path decoder
SCL_HDR = SCL + (_PARITY + "::test_device_softplus_bits", _SL + "::test_device_f_edge_operands_bits")
SCL_RANGE = SCL_HDR + (_PARITY + "::test_scl_softplus_fallback_ranges",)
# with the tests written for the survivors of the first run (tests/test_gpu_scl_decision_edges.py)
SCL_ZERO = SCL + (_SEDGE + "::test_zero_llrs_decide_the_hard_crc",)
SCL_K0 = SCL_HDR + (_SEDGE + "::test_log1p_k_boundary_inside_the_tree",)
SCL_CORNER_FIRST = SCL_HDR + (_SEDGE + "::test_log1p_corner_first_word_inside_the_tree",)
SCL_CORNER_LAST = SCL_HDR + (_SEDGE + "::test_log1p_corner_last_word_inside_the_tree",)

_RANK = ("Reverses the order of equal metrics in a rank: `<` and `>` on distinct indices are both strict total orders, so the ranks stay a "
         "permutation of the same range and every guarded store under `rank < keep` or into the rows below cnt writes the same set of slots.")
_HARD = "A comparison inside a value computation: one bit of the hard decision's word, which is only folded, gathered into bytes and stored."
_PEN = "Chooses which of two softplus values already computed for this path becomes a penalty: a float64 that is only added, compared and stored."
_CRC = "A comparison inside a value computation: the stored CRC verdict of one candidate row, from bytes already read."
_HOK = ("Flips the wave-uniform CRC verdict of the hard decision: it is stored, and with skip_if_hard_ok it chooses between the two paths "
        "(zeroed rows or the list) that the unmutated kernel takes for other frames of the same launch.")
_RNG = ("Moves the bound of the range flag of the straight-line softplus: operands in [512, 1024) then keep the straight-line value, which is "
        "arithmetic and one table read under the untouched ki & 127 mask, in place of the generic one.")
_DEAD = ("lp_odd is read at an odd leaf alone, and holds what the decision of its even sibling stored.  The frozen arm stores it only where an "
         "even leaf is decided leaf by leaf and is frozen: every other frozen even leaf opens an all-frozen aligned block of two or more "
         "leaves (the rate-0 arm, which takes the odd leaf's term from L2last), so that is leaf 0, or an even leaf whose odd sibling "
         "carries information.  No Polar(1024, K) frozen set has either, K = 9 .. 1024: leaf 0 always carries information and a frozen "
         "even leaf always has a frozen odd sibling (tests/test_mutants_listed.py::test_no_code_has_a_frozen_even_leaf_before_an_information_leaf "
         "enumerates them), and these two kernels run the K = 448 code only.  The value the line stores is never read.")
_SEL = "A threshold on the high word of a float64 that selects among values all of which the straight-line softplus has already computed."

SCL_MUTANTS = [
    # ---- es_scl.hip: one wave per frame
    Mutant("s1_bit_tie", "es_scl.hip", "(mk == mc && k < cc_)", "(mk == mc && k > cc_)", SCL, _RANK),
    Mutant("s1_final_tie", "es_scl.hip", "(mk == metric && k < path)", "(mk == metric && k > path)", SCL, _RANK),
    Mutant("s1_hard_zero", "es_scl.hip", "__ballot(v > 0.0)", "__ballot(v >= 0.0)", SCL_ZERO, _HARD),
    Mutant("s1_odd_penalty_info", "es_scl.hip", "(q & 1) ? sp_diff : sp_sum", "(q & 1) ? sp_sum : sp_diff", SCL, _PEN),
    Mutant("s1_odd_penalty_frozen", "es_scl.hip", "lp_odd = sp_sum;", "lp_odd = sp_diff;", SCL, _PEN, equivalent=_DEAD),
    Mutant("s1_cand_crc", "es_scl.hip", "crc8_bytes(W.outb[path], ES_INFO_BYTES) == W.outb[path][ES_INFO_BYTES];",
           "(crc8_bytes(W.outb[path], ES_INFO_BYTES) & 0x7fu) == (W.outb[path][ES_INFO_BYTES] & 0x7fu);", SCL, _CRC),
    Mutant("s1_hard_crc", "es_scl.hip", "== W.outb[0][ES_INFO_BYTES]);", "!= W.outb[0][ES_INFO_BYTES]);", SCL, _HOK),
    Mutant("s1_rate0_penalty", "es_scl.hip", "double pen = (P >= 2 && (q & 1)) ? L2last : lp;", "double pen = (P >= 2 && (q & 1)) ? lp : L2last;", SCL,
           _PEN),
    # ---- es_scl_multi.hip: several frames per wave
    Mutant("sm_bit_tie", "es_scl_multi.hip", "(mk == mc && k < cc_)", "(mk == mc && k > cc_)", SCL, _RANK),
    Mutant("sm_final_tie", "es_scl_multi.hip", "(mk == metric && k < pl)", "(mk == metric && k > pl)", SCL, _RANK),
    Mutant("sm_hard_zero", "es_scl_multi.hip", "__ballot(v > 0.0)", "__ballot(v >= 0.0)", SCL_ZERO, _HARD),
    Mutant("sm_odd_penalty_info", "es_scl_multi.hip", "(q & 1) ? sp_diff : sp_sum", "(q & 1) ? sp_sum : sp_diff", SCL, _PEN),
    Mutant("sm_odd_penalty_frozen", "es_scl_multi.hip", "lp_odd = sp_sum;", "lp_odd = sp_diff;", SCL, _PEN, equivalent=_DEAD),
    Mutant("sm_cand_crc", "es_scl_multi.hip", "crc8_bytes(W.outb[path], ES_INFO_BYTES) == W.outb[path][ES_INFO_BYTES];",
           "(crc8_bytes(W.outb[path], ES_INFO_BYTES) & 0x7fu) == (W.outb[path][ES_INFO_BYTES] & 0x7fu);", SCL, _CRC),
    Mutant("sm_hard_crc", "es_scl_multi.hip", "== W.outb[0][ES_INFO_BYTES]);", "!= W.outb[0][ES_INFO_BYTES]);", SCL, _HOK),
    Mutant("sm_rate0_penalty", "es_scl_multi.hip", "double pen = (q & 1) ? L2last : lp;", "double pen = (q & 1) ? lp : L2last;", SCL, _PEN),
    # ---- es_scl_wide.hip: one lane per path (es_scl_wide_large.hip compiles it for two more capacities)
    Mutant("sw_final_tie", "es_scl_wide.hip", "(mk == metric && k < pl)", "(mk == metric && k > pl)", SCL, _RANK),
    Mutant("sw_hard_zero", "es_scl_wide.hip", "__ballot(v > 0.0)", "__ballot(v >= 0.0)", SCL_ZERO, _HARD),
    Mutant("sw_odd_penalty_wave", "es_scl_wide.hip", "bit ? sd : ss", "bit ? ss : sd", SCL, _PEN),
    Mutant("sw_odd_penalty_block", "es_scl_wide.hip", "xsp[xb][bit ? 0 : 1]", "xsp[xb][bit ? 1 : 0]", SCL,
           "Chooses which of the two softplus rows this step published, both written for every lane under the same barrier, becomes a "
           "penalty: the subscript stays one of the constants 0 and 1 that the unmutated line uses.",),
    Mutant("sw_odd_penalty_frozen", "es_scl_wide.hip", "lp_odd = sp_sum;", "lp_odd = sp_diff;", SCL, _PEN),
    Mutant("sw_cand_crc", "es_scl_wide.hip", "(wd[MWIN_W - 1] & 0xffu)", "(wd[MWIN_W - 1] & 0x7fu)", SCL, _CRC),
    Mutant("sw_hard_crc", "es_scl_wide.hip", "== hbytes[ES_INFO_BYTES]);", "!= hbytes[ES_INFO_BYTES]);", SCL, _HOK),
    Mutant("sw_cand_crc_k", "es_scl_wide.hip", "(uint8_t)(reg == ((((lo << 8) | hi) >> (8 - rem)) & 0xffu));",
           "(uint8_t)(reg == ((((lo << 8) | hi) >> (8 - rem)) & 0x7fu));", SCL_K, _CRC),
    Mutant("sw_hard_crc_k", "es_scl_wide.hip", "ok = (reg == (", "ok = (reg != (", SCL_K, _HOK),
    Mutant("sw_window_start", "es_scl_wide.hip", "const bool wstart = (info_idx & 31) == 0;", "const bool wstart = (info_idx & 31) == 1;", SCL,
           "Moves the step at which a trace-back window's history word and ancestor are reset: both are stored values, the ancestor is "
           "a lane index below LF and is masked by LF - 1 where the final trace-back reads it."),
    Mutant("sw_odd_leaf_g_bit", "es_scl_wide.hip", "(b0 >> 1) & 1u", "(b0 >> 2) & 1u", SCL,
           "Takes another bit of the path's partial-sum word as the sign g gives its first operand: an LLR value with no index derived from it."),
    Mutant("sw_fold", "es_scl_wide.hip", "cw = (left ^ cw) | (cw << S);", "cw = (left & cw) | (cw << S);", SCL,
           "Changes the bits of a partial-sum word, which are only stored, folded again and used as the signs of g; the words' positions are untouched."),
    # ---- es_softplus_dev.h: the straight-line softplus and f of the lane-per-path decoder
    Mutant("sd_leaf_range", "es_softplus_dev.h", "*bad |= !(al < 512.0);", "*bad |= !(al < 1024.0);", SCL_RANGE, _RNG),
    Mutant("sd_f_range", "es_softplus_dev.h", "(__builtin_fabs(d1) < 512.0) & (__builtin_fabs(sum) < 512.0)",
           "(__builtin_fabs(d1) < 1024.0) & (__builtin_fabs(sum) < 1024.0)", SCL_RANGE, _RNG),
    Mutant("sd_slg_range", "es_softplus_dev.h", "if (!(__builtin_fabs(d1) < 512.0)) L1 =", "if (!(__builtin_fabs(d1) < 1024.0)) L1 =", SCL_RANGE, _RNG),
    Mutant("sd_tiny29", "es_softplus_dev.h", "hy < 0x3e200000", "hy < 0x3e100000", SCL_HDR, _SEL),
    Mutant("sd_k0", "es_softplus_dev.h", "hy < 0x3FDA827A", "hy < 0x3FDA827B", SCL_K0, _SEL),
    Mutant("sd_corner", "es_softplus_dev.h", "hu0 > 0x3FFFFFFCu", "hu0 > 0x3FFFFFFDu", SCL_CORNER_FIRST, _SEL),
    # ---- es_math.h: the softplus of the other two decoders and of every cold path
    Mutant("em_tiny29", "es_math.h", "hy < 0x3e200000", "hy < 0x3e100000", SCL_HDR, _SEL),
    Mutant("em_k0", "es_math.h", "hy < 0x3FDA827A", "hy < 0x3FDA827B", SCL_K0, _SEL),
    Mutant("em_corner", "es_math.h", "(hu0 - 0x3FFFFFFDu) < 3u", "(hu0 - 0x3FFFFFFDu) < 2u", SCL_CORNER_LAST, _SEL),
    Mutant("em_fast_range", "es_math.h", "*ok = (__builtin_fabs(t) < 512.0);", "*ok = (__builtin_fabs(t) < 1024.0);", SCL_RANGE, _RNG),
    Mutant("em_lp1", "es_math.h", "#define ES_LP1 6.666666666666735130e-01", "#define ES_LP1 6.666666666666736130e-01", SCL_HDR,
           "Moves log1p's first polynomial coefficient to the next double (0x1.5555555555593p-1 -> ...94p-1): a float64 that is only multiplied and added."),
]

BY_ID = {m.id: m for m in MUTANTS + SCL_MUTANTS}
