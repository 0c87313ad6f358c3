/* echoseal_hip.h -- C ABI of libechoseal_hip.so, the MI355X (gfx950) implementation of the
 * EchoSeal receive hot path.
 *
 * The reference (PetarSt98/EchoSeal) is pure Python and has no FFI layer; the boundary a
 * maintainer would bind is therefore the set of NumPy/SciPy calls its detector makes on the hot
 * path.  Each entry point below names the reference code it replaces.  The Python host package
 * (echoseal_amd/, re-exported as `rtwm`) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - return value: 0 on success, negative ES_E* code on failure; es_last_error() gives text.
 *   - "dev" pointers are device (HBM) addresses owned by the caller (e.g. torch tensors);
 *     "host" pointers are ordinary host memory, copied during the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls only enqueue
 *     work; they never synchronise the device, so they may be captured into a hipGraph.
 *   - one es_ctx per host thread / Python object; a context is not re-entrant.
 *   - echoseal_amd/_native.py reads its ctypes signatures and every ES_* constant from this file (bind_header): parameters are pointers,
 *     int, int64_t, uint32_t or double; a `const uint8_t* <name>_host` is passed a bytes object; an ES_* #define is an integer literal
 *     or `a << b`.  Anything else is refused at import (tests/test_abi_binding.py).
 */
#ifndef ECHOSEAL_HIP_H
#define ECHOSEAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this ABI.  2 (round 4): the tap table of es_set_tables has a row stride of ES_MAX_TAPS = 576 floats (1: 160), the
 * `nflag` parameters are gone, es_info_bytes / es_front_batch exist.  Added within 2 (no existing signature or behaviour changed):
 * es_llr_at_batch, es_header_at_batch, es_front_peak_batch -- demodulation and header decode at detected peaks.  A binder must
 * compare es_abi_version() with the ES_ABI_VERSION it was written against and refuse a mismatch (echoseal_amd/_native.py:load
 * does; the stub in INTEGRATION.md does). */
#define ES_ABI_VERSION   2

#define ES_OK            0
#define ES_EINVAL      (-1)   /* bad argument (shape, list size, null pointer) */
#define ES_ENOTREADY   (-2)   /* tables / schedule not set */
#define ES_EHIP        (-3)   /* a HIP runtime call failed */
#define ES_ENOMEM      (-4)

#define ES_FRAME_LEN   1215   /* 63 preamble + 128 header + 1024 payload chips (rtwm/detector.py:13-19) */
#define ES_PRE_L         63
#define ES_HDR_L        128
#define ES_POLAR_N     1024
#define ES_POLAR_K      448
#define ES_INFO_BYTES    55
#define ES_NBANDS         4
#define ES_MAX_TAPS     576   /* row stride of the tap table: the reference's taps are 93..131 long at fs_target = 48 000, 550 at 44 100 (rtwm/detector.py:260-294) */
#define ES_MAX_TAPS_FAST 160  /* up to here the demodulator runs its small-footprint instantiation */
#define ES_MAX_PEAKS     32   /* detector consumes at most 25 peaks per scan (rtwm/detector.py:108) */
#define ES_MAX_LIST    1024   /* any list size 1..1024; the mapping of paths to lanes is chosen per launch (es_set_option) */
#define ES_PN_BYTES     152   /* ceil(1215 / 8): packed PN row of one frame counter */
#define ES_KEYRING_BYTES 304  /* one key-ring row (es_keyring_derive_batch) */
#define ES_MAX_TRIES    400   /* candidates per (key, band) scan (rtwm/detector.py:107) */
#define ES_PEAK_LIMIT    25   /* peaks looked at per scan (rtwm/detector.py:108) */

#define ES_DTYPE_F32      0
#define ES_DTYPE_I16      1
#define ES_DTYPE_F64      2

typedef struct es_ctx es_ctx;

/* Context: binds a device, owns table / scratch memory.  list_size_max 1..1024: the largest list es_scl_batch will be asked for (sizes
 * the list decoder's scratch slabs, 0.4 GB; above 32 also the 1.6 GB lane-per-path slab, 2.2 GB above 512).  list_size_max = 0: a FRONT-END context --
 * every entry point except es_scl_batch, no list-decoder scratch at all (what a pipeline's band-pass / sync / demodulator streams use). */
es_ctx*     es_create(int device, int list_size_max);
void        es_destroy(es_ctx* ctx);
const char* es_last_error(const es_ctx* ctx);          /* ctx may be NULL (creation errors) */
int         es_abi_version(void);                      /* == ES_ABI_VERSION of the header the library was built from */
int         es_info_bytes(const es_ctx* ctx);          /* bytes of one packed information row of es_scl_batch: 55, or ceil((K - 8) / 8) after es_set_tables with another K */

/* Static per-band tables (host pointers).
 *   ba      [4][18]  Butterworth b[9] then a[9], float64      <- rtwm/utils.py:52-55 butter_bandpass
 *   tpl     [4][63]  unit-norm cascaded preamble template      <- rtwm/detector.py:67-69
 *   taps    [4][ES_MAX_TAPS] float32 matched-filter taps, zero padded <- rtwm/detector.py:260-294 (any fs_target whose filters fit:
 *           93..131 taps at 48 000 Hz, 550 at 44 100; above ES_MAX_TAPS_FAST the demodulator runs its large-footprint instantiation)
 *   ntaps   [4]
 *   frozen  [1024]   1 = frozen bit                            <- rtwm/fastpolar.py:225-226
 * The mask leaves K information positions (information bits + CRC-8): 448 for the reference's own code (rtwm/polar_fast.py:8-9) and for
 * every entry point; es_scl_batch alone also serves any 9 <= K <= 1024 (what PolarCode(1024, K) of rtwm/fastpolar.py:209-234
 * builds), with rows of es_info_bytes(ctx) = ceil((K - 8) / 8) bytes in place of ES_INFO_BYTES: np.packbits of the K - 8
 * information bits, i.e. zero padding in the last byte when K is not a multiple of 8.                                           */
int es_set_tables(es_ctx* ctx, const double* ba, const double* tpl, const float* taps,
                  const int32_t* ntaps, const uint8_t* frozen);

/* Band-pass: y = lfilter(b, a, x.astype(float32)), zero initial state, float64 out.
 *   replaces rtwm/detector.py:59-60 (and :240-241)
 *   frames_dev [B][T] ES_DTYPE_F32 or ES_DTYPE_I16 (int16 is dequantised as x/32768, what soundfile.read hands the
 *              reference for PCM16 files, rx_app.py:26)
 *   band_dev   [B] uint8 index into the band tables
 *   y_dev      [B][T] float64                                                               */
int es_bpf_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                 const uint8_t* band_dev, double* y_dev, void* stream);

/* Normalised cross-correlation with the 63-chip template:
 *   corr[i] = sum_k y[i+k] tpl[k] / (sqrt(sum_k y[i+k]^2) + 1e-12),  i in [0, T-62)
 *   replaces rtwm/detector.py:76-79 (np.convolve + scipy.signal.correlate)
 *   corr_dev [B][T-62] float64                                                               */
int es_xcorr_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const uint8_t* band_dev,
                   double* corr_dev, void* stream);

/* Median/MAD threshold + non-maximum suppression (+ top-5 fallback):
 *   replaces rtwm/detector.py:83-99
 *   thr_dev    [B] float64
 *   peaks_dev  [B][ES_MAX_PEAKS] int32 (ascending; fallback: descending correlation); whole rows are written, -1 = unused
 *   npeaks_dev [B] int32: number of valid entries; bit 30 set when the fallback branch ran      */
int es_pick_batch(es_ctx* ctx, const double* corr_dev, int64_t B, int n_lags, double* thr_dev,
                  int32_t* peaks_dev, int32_t* npeaks_dev, void* stream);

/* Float32 correlation screen + float64 exact fix-ups (same thr / peaks / npeaks as the float64
 * calls above, bit for bit; see echoseal_amd/csrc/es_sync32.hip):
 *   es_bpf2_batch        like es_bpf_batch, and also writes y32_dev [B][T] = (float)y
 *                        (what _llr casts to anyway, rtwm/detector.py:323,329)
 *   es_xcorr32_batch     corr32_dev [B][T-62] float32 from y32_dev: 4 860 B in + 4 612 B out per
 *                        1215-sample record -- the HBM-graded kernel
 *   es_pick_exact_batch  thr/peaks/npeaks from corr32 with float64 re-evaluation of every value
 *                        near a decision, by the picker of es_sync_fused_batch (same results, flags
 *                        included); records the screen cannot settle are settled from float64
 *                        re-evaluations alone, and flags_dev [B] holds the reason code 1..5 (0 =
 *                        settled from the screen), for information.  No workspace.  T - 62 <= 4096.
 *                        The caller's screen must satisfy |corr32 - corr64| <= 3e-5 at every lag (corr64 =
 *                        what es_xcorr_batch computes from y_dev); ANY such screen yields the float64
 *                        result, and a non-finite or absurd value (|v| >= 1e30) only costs the record the
 *                        float64 redo (code 1).  tests/test_gpu_sync_screen.py holds this with screens
 *                        built to be the worst case for each decision. */
int es_bpf2_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                  const uint8_t* band_dev, double* y_dev, float* y32_dev, void* stream);
int es_xcorr32_batch(es_ctx* ctx, const float* y32_dev, int64_t B, int T, const uint8_t* band_dev,
                     float* corr32_dev, void* stream);
int es_pick_exact_batch(es_ctx* ctx, const float* corr32_dev, const double* y_dev, int64_t B, int T,
                        const uint8_t* band_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev,
                        uint8_t* flags_dev, void* stream);

/* The same result in ONE kernel (SURVEY.md section 8d "fused with threshold + NMS and writing only peaks"): the float32
 * correlation row of a record stays in LDS, threshold (median / MAD or the proof that it saturates at 0.95) and peaks are
 * settled from it with float64 re-evaluation of every value near a decision, and only thr / peaks / npeaks / flags reach
 * HBM: 4 T bytes of samples in (+ the few float64 samples the re-evaluations read), <= 150 bytes out per record.
 * thr / peaks / npeaks bit-identical to es_xcorr_batch + es_pick_batch.  Records the screen cannot settle (digital silence,
 * constants, exact repeats, a float32 overflow) are settled by the same wave from float64 re-evaluations alone -- slowly, with
 * no workspace and no second launch; flags_dev [B] then holds the reason code 1..5 (0 = settled from the screen), for
 * information.  T - 62 <= 4096.
 *   replaces rtwm/detector.py:76-99                                                                                  */
int es_sync_fused_batch(es_ctx* ctx, const float* y32_dev, const double* y_dev, int64_t B, int T,
                        const uint8_t* band_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev,
                        uint8_t* flags_dev, void* stream);

/* The receive front end of one batch in one call -- es_bpf2_batch, es_sync_fused_batch and es_llr_batch (variant 0, start_dev as
 * there: NULL = 0) enqueued on `stream` in that order: what a streaming pipeline submits per batch (one trip through the
 * binding instead of three; same kernels, same results).  T - 62 <= 4096.
 *   replaces rtwm/detector.py:59-99 + 296-416 for a batch of records                                                     */
int es_front_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const uint8_t* band_dev,
                   const uint8_t* pn_dev, const int32_t* start_dev, double* y_dev, float* y32_dev, double* thr_dev,
                   int32_t* peaks_dev, int32_t* npeaks_dev, uint8_t* flags_dev, float* llr_dev, void* stream);

/* es_front_batch with the demodulator at each record's FIRST DETECTED PEAK: es_bpf2_batch, es_sync_fused_batch and
 * es_llr_at_batch(row_dev = NULL, start_dev = peaks_dev, start_stride = ES_MAX_PEAKS, variant 0) enqueued on `stream` in that order.
 * A record without a peak (peaks_dev[i][0] = -1) is demodulated from 0, as clamp(min=0) would.  No host step and no other kernel
 * between sync and the demodulator.  T - 62 <= 4096.
 *   replaces rtwm/detector.py:59-99 + 110-161 (frame = y[start : start+1215] at the peak, then _llr) for a batch of records */
int es_front_peak_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const uint8_t* band_dev,
                        const uint8_t* pn_dev, double* y_dev, float* y32_dev, double* thr_dev, int32_t* peaks_dev,
                        int32_t* npeaks_dev, uint8_t* flags_dev, float* llr_dev, void* stream);

/* Size the context's float64 correlation workspace (used by es_sync_batch without corr_dev) for batches of up to B_max
 * records of T_max samples.  Allocation synchronises the device: call this once, outside any stream capture; afterwards
 * es_sync_batch only enqueues.  Without it es_sync_batch grows the workspace itself the first time a larger batch arrives
 * (same effect as calling es_reserve there).
 * es_reserve does not cover the list decoder: its slabs are allocated by es_create, and the 1.6 GB lane-per-path slab of contexts with
 * list_size_max <= 32 by es_set_option "scl_lane_slab" / "scl_lanes" = 1 -- set those before the first enqueue-only call as well.
 * Streams: the float64 workspace is shared by every call on the context (one stream at a time for the entry points that use it).  The list
 * decoder's slabs are guarded: es_scl_batch launches on one stream are ordered by the stream, launches of the same slot geometry on several
 * streams share the slab through its slot bitmap, and a launch of another geometry is ordered ON THE DEVICE behind the last launch of every
 * other stream that used the slab (hipStreamWaitEvent on an event the context records after each launch: the host does not block, the call
 * stays enqueue-only).  Stream capture: the guard is not part of a captured graph -- do not replay graphs of different slot geometry
 * (different list capacities / kernel mappings) of ONE context concurrently; launches with skip_if_hard_ok recorded into a capture keep a
 * frame counter of their own for the life of the context (at most 256 such launches per context, ES_ENOMEM beyond).                                 */
int es_reserve(es_ctx* ctx, int64_t B_max, int T_max);

/* Convenience: the three float64 calls above back to back (workspace owned by the context). */
int es_sync_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T,
                  const uint8_t* band_dev, double* y_dev, double* corr_dev /* nullable */,
                  double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev, void* stream);

/* es_sync_batch for records of unequal length in one batch (the float64 path: any row length).
 *   frames_dev [B][T] ES_DTYPE_F32 or ES_DTYPE_I16: T is the row stride, T >= 63
 *   len_dev    [B] int32: record i is frames[i][0 : len[i]], len[i] clamped to [0, T] on the device
 *   y_dev      [B][T], corr_dev (nullable) [B][T-62]: the row strides are those of T
 * For len[i] >= 63 record i gets what es_sync_batch gives for it alone with T = len[i], bit for bit: thr, the whole peaks row, npeaks
 * with its bit-30 fallback flag, y[i][0 : len[i]] and (when corr_dev is given) corr[i][0 : len[i]-62].  For len[i] < 63: npeaks 0, thr
 * 0.0 and a peaks row of -1, the reference's return for a record shorter than the template (rtwm/detector.py:71-73).
 * Samples of a row past len[i] may hold anything, NaN and +-inf included: no output listed above depends on them (the band-pass is
 * causal with zero initial state and runs the stored row to T; correlation and pick stop at the record's end).
 * y[i][len[i] : T] and corr[i][len[i]-62 : T-62] are UNSPECIFIED.  The peak-addressed calls (es_llr_at_batch, es_header_at_batch) on
 * such a y with this T are therefore defined only for frames that lie inside their record, start + 1215 <= len[row]; a frame that
 * runs past its record's end would be read from the unspecified tail.
 * Argument checks as es_sync_batch (T >= 63, B == 0 enqueues nothing, null pointers are refused, len_dev among them); the same
 * workspace rule: after es_reserve(B, T) the call only enqueues, so it can be captured in a graph.                              */
int es_sync_ragged_batch(es_ctx* ctx, const void* frames_dev, int dtype, int64_t B, int T, const int32_t* len_dev,
                         const uint8_t* band_dev, double* y_dev, double* corr_dev /* nullable */,
                         double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev, void* stream);

/* Soft demodulation of the payload of one frame per record:
 *   replaces WatermarkDetector._llr (rtwm/detector.py:296-416)
 *   y_dev      [B][T] float64 band-passed records
 *   start_dev  [B] int32 frame start inside the record (frame = y[start : start+1215], may be short)
 *   pn_dev     [B][ES_PN_BYTES] packed PN bits of the frame counter (MSB first)
 *                                                       <- SecureChannel.pn_bits, rtwm/crypto.py:46-48
 *   variant    0: payload PN = bits [191, 1215); 1: bits [0, 1024)   (rtwm/detector.py:306-312)
 *   llr_dev    [B][1024] float32
 *   best_s_dev [B] int32 (nullable), score_dev [B][2] float32 best / runner-up (nullable)      */
int es_llr_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const int32_t* start_dev,
                 const uint8_t* band_dev, const uint8_t* pn_dev, int variant, float* llr_dev,
                 int32_t* best_s_dev, float* score_dev, void* stream);

/* Header decode (16-bit counter, each bit repeated 8x, spread with the static header PN):
 *   replaces WatermarkDetector._decode_header (rtwm/detector.py:452-515)
 *   y_dev      [B][T] float64 band-passed records, start_dev [B] frame start (nullable = 0)
 *   hdr_pn_dev [B][16] packed header PN bits (pn_bits(0, 128), MSB first)
 *   ok_dev [B] uint8, val_dev [B] int32 (ctr & 0xFFFF estimate), score_dev [B] float32,
 *   best_s_dev [B] int32 (nullable)                                                          */
int es_header_batch(es_ctx* ctx, const double* y_dev, int64_t B, int T, const int32_t* start_dev,
                    const uint8_t* band_dev, const uint8_t* hdr_pn_dev, uint8_t* ok_dev, int32_t* val_dev,
                    float* score_dev, int32_t* best_s_dev, void* stream);

/* Peak-addressed forms of the two calls above: record i is read in place from row r of y at start s,
 *   r = row_dev ? row_dev[i] : i,   s = start_dev ? max(start_dev[i * start_stride], 0) : 0,
 * i.e. output i is what es_llr_batch / es_header_batch give for the gathered record y[r] with start s (bit for bit), with no
 * gathered copy.  band_dev, pn_dev / hdr_pn_dev and every output are indexed by i, not by r.
 *   y_dev        [n_rows][T] float64 band-passed records (n_rows >= 1 when B > 0)
 *   row_dev      [B] int32 (nullable); a row outside [0, n_rows) gives the output of a start at or past T (an empty frame) and
 *                reads nothing of y
 *   start_dev    int32, element i at start_dev[i * start_stride] (nullable); start_stride >= 1 -- ES_MAX_PEAKS with the peaks_dev
 *                of a sync call means "the first detected peak" (-1 = none: read as 0)
 *   replaces the frame = y[start : start+1215] step of _scan_band_multi_frame (rtwm/detector.py:110-161) before _llr /
 *   _decode_header                                                                                                           */
int es_llr_at_batch(es_ctx* ctx, const double* y_dev, int64_t n_rows, int T, int64_t B, const int32_t* row_dev,
                    const int32_t* start_dev, int start_stride, const uint8_t* band_dev, const uint8_t* pn_dev, int variant,
                    float* llr_dev, int32_t* best_s_dev, float* score_dev, void* stream);
int es_header_at_batch(es_ctx* ctx, const double* y_dev, int64_t n_rows, int T, int64_t B, const int32_t* row_dev,
                       const int32_t* start_dev, int start_stride, const uint8_t* band_dev, const uint8_t* hdr_pn_dev,
                       uint8_t* ok_dev, int32_t* val_dev, float* score_dev, int32_t* best_s_dev, void* stream);

/* Polar(1024,448)+CRC-8 decode: hard-decision shortcut and successive-cancellation list.
 *   replaces PolarCode.decode (rtwm/fastpolar.py:254-359) up to validator selection
 *   llr_dev         [B][1024] ES_DTYPE_F32 or ES_DTYPE_F64
 *   list_size       1..1024 (<= the context's list_size_max); any size, as in the reference: a size that is not a power of
 *                   two runs on the next power of two's kernel with the surplus paths switched off
 *   skip_if_hard_ok non-zero: records whose hard decision passes CRC skip the list loop
 *                   (the reference's behaviour when validator is None, fastpolar.py:268-276); the lane-per-path kernel then
 *                   fills its waves with the records that do not pass (drawn from a per-launch counter), so a batch of
 *                   mostly clean records costs what its noisy ones cost
 *   hard_info_dev   [B][55], hard_ok_dev [B]
 *   cand_info_dev   [B][L][55] candidates in ascending path-metric (stable) order
 *   cand_metric_dev [B][L] float64, cand_ok_dev [B][L] CRC flags
 *   ncand_dev       [B] int32: L, or 0 when the list loop was skipped (the record's candidate rows then read as zeros), or -1: the
 *                   kernel could not decode the record (its block found no free slot of the scratch slab -- not reachable while resident
 *                   blocks <= slots; reported, never silent: es_select_batch turns it into ok = -2 and the host layer raises) */
int es_scl_batch(es_ctx* ctx, const void* llr_dev, int dtype, int64_t B, int list_size,
                 int skip_if_hard_ok, uint8_t* hard_info_dev, uint8_t* hard_ok_dev,
                 uint8_t* cand_info_dev, double* cand_metric_dev, uint8_t* cand_ok_dev,
                 int32_t* ncand_dev, void* stream);

/* Polar encode (CRC-8 append, placement, butterfly): replaces PolarCode.encode
 * (rtwm/fastpolar.py:237-252).  info_dev [B][55] packed, code_dev [B][1024] uint8 {0,1}.      */
int es_polar_encode_batch(es_ctx* ctx, const uint8_t* info_dev, int64_t B, uint8_t* code_dev,
                          void* stream);

/* Key / PN / hop schedule on the device (schedule half of f-3): for each frame counter the 152
 * packed PN bytes of SecureChannel.pn_bits (rtwm/crypto.py:46-48 -> rtwm/utils.py:115-132: AES-128-ECB of
 * (ctr << 64 | j), j = 0..9, MSB-first bits) and the band index of choose_band (rtwm/utils.py:27-36:
 * HMAC-SHA256(band_key, ctr_be32)[0] % 4).  aes_key16_host = StreamPRNG's 16-byte sub-key, band_key32_host = the hop key
 * (the raw master key in the reference, rtwm/detector.py:31); counters are ctr_dev[i] (uint32) or, when ctr_dev is
 * NULL, ctr0 + i.  pn_rows_dev [n][152], band_dev [n]: the layout es_llr_batch / es_bpf_batch consume.            */
int es_schedule_batch(es_ctx* ctx, const uint8_t* aes_key16_host, const uint8_t* band_key32_host, const uint32_t* ctr_dev,
                      uint32_t ctr0, int64_t n, uint8_t* pn_rows_dev, uint8_t* band_dev, void* stream);

/* Frame generator: replaces WatermarkEmbedder._make_frame_chips for a batch
 * (rtwm/embedder.py:78-141): +-1 chips = 63 preamble | 128 header (lo16(ctr) MSB first, each bit 8 times, times the
 * header PN) | 1024 payload chips (code bit i times PN bit 191+i); band-pass of the frame's band with zero initial
 * state; if max|chips| + 1e-12 > 3 the frame is scaled by its reciprocal; float32 out.
 * code_dev [B][1024] {0,1} (es_polar_encode_batch), pn_rows_dev [B][152] and band_dev [B] (es_schedule_batch or the
 * broadcast schedule), ctr_dev [B] uint32; preamble8_host = np.packbits(mseq_63()) (8 bytes, last bit unused),
 * hdr_pn16_host = np.packbits(pn_bits(0, 128)); y_ws_dev = float64 workspace [B][1215]; frames_dev float32 [B][1215].
 * Both host arrays are read during the call and travel by value as kernel arguments: the call only enqueues and can be captured into a
 * graph, and calls under different keys on different streams share nothing. */
int es_tx_frames_batch(es_ctx* ctx, const uint8_t* code_dev, const uint8_t* pn_rows_dev, const uint8_t* band_dev,
                       const uint32_t* ctr_dev, const uint8_t* preamble8_host, const uint8_t* hdr_pn16_host, int64_t B,
                       double* y_ws_dev, float* frames_dev, void* stream);

/* Level mix, the last step of the transmit chain: replaces WatermarkEmbedder.process (rtwm/embedder.py:44-75) for a batch of
 * recordings.  x_dev float32 [R][n]; recording r is cut into blocks of `block` samples (the last one may be short) and each block is
 * what one process() call sees: in_rms = sqrt(mean(x * x)) + 1e-12 in float32 with NumPy's summation order (chunks of 8192 elements,
 * each summed pairwise: echoseal_amd/csrc/es_mix.hip), scale = max(alpha * in_rms, floor), limited to (0.98 - max|x|) / (max|chips| + 1e-12)
 * and to >= 0 (float64, Python's max / min, a NaN wins np.max), out = x + chips * (float)scale in float32.  alpha = db_to_lin(target_rel_db)
 * and floor = db_to_lin(floor_rel_dbfs) come from the host.  chips_dev float32 [R][chips_stride]: row r is the chip stream of recording r,
 * the frames of consecutive counters back to back (what es_tx_frames_batch writes for consecutive counters); sample t of recording r takes
 * chips[r][chip_off[r] + t] (chip_off_dev int64 [R], NULL = 0).  chips_stride is the row stride and the row's length: an offset that
 * leaves the row cannot be seen from the host, such reads are clamped to the row's first / last chip.  out_dev float32 [R][n]; out_dev == x_dev
 * (in place) is allowed, any other overlap is ES_EINVAL.  scale_dev nullable float64 [R][ceil(n / block)]: the gain of every block.
 * Bit-identical to the host code for every block length >= 1; blocks of 1024 samples (the reference's own, rtwm/audioio.py:18) in rows of
 * n % 4 == 0 samples at 16-byte aligned pointers run one wavefront per block.  Needs no tables (works before es_set_tables and on a
 * front-end context), only enqueues (capturable); R == 0 or n == 0 launches nothing.  NaN payloads other than those of the inputs are
 * those of SSE arithmetic (an invalid operation gives the negative quiet NaN).                                                       */
int es_mix_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n, int block, const float* chips_dev, int64_t chips_stride,
                 const int64_t* chip_off_dev, double alpha, double floor, float* out_dev, double* scale_dev, void* stream);

/* Input conditioning: the polyphase FIR inside resample_to (rtwm/utils.py:58-66 =
 * scipy.signal.resample_poly(audio, up, down) -> upfirdn, zero extension).  The caller designs the filter exactly as
 * SciPy does (firwin, Kaiser 5.0, scaled by `up`, padded) and passes it in SciPy's transposed / flipped polyphase layout
 * (h_tf_dev, `up` phases of h_per_phase taps, element type = dtype); x_dev [B][n_in] and out_dev [B][n_out] have the same
 * element type (ES_DTYPE_F32 for float32 signals, ES_DTYPE_F64 otherwise: SciPy's output type).  Output k of a row is
 * sample y0 + k of the full upfirdn result (y0 = SciPy's n_pre_remove).  Bit-identical to SciPy 1.15's compiled loop.  One rate pair and
 * one length per call, a lane per output with everything read through L2: the yardstick of es_resample_ragged_batch below, which is what
 * the detector's batch calls use. */
int es_resample_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t B, int64_t n_in, const void* h_tf_dev, int h_per_phase,
                      int up, int down, int64_t y0, int64_t n_out, void* out_dev, void* stream);

/* The same conditioning for a queue of clips of unequal length AND rate in one launch: what a batch call needs before es_sync_ragged_batch.
 * The clips' samples lie back to back, unpadded, in ONE pool (pool_dev, pool_n elements of `dtype`: ES_DTYPE_I16, ES_DTYPE_F32 or
 * ES_DTYPE_F64), their polyphase filters, one copy per distinct filter, in another (filt_dev, filt_n elements: float32 for int16 and
 * float32 samples, float64 for float64 samples -- SciPy's output type).  Record r is desc_dev[r][ES_RESAMPLE_DESC_WORDS] int64:
 *   [0] offset of its first sample in the pool   [1] n_in   [2] up   [3] down   [4] offset of its filter in the filter pool
 *   [5] taps per phase   [6] y0, first kept output of the full upfirdn result   [7] n_out
 * -- [2], [3], [5], [6], [7] and the filter are what es_resample_batch takes (utils.resample_plan).  Output: out_dev float32, rows of
 * out_stride; record r fills rows r * rep .. r * rep + rep - 1 with the same n_out values (rep >= 1: a sync row per band), samples past
 * n_out of a row are never written.  Each value is es_resample_batch's, bit for bit: an int16 sample enters as (float)s / 32768.0f, a
 * float64 record is computed in float64 and rounded once to float32 on store.  A record with up == down is copied (int16 converted),
 * bit patterns and signed zeros kept.  The descriptors are device data the host cannot refuse: n_out is clamped to out_stride, reads to
 * the record's own [offset, offset + n_in) inside the pool, and a record whose filter does not lie inside the filter pool (or with
 * up, down or taps per phase outside [1, ES_RESAMPLE_RATE_MAX], or a table above ES_RESAMPLE_TABLE_MAX values) writes nothing.  max_out >= every n_out sizes the grid (tiles of ES_RESAMPLE_TILE
 * outputs; a larger n_out is cut to it).  Needs no tables, only enqueues (capturable); R == 0 or max_out == 0 launches nothing. */
#define ES_RESAMPLE_DESC_WORDS 8
#define ES_RESAMPLE_TILE    1024
/* The kernel's own constants, stated here for the host (es_resample.hip keeps them as RS_WIN_MAX, RS_FILT_MAX, RS_RATE_MAX and a literal;
 * tests/test_condition_host.py holds the two files equal).  A tile whose input window has at most WIN_MAX samples is staged in LDS, a
 * polyphase table of at most FILT_MAX values too; larger ones are read through L2.  A record whose reduced up, down or taps per phase
 * exceed RATE_MAX, or whose table has more than TABLE_MAX values, is the one the kernel writes nothing for: utils.condition_plan refuses
 * it by name and scan.cut_launches conditions such a clip on the single-clip path instead. */
#define ES_RESAMPLE_WIN_MAX   4352
#define ES_RESAMPLE_FILT_MAX  3584
#define ES_RESAMPLE_RATE_MAX  (1 << 20)
#define ES_RESAMPLE_TABLE_MAX (1 << 30)
int es_resample_ragged_batch(es_ctx* ctx, const void* pool_dev, int dtype, int64_t pool_n, const void* filt_dev, int64_t filt_n,
                             const int64_t* desc_dev, int64_t R, int rep, float* out_dev, int64_t out_stride, int64_t max_out,
                             void* stream);

/* The same conditioning for live streams that arrive chunk by chunk at rates of their own: what a monitor runs in front of
 * es_bpf_stream_batch.  Continues resample_to (rtwm/utils.py:58-66 = scipy.signal.resample_poly) across calls.
 * Definition.  Stream s has a rate pair reduced to (up, down), fixed when its slot is opened, and has received n samples X (float32, or
 * int16 read as x / 32768).  With half_len = 10 max(up, down), n_pre_pad = down - half_len % down and y0 = (half_len + n_pre_pad) / down,
 *   F(n) = max(0, (n up - 1) / down - y0 + 1),  F(0) = 0
 * is the number of leading outputs of resample_poly(X[:n], up, down) that no later sample changes: output k is final once its newest input
 * sample, ((y0 + k) down) / up, has arrived.  The stream's conditioned stream is r = resample_poly(X, up, down)[:F(n)], float32; a call
 * that takes a stream from n_old to n_old + len samples writes r[F(n_old) : F(n_old + len)], bit for bit (accumulator from +0, products in
 * ascending input index, multiply and add rounded separately), possibly no sample at all.  Finite samples only: an Inf or NaN that meets
 * a zero tap makes SciPy's own value depend on the clip's length.
 *   rate_dev [S][ES_RSTREAM_RATE_WORDS] int64   (up, down, offset of the filter in the filter pool, taps per phase hpp, y0); up == down:
 *                                               a stream at the target rate, copied
 *   filt_dev [filt_n] float32                   polyphase tables in utils.resample_plan's transposed, flipped layout, without post padding:
 *                                               hpp = ceil((2 half_len + 1 + n_pre_pad) / up) <= ES_RSTREAM_TAIL
 *   tail_dev [S][ES_RSTREAM_TAIL] float32       the last samples received, newest last (+0.0 in a fresh slot); the kernel reads the last 255
 *   nin_dev  [S] int64                          samples received (0 in a fresh slot)
 * Record r = the chunk x_dev[r][0 : len[r]] (rows of n_stride, ES_DTYPE_F32 or ES_DTYPE_I16) of stream sid[r]; its outputs go to
 * out_dev[r][0 : count] (float32, rows of out_stride), the rest of the row is not written.  Then, by a second kernel behind the first,
 * tail := the last of (tail ++ chunk as float32) and nin += len.  rec_host [R][ES_RSTREAM_REC_WORDS] int64 = (sid, len, n_old, F(n_old),
 * count, up, down, y0) as the host laid the tick out, checked before anything is enqueued: ES_EINVAL for a sid outside [0, S) or named
 * twice, len outside 0 .. n_stride, up or down outside [1, ES_RESAMPLE_RATE_MAX], a position with (n_old + len) up >= 2^62, F(n_old) or
 * count that disagree with the rate words, a count above out_stride; nothing is written then.  The device arrays must hold the same; what
 * they hold instead is clamped (a sid outside the table or rate words no filter in the pool fits: no output; len to the chunk row, the
 * count to the output row; no read or write leaves x, the table or out).  The kernels take n_old from nin_dev, so a captured call
 * continues its streams on every replay.  Needs no tables, only enqueues (capturable); R == 0 launches nothing. */
#define ES_RSTREAM_REC_WORDS  8
#define ES_RSTREAM_RATE_WORDS 5
#define ES_RSTREAM_TAIL       256
#define ES_RSTREAM_Y0_MAX     (1 << 24)
int es_resample_stream_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t R, int64_t n_stride, const int64_t* sid_dev,
                             const int64_t* len_dev, const int64_t* rec_host, int64_t S, const int64_t* rate_dev, const float* filt_dev,
                             int64_t filt_n, float* tail_dev, int64_t* nin_dev, float* out_dev, int64_t out_stride, void* stream);

/* Diagnostic: out[i] = log1p(exp(t[i])) for t[i] <= 0 exactly as the list decoder's f / penalty evaluate it on the device
 * (np.logaddexp / np.log1p(np.exp(.)) of rtwm/fastpolar.py:18-23, 32-40 through the C library's exp and log1p) -- lets a
 * test compare the device arithmetic with the host C library bit for bit.  t_dev, out_dev float64 [n].                   */
int es_softplus_batch(es_ctx* ctx, const double* t_dev, int64_t n, double* out_dev, void* stream);

/* Diagnostic: f(a[i], b[i]) as the lane-per-path list decoder's hot loops evaluate it on the device (es_softplus_dev.h), with its two
 * softplus terms: out_dev float64 [3][n] = f, log1p(exp(-|a-b|)), log1p(exp(-|a+b|)); bad_dev int32 [n] = 1 where |a-b| or |a+b| is
 * outside the straight-line form's range (the three values are then unspecified).  a_dev, b_dev float64 [n].                          */
int es_polar_f_batch(es_ctx* ctx, const double* a_dev, const double* b_dev, int64_t n, double* out_dev, int32_t* bad_dev, void* stream);

/* Tuning knobs; results never depend on them.  es_scl_batch has three mappings of list paths to lanes for lists of up to
 * 32 paths: one frame per wavefront (a path owns 64/L lanes: lowest latency, one wavefront per SIMD), several frames per
 * wavefront (a path owns 4 or 2 lanes: 16 or 32 paths per wavefront, three wavefronts per SIMD), and one lane per path (64/L
 * frames per wavefront, every lane busy at every tree depth: fewest instructions per frame, but a wavefront carries 64/L
 * frames through the whole decode, so it wants tens of thousands of frames per launch; the kernel that also serves lists of
 * 64..1024 paths).  "scl_multi": -1 (default) chooses by batch size, 0 forces one frame per wavefront, 1 several.
 * "scl_lanes": lanes per path of the latter -- 4, 2, 1, or 0 (default: by batch size; 1 only when the context has that
 * kernel's scratch slab).  "scl_lane_slab" = 1 allocates that slab (1.6 GB; contexts created with list_size_max > 32 have
 * it from the start) without forcing anything: an allocation, so it belongs next to es_create / es_reserve, never between
 * enqueue calls that must not synchronise.  "scl_lanes" = 1 allocates it too.  "scl_prio" (0..3, default 0): wave priority
 * of the one-lane-per-path launches that follow -- a pipeline gives the later launch of a burst 1 so that it does not finish as
 * much later as it started (the short front-end kernels issue at 2 and 3).                                                                          */
int es_set_option(es_ctx* ctx, const char* name, int value);

/* ---- the step after the list decoder ------------------------------------------------
 * Payload validator: replaces the Python closure the reference passes to PolarCode.decode
 * (rtwm/detector.py:168-176): SecureChannel.open (rtwm/crypto.py:39-43: blob = nonce 12 | ciphertext 27 | tag 16,
 * ChaCha20-Poly1305 per RFC 8439, no AAD), plaintext starts with "ESAL", plaintext[4:8] big endian == counter.
 * blobs_dev [n][55]; blob i is checked against ctr_dev[i / group] (group = L for a [B][L][55] candidate array,
 * 1 for [B][55]); key32_host = the 32-byte AEAD key (host memory, passed by value to the kernel);
 * ok_dev [n] 1/0; plain_dev nullable [n][27] (plaintext when the tag verifies, zeros otherwise).               */
int es_aead_check_batch(es_ctx* ctx, const uint8_t* key32_host, const uint8_t* blobs_dev, int64_t n, int group,
                        const uint32_t* ctr_dev, uint8_t* ok_dev, uint8_t* plain_dev, void* stream);

/* The producer side of the same AEAD: SecureChannel.seal (rtwm/crypto.py:33-37) for 27-byte plaintexts with given
 * nonces: blobs_dev [n][55] = nonce 12 | ciphertext 27 | tag 16 (what the embedder puts into a frame, rtwm/embedder.py:153-168).
 * nonces_dev [n][12], plain_dev [n][27].                                                                            */
int es_aead_seal_batch(es_ctx* ctx, const uint8_t* key32_host, const uint8_t* nonces_dev, const uint8_t* plain_dev, int64_t n,
                       uint8_t* blobs_dev, void* stream);

/* Candidate selection: replaces the tail of PolarCode.decode (rtwm/fastpolar.py:268-276, 332-359) over the outputs
 * of es_scl_batch: the hard candidate if its CRC holds and the validator accepts it; else the first list candidate
 * (ascending metric) whose CRC holds and which the validator accepts (ok = 1); else the lowest-metric CRC-ok
 * candidate; else the lowest-metric candidate (ok = 0).  key32_host == NULL means validator=None; otherwise the
 * validator is the one of es_aead_check_batch with ctr_dev [B].  payload_dev [B][55]; ok_dev [B] int8 (1, 0, or
 * -1 when ncand is 0 although the shortcut did not return: run es_scl_batch with skip_if_hard_ok = 0 when a
 * validator is used; -2 when ncand is negative: es_scl_batch reported that it could not decode the record -- its payload row
 * is zeroed); which_dev [B] int32 (-1 = hard candidate, else list index).                              */
int es_select_batch(es_ctx* ctx, const uint8_t* key32_host, const uint32_t* ctr_dev, int64_t B, int L,
                    const uint8_t* hard_info_dev, const uint8_t* hard_ok_dev, const uint8_t* cand_info_dev,
                    const double* cand_metric_dev, const uint8_t* cand_ok_dev, const int32_t* ncand_dev,
                    uint8_t* payload_dev, int8_t* ok_dev, int32_t* which_dev, void* stream);

/* ---- many keys at once: "which of the N keys we issued marked this clip?" ---------------------------------------------
 * Key ring: everything the keyed kernels need of a 32-byte master key, derived on the device, one lane per key.  Replaces
 * SecureChannel.__init__ (rtwm/crypto.py:19-30: HKDF-SHA256(master, salt none, info "EchoSeal:KDF:v1", 64 bytes) -> AEAD key |
 * PRNG seed), StreamPRNG.__init__ (rtwm/utils.py:86-88: BLAKE2s(seed, digest 16, person "EchoSeal") -> AES-128 key), the AES key
 * expansion and HMAC pad blocks that es_schedule_batch does on the host, WatermarkDetector.__init__'s header PN
 * (rtwm/detector.py:36: pn_bits(0, 128)) and the first band of its band order (rtwm/detector.py:46: choose_band(key, 0)).
 * master32_dev [N][32]; ring_dev [N][ES_KEYRING_BYTES], 16-byte aligned.  Row layout (byte offsets):
 *     0  AEAD key, 32 bytes as SecureChannel holds them
 *    32  44 AES round-key words (FIPS 197 w[0..43], each a native uint32 whose top byte is the word's first byte)
 *   208  SHA-256 state (8 native uint32) after the HMAC inner pad block of the hop key (= the master key, rtwm/detector.py:31)
 *   240  the same after the outer pad block
 *   272  header PN, 16 bytes = np.packbits(pn_bits(0, 128))
 *   288  hop0 = band index of counter 0; 289..303 zero                                                                     */
int es_keyring_derive_batch(es_ctx* ctx, const uint8_t* master32_dev, int64_t N, uint8_t* ring_dev, void* stream);

/* es_schedule_batch for records of several keys: record i = (ring row key_dev[i], counter ctr_dev[i]); replaces the same reference
 * lines (rtwm/crypto.py:46-48, rtwm/utils.py:27-36, 115-132) per (key, counter).  key_dev [n] int32, ctr_dev [n] uint32; outputs as
 * es_schedule_batch.  Either output may be NULL; with pn_rows_dev == NULL the ten AES blocks are skipped (bands only: the hop
 * table of es_plan_batch).  A key index outside [0, N) gives band 0 and a zero PN row and reads nothing of the ring (the indices
 * are device data: the host cannot refuse them); N == 0 with n > 0 is ES_EINVAL.  Records sorted by key read the ring best. */
int es_schedule_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint32_t* ctr_dev, int64_t n,
                            uint8_t* pn_rows_dev, uint8_t* band_dev, void* stream);

/* es_aead_check_batch / es_select_batch with the AEAD key of ring row key_dev[r] in place of key32_host, r = i / group for the
 * check (one key and one counter per group) and r = the record for the selection (key_dev [B]); same outputs, same ok codes
 * (-1 and -2 included).  A key index outside [0, N) is a validator that accepts nothing (ok 0, zero plaintext).              */
int es_aead_check_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* blobs_dev, int64_t n,
                              int group, const uint32_t* ctr_dev, uint8_t* ok_dev, uint8_t* plain_dev, void* stream);
int es_select_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint32_t* ctr_dev, int64_t B, int L,
                          const uint8_t* hard_info_dev, const uint8_t* hard_ok_dev, const uint8_t* cand_info_dev,
                          const double* cand_metric_dev, const uint8_t* cand_ok_dev, const int32_t* ncand_dev,
                          uint8_t* payload_dev, int8_t* ok_dev, int32_t* which_dev, void* stream);

/* Candidate planning: replaces the (peak, counter) loop of _scan_band_multi_frame (rtwm/detector.py:105-142) for every
 * (key, row) at once, row = one band-passed record of a sync call.  One wave per pair k * rows + r:
 *   - of the first min(npeaks_dev[r] & 0xFFFF, ES_PEAK_LIMIT) entries of peaks_dev [rows][ES_MAX_PEAKS] only those with
 *     0 <= start and start + 1215 <= T are looked at, in order, while fewer than ES_MAX_TRIES candidates are planned;
 *   - the j-th of them (j from 0) has its header result at hdr_ok_dev / hdr_lo16_dev [k * P + hdr_base_dev[r] + j] (the outputs of
 *     one es_header_at_batch over key-major (key, fitting peak) records; P = fitting peaks of all rows);
 *   - ctr_est = (2 * start + 1215) / 2430 (= round(start / 1215)); header ok: counters of [max(0, ctr_est - 200), ctr_est + 200]
 *     with (ctr & 0xFFFF) == lo16 and hop_dev[k * C + ctr] == rowband_dev[r]; else the +-3 window gated by the hop alone and,
 *     only if that is empty, the +-200 window gated by the hop alone;
 *   - at most ES_MAX_TRIES candidates per pair: the last peak's list is cut, later peaks are not looked at.
 * hop_dev [N][C] uint8 = band of (key, counter), C >= ceil(T / 1215) + 201 (else ES_EINVAL): es_schedule_keyed_batch, bands only.
 * Out, per pair: cand_slot_dev [N * rows][ES_MAX_TRIES] uint8 (index into the row's peaks) and cand_ctr_dev [..][ES_MAX_TRIES]
 * uint32 in try order (entries past the count are not written), count_dev [N * rows] int32, looked_dev (nullable) = fitting peaks
 * looked at (the length of the scan's header log).  Needs no tables, only enqueues.                                           */
int es_plan_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev, const int32_t* hdr_base_dev,
                  int64_t rows, int T, const uint8_t* hdr_ok_dev, const int32_t* hdr_lo16_dev, int64_t P, const uint8_t* hop_dev, int64_t N,
                  int C, uint8_t* cand_slot_dev, uint32_t* cand_ctr_dev, int32_t* count_dev, int32_t* looked_dev, void* stream);

/* es_plan_batch for the rows of an es_sync_ragged_batch call: len_dev [rows] int32 takes the place of T in the test of which peaks
 * can hold a frame, 0 <= start and start + 1215 <= len_dev[r]; T_max (the longest record) that of T in the bound on the hop table,
 * C >= ceil(T_max / 1215) + 201.  The lengths are taken as given, not clamped (there is no row stride here to clamp them to): T_max
 * must be at least every len_dev[r]; with a larger length the counters a window reaches past the hop table are skipped (every hop read
 * is guarded by ctr < C), so the call stays in bounds but plans fewer candidates than the rules give.  Everything else -- outputs, try order, the ES_MAX_TRIES cut -- as es_plan_batch.                 */
int es_plan_ragged_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev,
                         const int32_t* hdr_base_dev, int64_t rows, const int32_t* len_dev, int T_max, const uint8_t* hdr_ok_dev,
                         const int32_t* hdr_lo16_dev, int64_t P, const uint8_t* hop_dev, int64_t N, int C, uint8_t* cand_slot_dev,
                         uint32_t* cand_ctr_dev, int32_t* count_dev, int32_t* looked_dev, void* stream);

/* es_plan_ragged_batch for rows that lie somewhere in a marked stream (a monitor's window, a clip cut out of a session): row r starts at
 * absolute stream sample pos0_dev[r] (int64 [rows], 0 <= pos0 < 2^62; 0 for a clip) of a stream whose frame k carries counter
 * ctr0_dev[r] + k (uint32 [rows]).  Line 117 of the reference (rtwm/detector.py: ctr_est = int(round(start / FRAME_LEN))) becomes
 *     ctr_est = ctr0 + (2 * (pos0 + start) + 1215) / 2430                      in 64-bit integers;
 * everything else of rtwm/detector.py:105-142 is es_plan_batch's: the low-16 header gate, the +-3 then +-200 windows, max(0, .), the hop
 * gate, ES_PEAK_LIMIT peaks, ES_MAX_TRIES tries, the try order.  A counter above 2^32 - 1 is never a candidate.
 * hop_dev [N][HR][C] uint8: HR hop rows per key, column 0 of row h is counter hop_base_dev[h] (uint32 [HR]) -- es_hop_window_batch; the pair
 * (k, r) reads hop_dev[(k * HR + hop_row_dev[r]) * C + (ctr - hop_base_dev[hop_row_dev[r]])] (hop_row_dev int32 [rows]), every read guarded
 * by 0 <= column < C: a counter outside the hop row is skipped.  A hop_row outside [0, HR) plans nothing for the row (count 0, looked 0).
 * Host contract: hop_base = max(0, ctr0 + (2 * pos0 + 1215) / 2430 - 200) for every row that reads the hop row; with
 * C >= ceil(T_max / 1215) + 402 (else ES_EINVAL, as HR < 1) the row then covers every counter the rules reach from a row of at most T_max
 * samples.  With pos0 = ctr0 = 0, one hop row and base 0 the outputs are es_plan_ragged_batch's.  A refused call enqueues nothing;
 * rows * N == 0 is ES_OK.  Outputs as es_plan_batch.  Needs no tables, only enqueues.                                              */
int es_plan_at_batch(es_ctx* ctx, const int32_t* peaks_dev, const int32_t* npeaks_dev, const uint8_t* rowband_dev, const int32_t* hdr_base_dev,
                     int64_t rows, const int32_t* len_dev, int T_max, const uint8_t* hdr_ok_dev, const int32_t* hdr_lo16_dev, int64_t P,
                     const uint8_t* hop_dev, int64_t N, int C, const int64_t* pos0_dev, const uint32_t* ctr0_dev, const int32_t* hop_row_dev,
                     const uint32_t* hop_base_dev, int HR, uint8_t* cand_slot_dev, uint32_t* cand_ctr_dev, int32_t* count_dev,
                     int32_t* looked_dev, void* stream);

/* The hop rows of es_plan_at_batch, filled on the device: hop_dev[(k * HR + h) * C + col] = band of counter hop_base_dev[h] + col under
 * key k, one lane per entry -- choose_band (rtwm/utils.py:27-36) from the ring's HMAC pad states, as es_schedule_keyed_batch with
 * pn_rows_dev == NULL, without a list of (key, counter) records to upload.  A counter past 2^32 - 1 gets 0xFF, which matches no band.
 * hop_base_dev [HR] uint32.  N * HR * C == 0 is ES_OK; a negative count or a null pointer with work to do is ES_EINVAL.  Only enqueues. */
int es_hop_window_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const uint32_t* hop_base_dev, int64_t HR, int64_t C, uint8_t* hop_dev,
                        void* stream);

/* ---- acquisition: the counters a decoded header may belong to, over a span of the whole 32-bit range -------------------------------
 * Extends rtwm/detector.py:117-127 (ctr_est = int(round(start / FRAME_LEN)); the low-16 gate over ctr_est +- 200): where the caller does
 * not know where in its stream a clip or a window lies, the estimate says nothing, and what is left of lines 122-127 is the header's low
 * half and the hop (rtwm/utils.py:27-36) -- over every counter there is.  A record p is one (key, fitting peak) pair with its header decode,
 * as one es_header_at_batch gives it: ring row key_dev[p] (int32), ok_dev[p] (uint8), lo16_dev[p] (int32) and band_dev[p] (uint8), the band
 * of the sync row the peak was found in.  The span [ctr_lo, ctr_hi) is given in 64-bit integers, 0 <= ctr_lo <= ctr_hi <= 2^32; with
 *     h0 = ctr_lo >> 16,   h1 = (ctr_hi + 65535) >> 16,   H = h1 - h0,   W = ceil(H / 32)
 * es_acquire_mask_batch writes mask_dev [P][W] uint32: bit (h - h0) & 31 of word (h - h0) >> 5 of row p is set exactly when ok_dev[p] != 0,
 * 0 <= key_dev[p] < N, 0 <= lo16_dev[p] <= 65535, c = (h << 16) | lo16_dev[p] lies in [ctr_lo, ctr_hi) and the band of counter c under
 * ring row key_dev[p] (HMAC-SHA256 from the row's pad states, as es_hop_window_batch) equals band_dev[p].  One lane per (record, h); every
 * word of every row is written, zeros included; count_dev [P] int32 = the set bits of each row, summed by a second launch over the finished
 * rows (no atomics: the same on every run).  A record that is not ok, or whose key or low half is out of range, reads nothing of the ring.
 * ES_EINVAL, with nothing enqueued and nothing written: a negative count, a span outside [0, 2^32] or reversed, N < 1 or a null pointer
 * with work to do, more than 2^31 - 1 workgroups (four (record, 64 high halves) tiles each: the grid is exact, P * H is small in every real
 * call).  P == 0 or H == 0: ES_OK, nothing enqueued.  Needs no tables, only enqueues.                                                   */
int es_acquire_mask_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* ok_dev, const int32_t* lo16_dev,
                          const uint8_t* band_dev, int64_t P, int64_t ctr_lo, int64_t ctr_hi, uint32_t* mask_dev, int32_t* count_dev, void* stream);

/* The set bits of es_acquire_mask_batch's rows as a flat candidate list, in an order the host chooses after reading the P counts: for every
 * record p with base_dev[p] >= 0 (int64 [P]) the i-th set bit of row p, h ascending, becomes
 *     cand_rec_dev[base_dev[p] + i] = p (int32),   cand_ctr_dev[base_dev[p] + i] = (h << 16) | (lo16_dev[p] & 0xFFFF) (uint32).
 * A record with base_dev[p] < 0 is skipped.  Nothing outside the named ranges is written, and no entry at or past `total`, the entries of
 * the two output arrays (the host's ranges, base[p] + count[p] <= total, are disjoint by its own choice).  One wave per (record, 64 high
 * halves): the order inside comes from the wave's ballot, the offset from the popcounts of the row's words before it, which the wave sums
 * itself -- no workgroup waits for another, no atomic decides an order.  mask_dev, the span and P as in the mask call.  Refusals as
 * es_acquire_mask_batch (and total < 0); P == 0, H == 0 or total == 0: ES_OK, nothing enqueued.  Needs no tables, only enqueues.          */
int es_acquire_list_batch(es_ctx* ctx, const uint32_t* mask_dev, const int32_t* lo16_dev, int64_t P, int64_t ctr_lo, int64_t ctr_hi,
                          const int64_t* base_dev, int64_t total, int32_t* cand_rec_dev, uint32_t* cand_ctr_dev, void* stream);

/* ---- the transmit side for many keys: clips of unequal length, each marked under its own key, in one launch sequence ----------
 * es_aead_seal_batch with the ChaCha20 key of ring row key_dev[i] (read as es_aead_check_keyed_batch reads it) in place of key32_host:
 * SecureChannel.seal (rtwm/crypto.py:33-37) per (key, blob), what WatermarkEmbedder._build_payload puts into a frame
 * (rtwm/embedder.py:153-168).  key_dev [n] int32, nonces_dev [n][12], plain_dev [n][27] -> blobs_dev [n][55].  A key index outside
 * [0, N) reads nothing of the ring and writes a zero blob (the indices are device data: the host cannot refuse them); N == 0 with
 * n > 0 is ES_EINVAL.  Needs no tables, only enqueues.                                                                            */
int es_aead_seal_keyed_batch(es_ctx* ctx, const uint8_t* ring_dev, int64_t N, const int32_t* key_dev, const uint8_t* nonces_dev,
                             const uint8_t* plain_dev, int64_t n, uint8_t* blobs_dev, void* stream);

/* es_tx_frames_batch (rtwm/embedder.py:78-141) for frames of several keys: the header PN of frame f (rtwm/embedder.py:50, 105:
 * pn_bits(0, 128) of the frame's key) is the 16 bytes at offset 272 of ring row key_dev[f]; pn_rows_dev and band_dev come from
 * es_schedule_keyed_batch over the same (key, counter) records.  Band-pass and peak rule are those of es_tx_frames_batch.  key_dev [B]
 * int32; a key index outside [0, N) gives a header PN of zero bytes and reads nothing of the ring; N == 0 with B > 0 is ES_EINVAL.
 * Like es_tx_frames_batch it only enqueues and can be captured into a graph (preamble8_host is read during the call and travels by
 * value).                                                                                                                          */
int es_tx_frames_keyed_batch(es_ctx* ctx, const uint8_t* code_dev, const uint8_t* pn_rows_dev, const uint8_t* band_dev,
                             const uint32_t* ctr_dev, const uint8_t* preamble8_host, const uint8_t* ring_dev, int64_t N,
                             const int32_t* key_dev, int64_t B, double* y_ws_dev, float* frames_dev, void* stream);

/* es_mix_batch (WatermarkEmbedder.process, rtwm/embedder.py:44-75) for recordings of unequal length.  x_dev / out_dev float32
 * [R][n_stride]; record r is x[r][0 : len[r]], len_dev [R] int64 clamped to [0, n_stride] on the device (the rule of
 * es_sync_ragged_batch).  The record is cut into ceil(len[r] / block) blocks, the last one possibly short, and each block gets exactly the
 * gain and the output es_mix_batch gives the record alone with n = len[r].  chips_dev is ONE flat float32 pool of chips_total chips, the
 * frames back to back as the frame generator writes them; sample t of record r takes chips[chip_base[r] + t] (chip_base_dev,
 * chip_cnt_dev [R] int64).  Chip reads are clamped to [chip_base[r], chip_base[r] + chip_cnt[r] - 1], that range is clamped to the
 * pool (no read ever leaves it), and a record whose clamped range is empty is treated as a record of length 0.
 * Samples of a row past len[r] may hold anything.  out[r][len[r]:] and the scale_dev entries of block slots past a record's last block
 * are NOT written: in place the padding survives, otherwise whatever the caller put there.  out_dev == x_dev is allowed, any other
 * overlap is ES_EINVAL.  scale_dev nullable float64 [R][ceil(n_stride / block)].
 * With block == 1024, n_stride % 4 == 0 and 16-byte aligned x_dev / out_dev the full blocks run one wavefront per block and each
 * record's short last block on the workgroup kernel; otherwise every block runs on the workgroup kernel.  Block slots wholly past a
 * record's end do no work.  Needs no tables, only enqueues (capturable); R == 0 or n_stride == 0 launches nothing.               */
int es_mix_ragged_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n_stride, const int64_t* len_dev, int block,
                        const float* chips_dev, int64_t chips_total, const int64_t* chip_base_dev, const int64_t* chip_cnt_dev,
                        double alpha, double floor, float* out_dev, double* scale_dev, void* stream);

/* Live streams: many streams, each under its own key, marked chunk by chunk (the reference's WatermarkEmbedder.process keeps its chip
 * buffer and counter between calls, rtwm/embedder.py:34-36,44-75).  A stream table of S rows holds per stream the frame it stands in,
 * tail_dev float32 [S][1215], the chips of that frame already used, off_dev int64 [S] in 0 .. 1214 (0: nothing pending), and the counter
 * of the next frame to generate, ctr_dev int64 [S] in 0 .. 2^32 - 1.
 *
 * es_mix_stream_batch is es_mix_ragged_batch for records that continue streams: record r = x[r][0 : len[r]] is a chunk of stream
 * sid_dev[r] (int64 [R]).  Its chips are the row [tail[sid[r]] | the record's new frames at chips[chip_base[r] ..] of the flat pool]; its
 * first sample takes row position start = off[sid[r]], or 1215 where off is 0, and the record needs
 * ceil((start + len[r]) / 1215) - 1 new frames: chip_cnt[r] is 1215 times that.  Both sources are read where they lie.  Block grid,
 * gains, kernels' cut and what is left unwritten are those of es_mix_ragged_batch; a chunk is mixed exactly as es_mix_batch mixes it alone
 * with the concatenated row and chip_off = start.  The table is only read.
 * rec_host [R][ES_STREAM_REC_WORDS] int64 = (sid, off, len, chip_base, chip_cnt) of every record as the host laid them out, checked
 * before anything is enqueued: ES_EINVAL for a sid outside [0, S) or named twice, off outside 0 .. 1214, len outside 0 .. n_stride, a
 * chip_cnt other than the one above, a pool shorter than chip_base + chip_cnt.  The device arrays must hold the same; what they hold
 * instead is clamped as es_mix_ragged_batch clamps (a sid outside the table: a record of length 0; no read leaves table or pool).
 * chips_dev may be NULL where chips_total == 0 (no record makes a new frame).  Only enqueues; R == 0 or n_stride == 0 launches nothing. */
#define ES_STREAM_REC_WORDS 5
int es_mix_stream_batch(es_ctx* ctx, const float* x_dev, int64_t R, int64_t n_stride, const int64_t* len_dev, int block,
                        const int64_t* sid_dev, int64_t S, const float* tail_dev, const int64_t* off_dev, const float* chips_dev,
                        int64_t chips_total, const int64_t* chip_base_dev, const int64_t* chip_cnt_dev, const int64_t* rec_host,
                        double alpha, double floor, float* out_dev, double* scale_dev, void* stream);

/* The state of the pushed streams after es_mix_stream_batch over the same records, enqueued behind it on the same stream (a launch of
 * its own: many workgroups of the mix read a stream's tail).  With end = start + len[r]: off[sid] = end % 1215, ctr[sid] advances by the
 * record's new frames mod 2^32, and tail[sid] becomes the frame the stream now stands in -- frame end / 1215 of the row where
 * end % 1215 > 0, the frame just used up where the chunk ended on a frame edge, the old tail (left as it is) where that is row frame 0.
 * Rows of streams the records do not name are not touched.  Arguments and refusals as above.                                      */
int es_stream_commit_batch(es_ctx* ctx, int64_t R, int64_t n_stride, const int64_t* len_dev, const int64_t* sid_dev, int64_t S,
                           float* tail_dev, int64_t* ctr_dev, int64_t* off_dev, const float* chips_dev, int64_t chips_total,
                           const int64_t* chip_base_dev, const int64_t* chip_cnt_dev, const int64_t* rec_host, void* stream);

/* ---- the receive side of live streams: a monitor that verifies many streams chunk by chunk ---------------------------------------
 * Definition.  A monitor table holds S stream slots; stream s has received n samples X since it was opened.  Per band,
 * y = lfilter(b, a, X) from zero state at the opening, never restarted, and corr is the normalised correlation of that y, lag i
 * absolute, 0 <= i < n - 62.  The table keeps the recent part of both, linear rows (not a ring: the pick and the peak-addressed calls
 * read 1215 or more contiguous columns):
 *   z_dev         [4 S][8] float64   the band-pass's eight delay elements of row 4 s + j as they stand after sample n - 1 (+0.0 when opened)
 *   pos_dev       [S][2] int64       (n, base): samples received, absolute index of column 0 of the stream's rows; base % 1216 == 0
 *   y_hist_dev    [4 S][H] float64   sample a of row 4 s + j at column a - base
 *   corr_hist_dev [4 S][H] float64   lag a at column a - base
 *   band_dev      [4 S] uint8        band of each row
 * 1216 = 64 * 19 is the correlation kernel's segment and 19 its chunk: the order of a lag's energy sum follows the lag's index mod 19, so
 * any window that starts at a multiple of 19 sees, bit for bit, the correlation values the stream already has.
 *
 * A tick is R records; record r = the chunk x[r][0 : len[r]] of stream sid[r], appended at column col[r] = n_old - base of its rows.
 * rec_host [R][ES_MONITOR_REC_WORDS] int64 = (sid, len, col, move, base) as the host laid them out, checked before anything is enqueued:
 * ES_EINVAL for a sid outside [0, S) or named twice, len outside 0 .. n_stride, a chunk that does not fit its row (col outside 0 .. H or
 * col + len > H), a move that is not a multiple of 1216 with move + col <= H, a base that is not a multiple of 1216; nothing is written
 * then.  The device arrays (int64 [R] each) must hold the same; what they hold instead is clamped (a sid outside the table: a record of
 * length 0; len to the chunk row and to H - col; no read or write leaves x or the table).  Both calls only enqueue (capturable).
 *
 * es_bpf_stream_batch continues rtwm/detector.py:59-60 (y = lfilter(b, a, x)) across calls: the four rows of each record run SciPy's
 * direct-form-II-transposed loop from z over the chunk, x ES_DTYPE_F32 or ES_DTYPE_I16 (read as x / 32768, as es_bpf_batch) in rows of
 * n_stride, and z is stored as it stands after sample len - 1 exactly (len == 0 leaves it): y_hist equals es_bpf_batch over the whole
 * stream, bit for bit, whatever the cuts.  Where move[r] > 0, columns [move, move + col) of the stream's rows of y_hist and corr_hist are
 * first moved down to [0, col) -- the host does this when a chunk would not fit -- and base[r] is the base after that move.  pos is set to
 * (base + col + len, base).  Rows of streams the records do not name are not touched. */
#define ES_MONITOR_REC_WORDS 5
#define ES_XC_SEG 1216   /* lags per segment of the correlation kernel (64 lanes x 19): a monitor's window grid */
int es_bpf_stream_batch(es_ctx* ctx, const void* x_dev, int dtype, int64_t R, int64_t n_stride, const int64_t* sid_dev, const int64_t* len_dev,
                        const int64_t* col_dev, const int64_t* move_dev, const int64_t* base_dev, const int64_t* rec_host, int64_t S, int H,
                        const uint8_t* band_dev, double* z_dev, int64_t* pos_dev, double* y_hist_dev, double* corr_hist_dev, void* stream);

/* The lags the same records complete, enqueued behind es_bpf_stream_batch: continues rtwm/detector.py:76-79 (corr = correlate(y, tpl,
 * 'valid') / (sqrt(conv(y^2, 1)) + 1e-12)).  Columns [max(0, col - 62), col + len - 62) of each record's four rows of corr_hist are
 * written, computed as es_xcorr_batch computes them on the row's own 1216-lag segment grid, from the first lag of the segment that holds
 * the first new one (lags written again keep their values): corr_hist equals es_xcorr_batch over the whole stream's y at every lag held.
 * A chunk that completes no lag does no work.  Arguments and refusals as above. */
int es_xcorr_stream_batch(es_ctx* ctx, const double* y_hist_dev, int64_t R, int64_t n_stride, const int64_t* sid_dev, const int64_t* len_dev,
                          const int64_t* col_dev, const int64_t* rec_host, int64_t S, int H, const uint8_t* band_dev, double* corr_hist_dev,
                          void* stream);

/* es_pick_batch on windows read in place: continues rtwm/detector.py:83-99 (threshold, NMS +-607, top-5 fallback).  Record i is the
 * nlag_dev[i] lags from column col_dev[i] of row row_dev[i] (int32 [B]; row_dev NULL = i) of corr_dev [n_rows][stride]; thr, the whole
 * peaks row (window-relative) and npeaks with its bit-30 flag are those of es_pick_batch on that slice, bit for bit (the ragged pick's
 * kernel: same saturation proof, order statistics, NMS and fallback).  nlag < 1: npeaks 0, thr 0.0 and a peaks row of -1, as
 * es_sync_ragged_batch gives a record shorter than the template.  For a monitor the window after a push is [w0, n) with
 * w0 = 1216 * ceil(max(0, n - W) / 1216): col = w0 - base, nlag = n - w0 - 62.  The three arrays are device data: col is clamped to
 * [0, stride], nlag to stride - col, a row outside [0, n_rows) is a window without a lag.  Needs no tables beyond es_set_tables having
 * been called, only enqueues. */
int es_pick_at_batch(es_ctx* ctx, const double* corr_dev, int64_t n_rows, int stride, int64_t B, const int32_t* row_dev, const int32_t* col_dev,
                     const int32_t* nlag_dev, double* thr_dev, int32_t* peaks_dev, int32_t* npeaks_dev, void* stream);

/* ---- the verdict memo of live identification: which (key, row, position, counter) candidates are already known to fail ----------
 * A candidate's verdict (the four list decodes of rtwm/detector.py:161-190 and their validation) depends on the key, the band row, the
 * 1215 band-passed samples at an absolute position and the counter alone, and a monitor's band-passed history is bit-identical from
 * push to push: a candidate that failed once fails for as long as its stream lives.  The memo remembers such candidates, exactly.
 *
 * table_dev [slots][2] uint64, 16-byte aligned, slots a power of two; an entry is the record (k0, k1) itself, ES_MEMO_EMPTY in both
 * words when empty.  The caller packs the records (echoseal_amd/memo.py pack):
 *     k0 = key index (bits 0..19) | history row 4 s + j (bits 20..43) | epoch of stream slot s (bits 44..59); bits 60..63 zero
 *     k1 = absolute start w0 + peak (bits 0..47) | counter (bits 48..63)
 * so no record equals the empty entry.  Record (k0, k1) lives at
 *     slot = mix(k0 * 0x9E3779B97F4A7C15 + k1) & (slots - 1),   mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *                                                                        z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31
 * (the splitmix64 finaliser, arithmetic mod 2^64) or nowhere: direct-mapped, no probe sequence.  A miss only costs a decode.
 *
 * es_memo_probe_batch: hit_dev[i] = (table[slot_i] == (k0_dev[i], k1_dev[i])), both words; reads only.
 * es_memo_insert_batch: among the records of the call that map to one slot, the one with the lowest index replaces whatever the slot
 * held and the others are dropped; a record whose k0 is ES_MEMO_EMPTY is ignored (how a caller masks records out).  The table after
 * the call is a function of the table before it and the records.  Two kernels, no wait of any kind: an atomic min of the record
 * index on claim_dev [slots] uint32, which must rest at 0xFFFFFFFF, then the record whose index the claim word holds writes both
 * words and puts 0xFFFFFFFF back.  claim_dev is all 0xFFFFFFFF again when the call has run.
 * ES_EINVAL, before anything is enqueued and with nothing written: slots < 1 or not a power of two, n < 0 or n >= 2^32 - 1, a null
 * pointer with n > 0.  n == 0 enqueues nothing.  Both need no tables and only enqueue (capturable). */
#define ES_MEMO_EMPTY 0xFFFFFFFFFFFFFFFFull
int es_memo_probe_batch(es_ctx* ctx, const uint64_t* table_dev, int64_t slots, const uint64_t* k0_dev, const uint64_t* k1_dev, int64_t n,
                        uint8_t* hit_dev, void* stream);
int es_memo_insert_batch(es_ctx* ctx, uint64_t* table_dev, uint32_t* claim_dev, int64_t slots, const uint64_t* k0_dev, const uint64_t* k1_dev,
                         int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ECHOSEAL_HIP_H */
