// es_scl_wide.hip -- successive-cancellation LIST decoder with ONE LANE PER PATH: lists of 64 to 1024 paths (one frame
// per block of L lanes; the detector's default list size is 256, rtwm/detector.py:27 -- this kernel is what lets
// WatermarkDetector(key).verify(...) run unchanged), and shorter lists as 64/L whole frames per one-wave block -- the
// throughput mapping of large launches.  Same arithmetic and the same bookkeeping idea as es_scl.hip (per-depth slot
// pointers instead of path copies, trace-back instead of per-path bit arrays, Python's stable sort order).
//
// Where things live (lane p owns path p and slot p of every slot-indexed store):
//   * LLR tree depths 1..DL-1 (512..16 values per path): a scratch slab laid out [element][slot] (no cache holds it), so the lanes of a
//     wave touch one contiguous row; a lane walks a node's elements serially.  DL = 7 in one-wave blocks, 8 in blocks of several waves.
//     The g half of depth 1 (bits 512..) is never stored: llr[e + 512] +- llr[e], formed on the fly where it is consumed (float32 channel LLRs).
//   * depths DL..9 (8 + 4 + 2 values at DL = 7): LDS, [element][slot]; depth 10 (the leaf LLR): a register.
//   * slot pointers (which slot holds my data at depth d): one byte per depth packed in two 64-bit registers (16 bits above 256 paths),
//     partial-sum blocks of 1..16 bits in one 32-bit register (as in es_scl.hip), of 32 and 64 bits in LDS by
//     slot, of 128 / 256 / 512 bits (read a few times per frame) in the slab.
//   * a sort moves registers only.  One-wave blocks: the survivor of rank r -- lane r -- fetches sorted element r and its parent's
//     (pointers, small partial sums, trace-back window, softplus pair of the even sibling) straight from the registers of the lanes that
//     hold them (ds_bpermute).  Blocks of several waves publish them to LDS and read the parent's after the sort's barriers.
//   * trace-back by windows of 32 information bits (as in es_scl_multi.hip): a path carries the bits of the
//     current window and the path it descended from at the window's start; a full window goes to the slab once.
//
// The sort is a bitonic network over the 2L candidates on (metric, candidate index) -- a strict total order, so
// the result is Python's stable list.sort -- with two candidates per lane IN REGISTERS: partner lanes exchange
// through DPP / ds_swizzle / ds_bpermute, only the stages whose partner sits in another wave (3 of 45 at L = 256)
// go through LDS and a workgroup barrier.  Lists that fit one wave run the network's all-ascending form (wide_sort): its masks are constants and
// the first stage of a merge phase meets the mirrored lane, a DPP operand up to groups of 16 lanes.
//
// Barriers.  A path may read a slot that another wave wrote, but only one it inherited at a sort (whose barriers
// order the write before the read); and a lane only ever writes its OWN slot.  What remains is write-after-read:
// before a step that writes shared slots, every wave must have finished the reads of earlier steps -- one barrier,
// and only when no sort has happened since those reads (`dirty`).  A depth-by-depth barrier is not needed: within a
// step a path reads what it has itself just written.
//
// SHORT lists (LF = 1..64 paths per frame): the block is one wave that carries 64/LF whole frames (8 at LF = 8); the sort network
// stops at the frame's 2 LF candidates and every "barrier" is a wave fence.  All 64 lanes are busy at every tree depth, which the
// lanes-share-a-path kernels (es_scl.hip, es_scl_multi.hip) cannot offer at the bottom of the tree: 126 k instead of 184 k / 224 k
// vector instructions per frame at L = 8.  The price is latency: a wave carries its frames through the whole decode (~7 ms), so
// es_scl_batch picks this mapping for large launches only (or es_set_option "scl_lanes" = 1: the grouped pipeline).
//
// Blocks are not persistent: a block decodes its frames and leaves; its slab slot comes from a bitmap (as in es_scl_multi.hip).
//
// Values are bit-identical to the reference list decoder for the same reason as in es_scl.hip (es_math.h).
// This file's kernels use dynamic LDS only, with the exp table first in it: the table sits at LDS address 0 (checked at kernel start),
// which lets es_math.h address its entries without adding a base.
//
// Lists of 257..1024 paths (capacities 512 and 1024: 8 and 16 waves per block) are instantiated in a translation unit of their own,
// es_scl_wide_large.hip, which includes this file with ES_WIDE_LARGE_TU = 1: the compiler's inlining choices for the helpers every
// instantiation calls depend on how many instantiations a unit holds, and the tuned ones of lists up to 256 stay as they are.
#define ES_EXP_TAB_LDS_ADDR 0u
#ifndef ES_WIDE_LARGE_TU
#define ES_WIDE_LARGE_TU 0
#endif
#include "es_scl_common.h"
#include "es_softplus_dev.h"
#include <type_traits>

namespace {

constexpr int WIDE_GBATCH = 8;                    // load pairs in flight in the lane-serial g loops (divides 8; 8: +1 % over 4, measured)
constexpr int WIDE_WPS = 3;                       // waves per SIMD the kernel is compiled for (168 VGPRs at 3)

struct WideArgs {
    const void* llr; int is_f64; long long B;
    es_frozen_mask frozen;
    const uint16_t* data_pos;
    const uint64_t* exp_tab;
    double* alpha;            // [slots][1024][L]   (elements 8..1023 used: depth d at [1024 >> d, 2 * (1024 >> d)))
    unsigned char* aux;       // [slots][ES_WIDE_AUX_PER_PATH * L]: trace-back windows, wide partial-sum blocks, fold scratch
    uint8_t* hard_info; uint8_t* hard_ok;
    uint8_t* cand_info; double* cand_metric; uint8_t* cand_ok; int32_t* ncand;
    int skip_if_hard_ok;
    int lsz;                                  // the caller's list size (<= L)
    unsigned* slot_bits; int n_slots, slot_words;   // bitmap of slab slots (one per resident block), as in es_scl_multi.hip
    int* cursor;                              // null: block g decodes frames [g * FRG, (g + 1) * FRG).  Else (skip_if_hard_ok) blocks draw frames from this counter
                                              //   (zeroed before the launch) until they hold FRG that failed the hard decision: settled frames never ride along
    int n_info, info_bytes;                   // GK instantiations: data bits K (information + CRC) and bytes of a packed information row, ceil((K - 8) / 8)
    int prio;                                 // wave priority 0..3 (es_set_option "scl_prio"): a later launch of a burst may overtake an earlier one
};

constexpr int MWIN_W = KINFO / 32;            // trace-back windows of the default code (448 data bits)
constexpr int MWIN_MAX = N / 32;              // ... of any code (GK instantiations: K data bits, 16 <= K <= 1024, K % 8 == 0)
// aux slab per path: windows 32 x (4 + 2) B (14 used by the default code), partial-sum blocks of 128 / 256 / 512 bits 28 x 4 B, fold scratch 16 x 4 B
constexpr int WIDE_AUX_PER_PATH = MWIN_MAX * 6 + 28 * 4 + 16 * 4;

// LLR-tree depths DL..9 live in LDS, [element][slot]: depth d at rows [wide_low_row(DL, d), +1024 >> d).  A block that is one wave keeps depth 7
// there too (DL = 7: a step whose top is depth 7 or below then touches the slab only to READ depth 6, and the values that are written and
// read back within a few hundred cycles never leave the CU); blocks of several waves hold a frame of 128 / 256 paths and have no LDS to spare.
// (one-wave blocks: 7 = 8 + 4 + 2 rows of doubles by slot; 8 was round 3's layout; 6 needs two waves per SIMD)
constexpr int wide_dl(bool one_wave) { return one_wave ? 7 : 8; }
constexpr int wide_low_row(int DL, int d) { int r = 0; for (int k = DL; k < d; ++k) r += N >> k; return r; }

// Slot pointers of a path (which slot holds its data at a depth): one byte per depth in a 64-bit word while slots fit a byte (L <= 256),
// else 16 bits per depth over two words (entries 0..3 in `lo`, 4..7 in `hi`).  The partial-sum word also carries the depth-9 LLR pointer
// (entry 5) and, while published, the window ancestor (bits 48.. of the one word / entry 6 of the pair).
struct WidePtr16 { uint64_t lo, hi; };
template <int L> using wide_ptr_t = std::conditional_t<(L > 256), WidePtr16, uint64_t>;

// (bytes of the proper 32-bit half: the half is selected first and the shifts are 32-bit -- a 64-bit shift by a run-time count, which the depth
// is in the slab loop and the partial-sum fold, issues at the float64 rate.  The depth is wave-uniform: the masks are scalar.  With a
// compile-time depth this folds to one byte extract / insert.)
__device__ __forceinline__ uint64_t p8_set(uint64_t w, int k, int v)
{
    const int sh = 8 * (k & 3);
    const uint32_t m = 255u << sh, x = (uint32_t)v << sh, mlo = k < 4 ? m : 0u, mhi = k < 4 ? 0u : m;
    const uint32_t lo = ((uint32_t)w & ~mlo) | (x & mlo), hi = ((uint32_t)(w >> 32) & ~mhi) | (x & mhi);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int p8_get(uint64_t w, int k) { return (int)(((k < 4 ? (uint32_t)w : (uint32_t)(w >> 32)) >> (8 * (k & 3))) & 255u); }
__device__ __forceinline__ WidePtr16 p8_set(WidePtr16 w, int k, int v)
{
    const int sh = 16 * (k & 3);
    const uint64_t m = ~(0xFFFFULL << sh), x = (uint64_t)(uint32_t)v << sh;
    if (k < 4) w.lo = (w.lo & m) | x; else w.hi = (w.hi & m) | x;
    return w;
}
__device__ __forceinline__ int p8_get(WidePtr16 w, int k) { return (int)(((k < 4 ? w.lo : w.hi) >> (16 * (k & 3))) & 0xFFFFULL); }
// (L > 256) a path's pointers at slot s: the LLR tree's (depths 1..8, `a`) and the partial sums' (depths 1..5, depth-9 LLR pointer, `b`)
__device__ __forceinline__ WidePtr16 wide_ptr_fill_a(int s) { const uint64_t r = (uint64_t)(uint32_t)s * 0x0001000100010001ULL; return WidePtr16{r, r}; }
__device__ __forceinline__ WidePtr16 wide_ptr_fill_b(int s) { const uint64_t r = (uint64_t)(uint32_t)s * 0x0001000100010001ULL; return WidePtr16{r, r & 0xFFFFFFFFULL}; }
// ... the partial-sum pointers with the window ancestor beside them (entry 6: published through a sort), and back
__device__ __forceinline__ WidePtr16 wide_ptr_join(WidePtr16 b, uint32_t anc) { b.hi |= (uint64_t)anc << 32; return b; }
__device__ __forceinline__ void wide_ptr_split(WidePtr16 t, WidePtr16& b, uint32_t& anc) { anc = (uint32_t)(t.hi >> 32) & 0xFFFFu; t.hi &= 0xFFFFFFFFULL; b = t; }

// What follows a path through a sort.  Several waves per frame: every path publishes it to LDS and the survivor of rank r reads its
// parent's -- double-buffered by information index (NBUF = 2: a wave may still be reading while another is a sort further) up to 512
// paths; at 1024 paths two buffers do not fit beside the rest (LDS), so ONE buffer with a barrier before every write to it.  ONE wave
// per block: nothing is stored -- the survivor fetches its parent's registers with ds_bpermute (the lanes of a wave run in lock step).
template <int L, int NBUF>
struct WidePub {
    double   skey[NBUF][2 * L];         // cross-wave sort stages and the read-out
    double   xsp[NBUF][2][L];           // softplus pair of the even sibling,
    wide_ptr_t<L> xpa[NBUF][L];         // ... LLR-tree slot pointers,
    wide_ptr_t<L> xpb[NBUF][L];         // ... partial-sum slot pointers, depth-9 pointer and window ancestor (wide_ptr_join),
    uint32_t xb0[NBUF][L];              // ... partial sums of 1..16 bits,
    uint32_t xhist[NBUF][L];            // ... bits of the current trace-back window
    uint16_t sidx[NBUF][2 * L];
};
struct WidePubBperm { };
// buffers of the published state: NB = 1 one wave per block, 2 several
constexpr int wide_pub_bufs(int L, int NB) { return (NB == 2 && L > 512) ? 1 : NB; }
template <int L, int NB>
using wide_pub_t = std::conditional_t<NB == 1, WidePubBperm, WidePub<L, wide_pub_bufs(L, NB)>>;

template <int L, int NB>
struct WideLds {
    static constexpr int DL = wide_dl(NB == 1);
    static constexpr int NLOW = wide_low_row(DL, 10);
    uint64_t exp_tab[ES_EXP_TAB_WORDS];
    double   low[NLOW][L];              // depths DL..9, by slot (also: the hard decision's 184 bytes and the final ordering's metrics, outside the list loop)
    uint32_t betaM[3][L];               // partial-sum blocks of 32 (row 0) and 64 bits (1, 2), by slot (wider ones, touched a few times per frame: slab)
    int      flag;
    wide_pub_t<L, NB> pub;              // (the frames drawn from the cursor, up to 64 ints per one-wave block, borrow row 1 of `low` before the list loop starts)
};

// lane l <-> lane l ^ D inside a wave, D a constant after unrolling
__device__ __forceinline__ int wxor_b32(int v, int D)
{
    switch (D) {
        case 1:  return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, true);     // quad_perm [1,0,3,2]
        case 2:  return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, true);     // quad_perm [2,3,0,1]
        case 4:  return __builtin_amdgcn_ds_swizzle(v, 0x101F);                // bit mode: xor 4
        case 8:  return __builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, true);    // row_ror:8
        case 16: return __builtin_amdgcn_ds_swizzle(v, 0x401F);                // bit mode: xor 16
        default: return __shfl_xor(v, 32);
    }
}

// Compare-exchange steps of the sort network, written out: path metrics are sums of non-negative penalties (or +inf for a dead
// lane), so their bit patterns order like their values and (metric, index) compares as the 96-bit unsigned number hi:lo:index --
// ONE borrow chain of three subtractions leaves "mine sorts before the partner's" in VCC, and with the partner in a lane that DPP
// reaches the partner's words are an operand modifier of the subtractions and of the three selects: 6 vector instructions per
// element and stage where the compiler's rendering of the plain C++ compare (ka < kb || (ka == kb && ia < ib)) + selects takes 10.  With the DPP modifier the subtraction is
// partner - mine (the modified operand is the minuend; tools/ub/ub_dppvcc.hip), so VCC = "the partner sorts before mine" and keeping
// mine is VCC xor take_min (equal elements are two dead lanes' identical fillers: either may be kept).  (s_nop 1: a DPP operand must
// not have been written by the two preceding vector instructions; the compiler cannot see into the block.)  tools/ub/ub_sortce.hip
// checks every step form against plain C++.  The scalar xor / xnor of the mask also writes SCC: it is in the clobber list ("scc") -- without
// it the compiler kept a scalar compare's result live across a step (round 4: `info_idx % 32 == 0` evaluated before the sort and selected
// on after it came out wrong in the 64-path instantiation, whose scheduling happened to put the compare there).
#define ES_CE_DPP(CTRL, lo, hi, ix, tmask)                                                                                   \
    do { uint32_t t_;                                                                                                        \
        asm volatile("s_nop 1\n\t"                                                                                           \
                     "v_sub_co_u32_dpp %3, vcc, %2, %2 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                              \
                     "v_subb_co_u32_dpp %3, vcc, %0, %0, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                     "v_subb_co_u32_dpp %3, vcc, %1, %1, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                        \
                     "s_xor_b64 vcc, vcc, %4\n\t"                                                                            \
                     "v_cndmask_b32_dpp %2, %2, %2, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                             \
                     "v_cndmask_b32_dpp %0, %0, %0, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                             \
                     "v_cndmask_b32_dpp %1, %1, %1, vcc " CTRL " row_mask:0xf bank_mask:0xf"                                 \
                     : "+v"(lo), "+v"(hi), "+v"(ix), "=&v"(t_) : "s"(tmask) : "vcc", "scc");                                 \
    } while (0)
// the partner's words already fetched (ds_swizzle / ds_bpermute / LDS): keep mine where (mine < other) == take_min
__device__ __forceinline__ void ce_pair(uint32_t& lo, uint32_t& hi, uint32_t& ix, uint32_t olo, uint32_t ohi, uint32_t oix, unsigned long long tmask)
{
    uint32_t t_;
    asm volatile("v_sub_co_u32 %3, vcc, %2, %6\n\t"
                 "v_subb_co_u32 %3, vcc, %0, %4, vcc\n\t"
                 "v_subb_co_u32 %3, vcc, %1, %5, vcc\n\t"
                 "s_xnor_b64 vcc, vcc, %7\n\t"
                 "v_cndmask_b32 %2, %6, %2, vcc\n\t"
                 "v_cndmask_b32 %0, %4, %0, vcc\n\t"
                 "v_cndmask_b32 %1, %5, %1, vcc"
                 : "+v"(lo), "+v"(hi), "+v"(ix), "=&v"(t_) : "v"(olo), "v"(ohi), "v"(oix), "s"(tmask) : "vcc", "scc");
}
// a lane's own two elements: swap where (element 1 < element 0) == ascending
__device__ __forceinline__ void ce_inlane(uint32_t& lo0, uint32_t& hi0, uint32_t& ix0, uint32_t& lo1, uint32_t& hi1, uint32_t& ix1, unsigned long long amask)
{
    uint32_t t_, nlo0, nhi0, nix0;
    asm volatile("v_sub_co_u32 %3, vcc, %9, %6\n\t"
                 "v_subb_co_u32 %3, vcc, %7, %4, vcc\n\t"
                 "v_subb_co_u32 %3, vcc, %8, %5, vcc\n\t"
                 "s_xnor_b64 vcc, vcc, %10\n\t"
                 "v_cndmask_b32 %0, %4, %7, vcc\n\t"
                 "v_cndmask_b32 %1, %5, %8, vcc\n\t"
                 "v_cndmask_b32 %2, %6, %9, vcc\n\t"
                 "v_cndmask_b32 %7, %7, %4, vcc\n\t"
                 "v_cndmask_b32 %8, %8, %5, vcc\n\t"
                 "v_cndmask_b32 %9, %9, %6, vcc"
                 : "=&v"(nlo0), "=&v"(nhi0), "=&v"(nix0), "=&v"(t_), "+v"(lo0), "+v"(hi0), "+v"(ix0), "+v"(lo1), "+v"(hi1), "+v"(ix1)
                 : "s"(amask) : "vcc", "scc");
    lo0 = nlo0; hi0 = nhi0; ix0 = nix0;
}

// The first stage of a merge phase in the all-ascending network of lists up to 64 paths: element e meets e ^ (k - 1), which is the OTHER
// element of the mirrored lane -- a DPP operand for groups of 2, 4, 8 and 16 lanes (quad_perm:[1,0,3,2], quad_perm:[3,2,1,0],
// row_half_mirror, row_mirror).  Both of a lane's elements are the smaller (or both the larger) ones of their pairs: tmask = lanes that take
// the minima.  As ES_CE_DPP, twice, the lane's own two elements in swapped roles: mine 0 against the partner's 1, mine 1 against the
// partner's 0; the results go to fresh registers (the second compare reads what the first one would have overwritten).
#define ES_CE_DPP_X(CTRL, lo0, hi0, ix0, lo1, hi1, ix1, tmask)                                                               \
    do { uint32_t t_, a_, b_, c_, d_, e_, f_;                                                                                \
        asm volatile("s_nop 1\n\t"                                                                                           \
                     "v_sub_co_u32_dpp %6, vcc, %12, %9 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                             \
                     "v_subb_co_u32_dpp %6, vcc, %10, %7, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                       \
                     "v_subb_co_u32_dpp %6, vcc, %11, %8, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                       \
                     "s_xor_b64 vcc, vcc, %13\n\t"                                                                           \
                     "v_cndmask_b32_dpp %2, %12, %9, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                            \
                     "v_cndmask_b32_dpp %0, %10, %7, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                            \
                     "v_cndmask_b32_dpp %1, %11, %8, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                            \
                     "v_sub_co_u32_dpp %6, vcc, %9, %12 " CTRL " row_mask:0xf bank_mask:0xf\n\t"                             \
                     "v_subb_co_u32_dpp %6, vcc, %7, %10, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                       \
                     "v_subb_co_u32_dpp %6, vcc, %8, %11, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                       \
                     "s_xor_b64 vcc, vcc, %13\n\t"                                                                           \
                     "v_cndmask_b32_dpp %5, %9, %12, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                            \
                     "v_cndmask_b32_dpp %3, %7, %10, vcc " CTRL " row_mask:0xf bank_mask:0xf\n\t"                            \
                     "v_cndmask_b32_dpp %4, %8, %11, vcc " CTRL " row_mask:0xf bank_mask:0xf"                                 \
                     : "=&v"(a_), "=&v"(b_), "=&v"(c_), "=&v"(d_), "=&v"(e_), "=&v"(f_), "=&v"(t_)                           \
                     : "v"(lo0), "v"(hi0), "v"(ix0), "v"(lo1), "v"(hi1), "v"(ix1), "s"(tmask) : "vcc", "scc");               \
        lo0 = a_; hi0 = b_; ix0 = c_; lo1 = d_; hi1 = e_; ix1 = f_;                                                          \
    } while (0)
// Lanes of a wave whose index has bit d clear (d a power of two below 64, a constant after unrolling; 0: every lane), as a mask formed
// WHERE IT IS USED: handed plain constants the compiler hoists the masks out of the bit loop into scalar registers, of which the kernel
// has none to spare -- they came back through v_readlane / v_writelane, two vector instructions per stage.  A scalar move is free.
#define ES_WIDE_MASK32(C) ([]() { uint32_t h_; asm volatile("s_mov_b32 %0, " #C : "=s"(h_)); return h_; }())
__device__ __forceinline__ unsigned long long wide_lanes_clear(int d)
{
    uint32_t lo, hi;
    switch (d) {
        case 0:  lo = hi = ES_WIDE_MASK32(0xFFFFFFFF); break;
        case 1:  lo = hi = ES_WIDE_MASK32(0x55555555); break;
        case 2:  lo = hi = ES_WIDE_MASK32(0x33333333); break;
        case 4:  lo = hi = ES_WIDE_MASK32(0x0F0F0F0F); break;
        case 8:  lo = hi = ES_WIDE_MASK32(0x00FF00FF); break;
        case 16: lo = hi = ES_WIDE_MASK32(0x0000FFFF); break;
        default: lo = ES_WIDE_MASK32(0xFFFFFFFF); hi = ES_WIDE_MASK32(0); break;
    }
    return ((unsigned long long)hi << 32) | lo;
}
// lane l <-> lane l ^ 31 / l ^ 63 (the mirrored lane of a group of 32 / 64)
__device__ __forceinline__ int wmirror_b32(int v, int D) { return D == 31 ? __builtin_amdgcn_ds_swizzle(v, 0x7C1F) : __shfl_xor(v, 63); }

// Bitonic network over 2L (key, index) pairs, element e = 2 * lane + b held as (k0, i0) / (k1, i1); ascending on exit.
// Lists of up to 64 paths (one wave) run its all-ascending form: a merge phase of k elements starts by meeting element e with e ^ (k - 1)
// -- the two runs it merges both ascend -- and goes on with the half-cleaners e ^ j, j = k / 4 .. 1.  Every stage's "take the minimum" mask
// is then a constant of the lane index (no compare, no ballot), and the first stage's partner, the mirrored lane, is a DPP operand where
// the stage at the same distance of the alternating form (lane ^ 4, lane ^ 16) fetched three words per element through ds_swizzle.
// Both are sorting networks and (metric, index) is a strict total order (dead lanes' fillers are identical): the result is the same.
// (LF < L: independent networks over aligned groups of LF lanes -- one per frame; pl = lane index within the frame)
template <int L, int LF>
__device__ __forceinline__ void wide_sort(double& k0, uint32_t& i0, double& k1, uint32_t& i1, const int p, const int pl, WideLds<L, (LF > 64 ? 2 : 1)>& W, int& buf)
{
    constexpr int NBUF = wide_pub_bufs(L, LF > 64 ? 2 : 1);     // 1: one buffer, a barrier before each write to it (see WidePub)
    uint64_t u0, u1; __builtin_memcpy(&u0, &k0, 8); __builtin_memcpy(&u1, &k1, 8);
    uint32_t lo0 = (uint32_t)u0, hi0 = (uint32_t)(u0 >> 32), lo1 = (uint32_t)u1, hi1 = (uint32_t)(u1 >> 32);
    if constexpr (LF <= 64) {
    #pragma unroll
    for (int k = 2; k <= 2 * LF; k <<= 1) {
        if (k > 2) {                                             // element e <-> e ^ (k - 1): lane p ^ dm, the other element
            const int dm = (k >> 1) - 1;
            const unsigned long long tm = wide_lanes_clear(k >> 2);
            if (dm == 1) ES_CE_DPP_X("quad_perm:[1,0,3,2]", lo0, hi0, i0, lo1, hi1, i1, tm);
            else if (dm == 3) ES_CE_DPP_X("quad_perm:[3,2,1,0]", lo0, hi0, i0, lo1, hi1, i1, tm);
            else if (dm == 7) ES_CE_DPP_X("row_half_mirror", lo0, hi0, i0, lo1, hi1, i1, tm);
            else if (dm == 15) ES_CE_DPP_X("row_mirror", lo0, hi0, i0, lo1, hi1, i1, tm);
            else {
                const uint32_t a0 = (uint32_t)wmirror_b32((int)lo1, dm), b0 = (uint32_t)wmirror_b32((int)hi1, dm), c0 = (uint32_t)wmirror_b32((int)i1, dm);
                const uint32_t a1 = (uint32_t)wmirror_b32((int)lo0, dm), b1 = (uint32_t)wmirror_b32((int)hi0, dm), c1 = (uint32_t)wmirror_b32((int)i0, dm);
                ce_pair(lo0, hi0, i0, a0, b0, c0, tm);
                ce_pair(lo1, hi1, i1, a1, b1, c1, tm);
            }
        }
        #pragma unroll
        for (int j = (k == 2) ? 1 : (k >> 2); j >= 1; j >>= 1) {
            if (j == 1) ce_inlane(lo0, hi0, i0, lo1, hi1, i1, wide_lanes_clear(0));
            else {
                const int dl = j >> 1;                           // partner lane p ^ dl, same b
                const unsigned long long tm = wide_lanes_clear(dl);
                if (dl == 1) { ES_CE_DPP("quad_perm:[1,0,3,2]", lo0, hi0, i0, tm); ES_CE_DPP("quad_perm:[1,0,3,2]", lo1, hi1, i1, tm); }
                else if (dl == 2) { ES_CE_DPP("quad_perm:[2,3,0,1]", lo0, hi0, i0, tm); ES_CE_DPP("quad_perm:[2,3,0,1]", lo1, hi1, i1, tm); }
                else if (dl == 8) { ES_CE_DPP("row_ror:8", lo0, hi0, i0, tm); ES_CE_DPP("row_ror:8", lo1, hi1, i1, tm); }
                else {
                    const uint32_t a0 = (uint32_t)wxor_b32((int)lo0, dl), b0 = (uint32_t)wxor_b32((int)hi0, dl), c0 = (uint32_t)wxor_b32((int)i0, dl);
                    const uint32_t a1 = (uint32_t)wxor_b32((int)lo1, dl), b1 = (uint32_t)wxor_b32((int)hi1, dl), c1 = (uint32_t)wxor_b32((int)i1, dl);
                    ce_pair(lo0, hi0, i0, a0, b0, c0, tm);
                    ce_pair(lo1, hi1, i1, a1, b1, c1, tm);
                }
            }
        }
    }
    } else {
    #pragma unroll
    for (int k = 2; k <= 2 * LF; k <<= 1) {
        const bool asc = ((2 * pl) & k) == 0;                    // k == 2 LF: always ascending
        #pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            if (j == 1) {                                        // partner = the lane's other element
                ce_inlane(lo0, hi0, i0, lo1, hi1, i1, __builtin_amdgcn_ballot_w64(asc));
            } else {
                const int dl = j >> 1;                           // partner lane p ^ dl, same b
                const unsigned long long tm = __builtin_amdgcn_ballot_w64(((pl & dl) == 0) == asc);     // take the smaller of the pair
                if (dl == 1) { ES_CE_DPP("quad_perm:[1,0,3,2]", lo0, hi0, i0, tm); ES_CE_DPP("quad_perm:[1,0,3,2]", lo1, hi1, i1, tm); }
                else if (dl == 2) { ES_CE_DPP("quad_perm:[2,3,0,1]", lo0, hi0, i0, tm); ES_CE_DPP("quad_perm:[2,3,0,1]", lo1, hi1, i1, tm); }
                else if (dl == 8) { ES_CE_DPP("row_ror:8", lo0, hi0, i0, tm); ES_CE_DPP("row_ror:8", lo1, hi1, i1, tm); }
                else {
                    uint32_t a0 = 0, b0 = 0, c0 = 0, a1 = 0, b1 = 0, c1 = 0;
                    bool cross = false;
                    if constexpr (LF > 64) {
                        if (dl >= 64) {
                            cross = true;
                            if constexpr (NBUF == 1) __syncthreads();
                            W.pub.skey[buf][2 * p] = __builtin_bit_cast(double, ((uint64_t)hi0 << 32) | lo0);
                            W.pub.skey[buf][2 * p + 1] = __builtin_bit_cast(double, ((uint64_t)hi1 << 32) | lo1);
                            W.pub.sidx[buf][2 * p] = (uint16_t)i0; W.pub.sidx[buf][2 * p + 1] = (uint16_t)i1;
                            __syncthreads();
                            const int o = p ^ dl;
                            const uint64_t x0 = __builtin_bit_cast(uint64_t, W.pub.skey[buf][2 * o]), x1 = __builtin_bit_cast(uint64_t, W.pub.skey[buf][2 * o + 1]);
                            a0 = (uint32_t)x0; b0 = (uint32_t)(x0 >> 32); a1 = (uint32_t)x1; b1 = (uint32_t)(x1 >> 32);
                            c0 = W.pub.sidx[buf][2 * o]; c1 = W.pub.sidx[buf][2 * o + 1];
                            if constexpr (NBUF == 2) buf ^= 1;
                        }
                    }
                    if (!cross) {
                        a0 = (uint32_t)wxor_b32((int)lo0, dl); b0 = (uint32_t)wxor_b32((int)hi0, dl); c0 = (uint32_t)wxor_b32((int)i0, dl);
                        a1 = (uint32_t)wxor_b32((int)lo1, dl); b1 = (uint32_t)wxor_b32((int)hi1, dl); c1 = (uint32_t)wxor_b32((int)i1, dl);
                    }
                    ce_pair(lo0, hi0, i0, a0, b0, c0, tm);
                    ce_pair(lo1, hi1, i1, a1, b1, c1, tm);
                }
            }
        }
    }
    }
    u0 = ((uint64_t)hi0 << 32) | lo0; u1 = ((uint64_t)hi1 << 32) | lo1;
    __builtin_memcpy(&k0, &u0, 8); __builtin_memcpy(&k1, &u1, 8);
}

// v, as a value formed where this is called.  The loops that zero a settled frame's candidate rows start at it: handed the lane index itself
// the compiler strides them by eight, hoists the eight start offsets lane + 64 k out of the frame loop and carries them -- in registers or
// spilled -- through the whole list loop.
__device__ __forceinline__ int wide_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// hard decision -> butterfly -> data bits -> CRC of one frame by one wave (fastpolar.py:260-268); returns the CRC verdict to every lane
template <bool GK>
__device__ __forceinline__ int hard_decision_wave(const WideArgs& a, long long ff, int lane, uint32_t* hardw, uint8_t* hbytes, const uint16_t* dpos)
{
    const float* l32 = (const float*)a.llr + ff * N;
    const double* l64 = (const double*)a.llr + ff * N;
    uint32_t word = 0;
    for (int c = 0; c < 16; ++c) {
        const double v = a.is_f64 ? l64[64 * c + lane] : (double)l32[64 * c + lane];
        const unsigned long long m = __ballot(v > 0.0);
        if (((lane & 31) >> 1) == c) word = (lane & 1) ? (uint32_t)(m >> 32) : (uint32_t)m;
    }
    word ^= (word >> 1) & 0x55555555u;
    word ^= (word >> 2) & 0x33333333u;
    word ^= (word >> 4) & 0x0f0f0f0fu;
    word ^= (word >> 8) & 0x00ff00ffu;
    word ^= (word >> 16) & 0x0000ffffu;
    #pragma unroll
    for (int hw = 1; hw < 32; hw <<= 1) {
        const uint32_t o = __shfl_xor(word, hw);
        if (!((lane & 31) & hw)) word ^= o;
    }
    if (lane < 32) hardw[lane] = word;
    wave_fence_lds();
    int ok = 0;
    if constexpr (GK) {
        // K data bits (K - 8 information bits, then the CRC's 8), MSB first in ceil(K / 8) bytes; neither count need be a whole number of bytes
        const int K = a.n_info, nbits = K - 8, nib = a.info_bytes, rem = nbits & 7;
        for (int bi = lane; bi < ((K + 7) >> 3); bi += 64) {
            uint32_t byte = 0;
            #pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int j = 8 * bi + b;
                const int pos = dpos[j < K ? j : 0];
                if (j < K) byte |= ((hardw[pos >> 5] >> (pos & 31)) & 1u) << (7 - b);
            }
            hbytes[bi] = (uint8_t)byte;
        }
        wave_fence_lds();
        if (lane == 0) {
            uint32_t reg = crc8_bytes(hbytes, nbits >> 3);
            const uint32_t lo = hbytes[nbits >> 3], hi = (((nbits >> 3) + 1) < ((K + 7) >> 3)) ? hbytes[(nbits >> 3) + 1] : 0u;
            for (int b = 0; b < rem; ++b) {
                reg ^= ((lo >> (7 - b)) & 1u) << 7;
                reg = (reg & 0x80u) ? ((reg << 1) ^ 0x07u) & 0xffu : (reg << 1) & 0xffu;
            }
            ok = (reg == ((((lo << 8) | hi) >> (8 - rem)) & 0xffu));
        }
        ok = __shfl(ok, 0);
        for (int k = lane; k < nib; k += 64) {
            uint32_t v = hbytes[k];
            if (rem && k == nib - 1) v &= 0xffu << (8 - rem);          // the row is np.packbits(information bits): zero padding, not CRC bits
            a.hard_info[ff * nib + k] = (uint8_t)v;
        }
    } else {
        if (lane < 56) {
            uint32_t byte = 0;
            #pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int pos = dpos[8 * lane + b];
                byte |= ((hardw[pos >> 5] >> (pos & 31)) & 1u) << (7 - b);
            }
            hbytes[lane] = (uint8_t)byte;
        }
        wave_fence_lds();
        if (lane == 0) ok = (crc8_bytes(hbytes, ES_INFO_BYTES) == hbytes[ES_INFO_BYTES]);
        ok = __shfl(ok, 0);
        if (lane < ES_INFO_BYTES) a.hard_info[ff * ES_INFO_BYTES + lane] = hbytes[lane];
    }
    if (lane == 0) a.hard_ok[ff] = (uint8_t)ok;
    wave_fence_lds();
    return ok;
}

// L lanes per block, LF paths per frame.  LF > 64: one frame per block, the block is the group (barrier = __syncthreads).
// LF <= 64: every wave is a group of 64 / LF whole frames (barrier = wave fence), L / LF frames per block.
// GK: any code Polar(1024, K) + CRC-8, 9 <= K <= 1024 (the reference's PolarCode takes any K, rtwm/fastpolar.py:209-234): K, the row width
// and the number of trace-back windows are run-time values (a.n_info, a.info_bytes).  The default instantiation (K = 448, everything the
// reference itself instantiates) keeps them as compile-time constants: its code is unchanged by the existence of the other.
constexpr int wide_wps(int L) { return L == 1024 ? 4 : L == 512 ? 2 : WIDE_WPS; }     // waves per SIMD: 512 / 1024 paths -- one block per CU
template <int L, int LF, bool GK = false>
__global__ __launch_bounds__(L, wide_wps(L)) void es_scl_wide_kernel(WideArgs a)
{
    constexpr int MW = GK ? MWIN_MAX : MWIN_W;           // rows of the trace-back arrays in the aux slab
    const int NIB = GK ? a.info_bytes : ES_INFO_BYTES;   // bytes of a packed information row
    constexpr bool WAVE = (LF <= 64);                // the block is one wave
    constexpr int FRG = L / LF;                      // frames per block
    constexpr int NB = WAVE ? 1 : 2;
    constexpr int NBUF = wide_pub_bufs(L, NB);       // published-state buffers (WidePub); 1 with several waves: a barrier before each write
    static_assert(LF >= 1 && LF <= L && (L % 64) == 0 && L <= 1024 && (WAVE ? L == 64 : L == LF), "shape");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    WideLds<L, NB>& W = *reinterpret_cast<WideLds<L, NB>*>(smem_raw);
    if (a.prio == 1) __builtin_amdgcn_s_setprio(1); else if (a.prio == 2) __builtin_amdgcn_s_setprio(2); else if (a.prio >= 3) __builtin_amdgcn_s_setprio(3);
    const int p = threadIdx.x;                       // slot == lane of the block
    const int lane = p & 63, wv = p >> 6;
    const int pl = p % LF;                           // path within its frame
    const int fp0 = p - pl;                          // slot of the frame's path 0
    using WLds = WideLds<L, NB>;
    static_assert(__builtin_offsetof(WLds, exp_tab) == 0, "the exp table must be the first member (ES_EXP_TAB_LDS_ADDR)");
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_raw != ES_EXP_TAB_LDS_ADDR) __builtin_trap();   // never: no static LDS in this file
    for (int i = p; i < ES_EXP_TAB_WORDS; i += L) W.exp_tab[i] = a.exp_tab[i];
    __syncthreads();
    auto group_sync = [&]() { if constexpr (WAVE) wave_fence_global(); else __syncthreads(); };
    const uint64_t* tab = W.exp_tab;
    // ---- claim a slab slot for this block (bit per slot; LDS and registers keep resident blocks <= slots).  Blocks are not
    // persistent: a block decodes its frames and leaves, so a launch has no tail of half-empty iterations and the wave slots it
    // frees go to whatever is queued (the front end of the next batches, the next group's list decoder).
    if (p == 0) {
        int slot = -1;
        unsigned w = blockIdx.x % (unsigned)a.slot_words;
        const bool drained = a.cursor && __hip_atomic_load(a.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= a.B;   // (a launch is sized for B frames: blocks that come after the last frame was drawn leave at once)
        if (drained) slot = -2;
        for (int tries = 0; slot == -1 && tries < (1 << 22); ++tries) {
            const unsigned v = __hip_atomic_load(&a.slot_bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned valid = (w == (unsigned)a.slot_words - 1 && (a.n_slots & 31)) ? ((1u << (a.n_slots & 31)) - 1u) : 0xffffffffu;
            const unsigned freeb = ~v & valid;
            if (freeb) {
                const int bit = __ffs(freeb) - 1;
                const unsigned old = atomicOr(&a.slot_bits[w], 1u << bit);
                if (!(old & (1u << bit))) slot = (int)(w * 32u) + bit;
            } else {
                w = (w + 1u) % (unsigned)a.slot_words;
                if (tries > 64) __builtin_amdgcn_s_sleep(8);
            }
        }
        W.flag = slot;
    }
    __syncthreads();
    const int slot = W.flag;
    __syncthreads();
    if (slot == -2) return;
    if (slot < 0) {                                                    // cannot happen (see the launcher); never spin forever, never fail silently:
        constexpr int FRB = FRG;                                        // the block's frames read ncand = -1
        if (a.cursor) { if (p < FRB) { const long long ff = atomicAdd(a.cursor, 1); if (ff < a.B) a.ncand[ff] = -1; } }
        else for (long long ff = (long long)blockIdx.x * FRB + p; p < FRB && ff < a.B; ff += a.B) a.ncand[ff] = -1;
        return;
    }
    double* const A = a.alpha + (long long)slot * N * L;             // element e of slot s at A[e*L + s]
    unsigned char* const aux = a.aux + (long long)slot * WIDE_AUX_PER_PATH * L;
    uint32_t* const TBW = reinterpret_cast<uint32_t*>(aux);                          // [14][L] window bits (first = MSB)
    uint32_t* const BG = TBW + MW * L;                                           // [28][L] partial-sum blocks of 128 (rows 0..3), 256 (4..11) and 512 bits (12..27), by slot
    uint32_t* const CB = BG + 28 * L;                                                // [16][L] fold scratch, own column only
    uint16_t* const TBA = reinterpret_cast<uint16_t*>(CB + 16 * L);                  // [14][L] path (within the frame) at the window's start

    // partial-sum word `wi` (block of 32*Wd bits at words [Wd, 2Wd)) of slot s
    auto beta_ld = [&](int wi, int s) -> uint32_t { return wi < 4 ? W.betaM[wi - 1][s] : BG[(wi - 4) * L + s]; };
    auto beta_st = [&](int wi, int s, uint32_t v) { if (wi < 4) W.betaM[wi - 1][s] = v; else BG[(wi - 4) * L + s] = v; };

    constexpr int DL = WLds::DL;                                                             // first LLR-tree depth held in LDS
    auto lrow = [](int d) constexpr { return wide_low_row(WLds::DL, d); };                   // its first row in W.low
    uint32_t* const hd_words = reinterpret_cast<uint32_t*>(&W.low[0][0]);                   // 32 words ...
    uint8_t* const hd_bytes = reinterpret_cast<uint8_t*>(&W.low[0][16]);                    // ... and up to 128 bytes of the hard decision (first wave; the rows are idle outside the list loop)
    int* const drawn = reinterpret_cast<int*>(&W.low[1][0]);                                 // frames drawn from the cursor (<= 64 ints), read back before the list loop writes the rows
    const long long n_groups = a.cursor ? (long long)gridDim.x : (a.B + FRG - 1) / FRG;      // (cursor: one draw per block)
    for (long long g = blockIdx.x; g < n_groups; g += gridDim.x) {      // one group of FRG frames per block (grid = groups)
        long long f; bool f_valid;
        uint64_t active_mask = 0;                              // block-uniform: frames that go through the list loop (up to 64 of them)
        if (a.cursor) {
            // ---------------- draw frames until FRG of them fail the hard decision (fastpolar.py:260-268) or none are left
            if constexpr (WAVE) {
                int n = 0;
                while (n < FRG) {
                    int ff = 0;
                    if (lane == 0) ff = atomicAdd(a.cursor, 1);
                    ff = __shfl(ff, 0);
                    if (ff >= a.B) break;
                    const int ok = hard_decision_wave<GK>(a, ff, lane, hd_words, hd_bytes, a.data_pos);
                    if (ok) {                                  // settled: its candidate rows read as zeros
                        if (lane == 0) a.ncand[ff] = 0;
                        const int ln = wide_opaque(lane);
                        #pragma unroll 1
                        for (int k = ln; k < a.lsz * NIB; k += 64) a.cand_info[(long long)ff * a.lsz * NIB + k] = 0;
                        #pragma unroll 1
                        for (int k = ln; k < a.lsz; k += 64) { a.cand_metric[(long long)ff * a.lsz + k] = 0.0; a.cand_ok[(long long)ff * a.lsz + k] = 0; }
                    } else { if (lane == 0) drawn[n] = ff; ++n; }
                }
                wave_fence_lds();
                if (n == 0) break;
                f_valid = (lane / LF) < n;
                f = drawn[f_valid ? lane / LF : 0];             // a missing frame mirrors the first one (never stored)
                active_mask = (n >= 64) ? ~0ULL : ((1ULL << n) - 1ULL);
            } else {
                int ff;
                for (;;) {
                    if (p == 0) drawn[0] = atomicAdd(a.cursor, 1);
                    __syncthreads();
                    ff = drawn[0];
                    if (ff >= a.B) break;
                    if (wv == 0) {
                        const int ok = hard_decision_wave<GK>(a, ff, lane, hd_words, hd_bytes, a.data_pos);
                        if (lane == 0) W.flag = ok;
                    }
                    __syncthreads();
                    const int ok = W.flag;
                    __syncthreads();
                    if (!ok) break;
                    if (p == 0) a.ncand[ff] = 0;
                    for (int k = p; k < a.lsz * NIB; k += L) a.cand_info[(long long)ff * a.lsz * NIB + k] = 0;
                    if (p < a.lsz) { a.cand_metric[(long long)ff * a.lsz + p] = 0.0; a.cand_ok[(long long)ff * a.lsz + p] = 0; }
                }
                if (ff >= a.B) break;
                f = ff; f_valid = true; active_mask = 1ULL;
            }
        } else {
        const long long f_raw = g * FRG + (WAVE ? lane / LF : 0);
        f_valid = f_raw < a.B;
        f = f_valid ? f_raw : a.B - 1;          // a missing frame mirrors the last one (never stored)

        // ---------------- hard decision (fastpolar.py:260-268): frame by frame, one wave each
        if constexpr (WAVE) {
            for (int fi = 0; fi < FRG; ++fi) {
                const long long ff = g * FRG + fi;
                if (ff >= a.B) break;
                const int ok = hard_decision_wave<GK>(a, ff, lane, hd_words, hd_bytes, a.data_pos);
                if (ok && a.skip_if_hard_ok) {                 // no list for this record: its candidate rows read as zeros
                    if (lane == 0) a.ncand[ff] = 0;
                    const int ln = wide_opaque(lane);
                    #pragma unroll 1
                    for (int k = ln; k < a.lsz * NIB; k += 64) a.cand_info[ff * a.lsz * NIB + k] = 0;
                    #pragma unroll 1
                    for (int k = ln; k < a.lsz; k += 64) { a.cand_metric[ff * a.lsz + k] = 0.0; a.cand_ok[ff * a.lsz + k] = 0; }
                } else active_mask |= 1ULL << fi;
            }
        } else {
            if (wv == 0) {
                const int ok = hard_decision_wave<GK>(a, f, lane, hd_words, hd_bytes, a.data_pos);
                if (lane == 0) W.flag = ok;
            }
            __syncthreads();
            if (W.flag && a.skip_if_hard_ok) {
                if (p == 0) a.ncand[f] = 0;
                for (int k = p; k < a.lsz * NIB; k += L) a.cand_info[f * a.lsz * NIB + k] = 0;
                if (p < a.lsz) { a.cand_metric[f * a.lsz + p] = 0.0; a.cand_ok[f * a.lsz + p] = 0; }
            } else active_mask = 1ULL;
            __syncthreads();
        }
        }
        const float* llr32 = (const float*)a.llr + f * N;
        const double* llr64 = (const double*)a.llr + f * N;
        if (active_mask == 0) continue;
        const bool f_store = f_valid && ((active_mask >> (WAVE ? lane / LF : 0)) & 1ULL);

        // ---------------- list decoding (fastpolar.py:278-330)
        // slot of my LLR block at depth d = 1..8: byte d-1 (every path starts as a copy of its frame's path 0)
        // (L > 256: 16 bits per depth, WidePtr16)
        wide_ptr_t<L> pa_, pb_;
        if constexpr (L > 256) { pa_ = wide_ptr_fill_a(fp0); pb_ = wide_ptr_fill_b(fp0); }
        else {
        pa_ = (uint64_t)(uint32_t)fp0 * 0x0101010101010101ULL;
        // slot of my partial-sum block at depth d = 1..5: byte d-1; byte 5: LLR slot at depth 9
        pb_ = (uint64_t)(uint32_t)fp0 * 0x0000010101010101ULL;
        }
        uint32_t b0 = 0;                  // partial-sum blocks of S = 1..16 bits, block of S bits at bit S
        uint32_t hist = 0, anc = 0;       // trace-back window
        double metric = 0.0, lam = 0.0, sp_diff = 0.0, sp_sum = 0.0, lp_odd = 0.0;
        int cnt = 1, info_idx = 0;
        bool dirty = false;               // shared slots may still be being read by a wave that is behind (group-uniform)
        group_sync();

        // One leaf.  The even and the odd leaf of a pair are two instances of this text (ODD a compile-time constant): only the even one
        // walks the tree (an odd leaf's top is depth 10, a g of what its sibling left in LDS), evaluates a softplus and fetches the
        // softplus pair through the sort; the odd one takes its penalty from lp_odd and folds the partial sums upward.
        auto leaf = [&](auto odd_c, const int i) {
            constexpr bool ODD = decltype(odd_c)::value;
            const bool frozen = (a.frozen.w[i >> 5] >> (i & 31)) & 1u;
            // An even leaf's penalty softplus log1p(exp(-|lam|)), right behind the f that forms lam: the straight-line form over the
            // ES_EXP_SHIFT pair that f has just set up; out of range (|lam| >= 512) the generic form, a cold path behind one ballot.
            double lp_even = 0.0;
            auto leaf_softplus = [&](double x, double sh) {
                int bad = 0;
                const double al_ = __builtin_fabs(x);
                double v = es_leaf_softplus_sl_sh(al_, tab, &bad, sh);
                if (__builtin_amdgcn_ballot_w64(bad != 0) != 0ULL) { if (bad) v = es_softplus_neg_generic(-al_, tab); }
                return v;
            };
            if (!ODD && i == 0) {
                // First chain: the paths of a frame are still copies of its path 0, so each node is computed once, the frame's
                // lanes sharing its elements, into that path's slot (a barrier per depth here: lanes read what other lanes wrote).
                #pragma unroll 1
                for (int d = 1; d <= 9; ++d) {
                    const int S = N >> d;
                    const int rs = wide_low_row(DL, d - 1), rd = wide_low_row(DL, d);      // rows of depth d-1 / d when they are in LDS
                    #pragma unroll 1
                    for (int j = pl; j < S; j += LF) {
                        double pa, pb;
                        if (d == 1) { pa = a.is_f64 ? llr64[j] : (double)llr32[j]; pb = a.is_f64 ? llr64[j + S] : (double)llr32[j + S]; }
                        else if (d <= DL) { pa = A[(long long)(2 * S + j) * L + fp0]; pb = A[(long long)(2 * S + j + S) * L + fp0]; }
                        else { pa = W.low[rs + j][fp0]; pb = W.low[rs + j + S][fp0]; }
                        const double v = es_polar_f_slg(pa, pb, tab);
                        if (d < DL) A[(long long)(S + j) * L + fp0] = v; else W.low[rd + j][fp0] = v;
                    }
                    group_sync();
                }
                {                                                         // (generic softplus as a cold path, as at depth 10 below)
                    const double xa = W.low[lrow(9)][fp0], xb = W.low[lrow(9) + 1][fp0];
                    int bad = 0;
                    const double sh = es_shift_reg();
                    lam = es_polar_f_sl_sp_sh(xa, xb, tab, &sp_diff, &sp_sum, &bad, sh);
                    if (__builtin_amdgcn_ballot_w64(bad != 0) != 0ULL) lam = es_polar_f_sp(xa, xb, tab, &sp_diff, &sp_sum);
                    lp_even = leaf_softplus(lam, sh);
                }
                dirty = true;
            } else {
                if constexpr (!ODD) {
                const int top = NLEV - __builtin_ctz((unsigned)i);
                if (top <= 9 && dirty) { group_sync(); dirty = false; }         // this step writes slots
                // --- depths top..DL-1: slab to slab, the lane walks the node
                bool have_dl = false;                                               // depth DL already formed (in LDS) by a fused pass of this step
                int d_first = top;
                // Depth 1 of the SECOND half of the code word (bits 512..) is g(llr[e], llr[e + 512], u1[e]) = llr[e + 512] +- llr[e]: one bit of the
                // 512-bit partial-sum block picks one of two values that the frame's channel LLRs already hold.  It is never stored (512 doubles written
                // and twice read per path otherwise: 8.5 % of the slab traffic, and a 512-element load-add-store loop): the two passes that consume it --
                // the f level of depth 2 at bit 512, the g level of depth 2 (fused with the f level of depth 3) at bit 768 -- form its elements on the
                // fly from the channel LLRs (shared by the frame's paths: the lanes of a frame read the same addresses).
                // (float32 channel LLRs -- what es_llr_batch produces; a float64 launch keeps depth 1 in the slab.  The operands come from the L1 / L2,
                // not from the slab: one operand set ahead, rotated by copy, is enough.)
                if ((i == 512 || i == 768) && !a.is_f64) {
                    const int bs1 = p8_get(pb_, 0);                                 // slot of my 512-bit partial-sum block
                    double* const dst2 = A + (long long)256 * L + p;                // depth 2 at elements [256, 512)
                    auto g1 = [&](float lo, float hi, uint32_t u) { return es_polar_g((double)lo, (double)hi, u); };      // depth-1 element from llr[e], llr[e + 512]
                    if (i == 512) {
                        auto ld = [&](int j, float (&q)[4]) { q[0] = llr32[j]; q[1] = llr32[j + 512]; q[2] = llr32[j + 256]; q[3] = llr32[j + 768]; };
                        if constexpr (WAVE && LF >= 8) {
                        // The channel LLRs belong to the frame and the two signs are one bit each: element j of depth 2 takes one of FOUR values,
                        // whatever the path.  The frame's LF lanes evaluate them once between them: in a round of LF / 4 elements lane pl evaluates
                        // element pl >> 2 for sign combination pl & 3 (both bits lane constants: no bit extraction in the evaluation), and every path
                        // then takes each element of the round from the lane that holds its combination (ds_bpermute, registers only: nothing is
                        // stored but the results, and no fence is needed).  1024 / LF evaluations a lane instead of 256: 128 at L = 8, 16 at L = 64.
                        // Same g1 and f on the same operands, so the same bits: only the lane that evaluates them differs.  All 64 lanes are active
                        // here (dead paths and mirrored frames decode along), so every source lane of the exchange holds a value.
                        // (Measured against a 4 x 256 table in dead rows of the slab with a gather behind a fence: the table gave 0.3-1.3 % on
                        // the headline step, the exchange 1.7-2.7 %)
                        {
                            constexpr int ST = LF / 4;                              // elements per round: lane pl evaluates element pl >> 2 of the round
                            const int plo = wide_opaque(pl), c = plo & 3;               // my sign combination: bit 0 for (j, j + 512), bit 1 for (j + 256, j + 768)
                            const uint32_t ua = (uint32_t)c & 1u, ub = (uint32_t)c >> 1;
                            const int jl = plo >> 2;
                            const int fb = (p - plo) << 2;                          // ds_bpermute address of the frame's lane 0
                            // every path takes element j0 + t of a round from the lane of its frame that evaluated combination (t, my two bits)
                            auto hand_out = [&](double v, int j0, uint32_t ba, uint32_t bb) {
                                const int lo = (int)(uint32_t)__double_as_longlong(v), hi = (int)(uint32_t)((uint64_t)__double_as_longlong(v) >> 32);
                                #pragma unroll
                                for (int t = 0; t < ST; ++t) {
                                    const int src = fb + (int)((((ba >> t) & 1u) | (((bb >> t) & 1u) << 1) | (uint32_t)(4 * t)) << 2);
                                    const uint32_t xl = (uint32_t)__builtin_amdgcn_ds_bpermute(src, lo), xh = (uint32_t)__builtin_amdgcn_ds_bpermute(src, hi);
                                    dst2[(long long)(j0 + t) * L] = __longlong_as_double((long long)(((uint64_t)xh << 32) | xl));
                                }
                            };
                            float q0[4], q1[4];                                     // two operand sets in rotation (renamed, not copied)
                            ld(jl, q0); ld(jl + ST, q1);
                            uint32_t wa = 0, wb = 0;                                // my partial-sum bits of elements j .. and j + 256 .., a word per 32 elements
                            #pragma unroll 1
                            for (int j = 0; j < 256; j += 2 * ST) {                 // two rounds per pass
                                if ((j & 31) == 0) { wa = beta_ld((512 + j) >> 5, bs1); wb = beta_ld((512 + j + 256) >> 5, bs1); }
                                const double v0 = es_polar_f_slg(g1(q0[0], q0[1], ua), g1(q0[2], q0[3], ub), tab);
                                ld((j + 2 * ST + jl) & 255, q0);                    // (past the end: any element)
                                hand_out(v0, j, wa, wb);
                                const double v1 = es_polar_f_slg(g1(q1[0], q1[1], ua), g1(q1[2], q1[3], ub), tab);
                                ld((j + 3 * ST + jl) & 255, q1);
                                hand_out(v1, j + ST, wa >> ST, wb >> ST);
                                wa >>= (2 * ST) & 31; wb >>= (2 * ST) & 31;          // (LF = 64: a pass is a whole word, reloaded above)
                            }
                        }
                        } else {
                        float q[4], qn[4];
                        ld(0, q);
                        #pragma unroll 1
                        for (int j0 = 0; j0 < 256; j0 += 32) {
                            const uint32_t wa = beta_ld((512 + j0) >> 5, bs1), wb = beta_ld((512 + j0 + 256) >> 5, bs1);
                            #pragma unroll 1
                            for (int u = 0; u < 32; ++u) {
                                const int j = j0 + u;
                                ld(j < 255 ? j + 1 : 255, qn);
                                dst2[(long long)j * L] = es_polar_f_slg(g1(q[0], q[1], (wa >> u) & 1u), g1(q[2], q[3], (wb >> u) & 1u), tab);
                                #pragma unroll
                                for (int k = 0; k < 4; ++k) q[k] = qn[k];
                            }
                        }
                        }
                    } else {
                        const int bs2 = p8_get(pb_, 1);                             // slot of my 256-bit block
                        double* const dst3 = A + (long long)128 * L + p;            // depth 3 at elements [128, 256)
                        auto ld = [&](int j, float (&q)[8]) {
                            q[0] = llr32[j]; q[1] = llr32[j + 512]; q[2] = llr32[j + 256]; q[3] = llr32[j + 768];
                            q[4] = llr32[j + 128]; q[5] = llr32[j + 640]; q[6] = llr32[j + 384]; q[7] = llr32[j + 896];
                        };
                        float q[8], qn[8];
                        ld(0, q);
                        #pragma unroll 1
                        for (int j0 = 0; j0 < 128; j0 += 32) {
                            const uint32_t w1a = beta_ld((512 + j0) >> 5, bs1), w1b = beta_ld((512 + j0 + 256) >> 5, bs1);
                            const uint32_t w1c = beta_ld((512 + j0 + 128) >> 5, bs1), w1d = beta_ld((512 + j0 + 384) >> 5, bs1);
                            const uint32_t w2a = beta_ld((256 + j0) >> 5, bs2), w2b = beta_ld((256 + j0 + 128) >> 5, bs2);
                            #pragma unroll 1
                            for (int u = 0; u < 32; ++u) {
                                const int j = j0 + u;
                                ld(j < 127 ? j + 1 : 127, qn);
                                const double x = es_polar_g(g1(q[0], q[1], (w1a >> u) & 1u), g1(q[2], q[3], (w1b >> u) & 1u), (w2a >> u) & 1u);   // depth-2 element j
                                const double y = es_polar_g(g1(q[4], q[5], (w1c >> u) & 1u), g1(q[6], q[7], (w1d >> u) & 1u), (w2b >> u) & 1u);   // ... and j + 128
                                dst2[(long long)j * L] = x;
                                dst2[(long long)(j + 128) * L] = y;
                                dst3[(long long)j * L] = es_polar_f_slg(x, y, tab);
                                #pragma unroll
                                for (int k = 0; k < 8; ++k) q[k] = qn[k];
                            }
                        }
                    }
                    pa_ = p8_set(pa_, 1, p);
                    d_first = 3;
                    if (i == 768) { pa_ = p8_set(pa_, 2, p); d_first = 4; }
                }
                for (int d = d_first; d < DL; ++d) {
                    const int S = N >> d;
                    const bool is_g = (i >> (NLEV - d)) & 1;
                    const int ps = (d > 1) ? p8_get(pa_, d - 2) : 0;
                    const double* par = A + (long long)(2 * S) * L + ps;          // depth d-1 block at elements [2S, 4S)
                    double* dst = A + (long long)S * L + p;                        // depth d block at elements [S, 2S)
                    // The loaders are chosen OUTSIDE the element loops (slab / float32 LLRs / float64 LLRs): a branch inside a loader puts
                    // control flow between a load and its use, and the compiler then waits for ALL outstanding loads (s_waitcnt vmcnt(0)) right
                    // after issuing each pair -- the batches below would run one memory round trip per pair instead of GBATCH pairs in flight.
                    auto ld_slab = [&](int j, double& pa, double& pb) { pa = par[(long long)j * L]; pb = par[(long long)(j + S) * L]; };
                    if (d > 1 && d < 7 && is_g) {
                        // Two levels in ONE pass: level d, the g of the bit just decided at the top of a step, and the f level below it.
                        // (Fusing pairs of f levels as well measured no gain.  Its arm -- pair_ff and the !is_g loop -- can no longer be reached
                        // but stays in the text: without it the compiler allocates the kernel's registers differently, and the tuned code object
                        // is to stay as it is.)  The two level-d results that make an f operand pair -- elements i and i + S/2 -- are formed
                        // together, stored (their g child reads them later) and consumed from registers, so that level d+1 does not read
                        // back what was written S elements earlier (at these sizes from the Infinity Cache or HBM).
                        const int bs = (is_g && d <= 5) ? p8_get(pb_, d - 1) : 0;
                        const int H = S >> 1;
                        double* dstB = A + (long long)H * L + p;                   // depth d+1 block at elements [H, 2H)
                        auto ld4 = [&](int j, double (&q)[4]) {
                            q[0] = par[(long long)j * L]; q[1] = par[(long long)(j + S) * L];
                            q[2] = par[(long long)(j + H) * L]; q[3] = par[(long long)(j + H + S) * L];
                        };
                        // (the lower level's destination -- slab, or LDS when it is depth DL -- is chosen outside the element loops, like the loaders)
                        auto fused_pass = [&](auto stB) {
                        auto pair_gf = [&](int j, const double (&q)[4], uint32_t u1, uint32_t u2) {
                            const double g1 = es_polar_g(q[0], q[1], u1), g2 = es_polar_g(q[2], q[3], u2);
                            dst[(long long)j * L] = g1;
                            dst[(long long)(j + H) * L] = g2;
                            stB(j, es_polar_f_slg(g1, g2, tab));
                        };
                        auto pair_ff = [&](int j, const double (&q)[4]) {
                            const double f1 = es_polar_f_slg(q[0], q[1], tab);
                            dst[(long long)j * L] = f1;
                            const double f2 = es_polar_f_slg(q[2], q[3], tab);
                            dst[(long long)(j + H) * L] = f2;
                            stB(j, es_polar_f_slg(f1, f2, tab));
                        };
                        const int blk = H < 32 ? H : 32;
                        for (int i0 = 0; i0 < H; i0 += blk) {
                            uint32_t w1 = 0, w2 = 0;                                // partial-sum bits of elements i0 .. and i0 + H ..
                            if (is_g) {
                                if (S >= 64) { w1 = beta_ld((S + i0) >> 5, bs); w2 = beta_ld((S + i0 + H) >> 5, bs); }
                                else if (S == 32) { w1 = beta_ld(1, bs); w2 = w1 >> 16; }
                                else { w1 = b0 >> S; w2 = w1 >> H; }
                            }
                            double q0[4], q1[4];
                            ld4(i0, q0); ld4(i0 + 1, q1);
                            if (is_g) {
                                for (int u = 0; u < blk; u += 2) {                  // two operand sets in rotation (renamed, not copied)
                                    pair_gf(i0 + u, q0, (w1 >> u) & 1u, (w2 >> u) & 1u);
                                    ld4(u + 2 < blk ? i0 + u + 2 : i0 + blk - 1, q0);
                                    pair_gf(i0 + u + 1, q1, (w1 >> (u + 1)) & 1u, (w2 >> (u + 1)) & 1u);
                                    ld4(u + 3 < blk ? i0 + u + 3 : i0 + blk - 1, q1);
                                }
                            } else {
                                for (int u = 0; u < blk; u += 2) {
                                    pair_ff(i0 + u, q0);
                                    ld4(u + 2 < blk ? i0 + u + 2 : i0 + blk - 1, q0);
                                    pair_ff(i0 + u + 1, q1);
                                    ld4(u + 3 < blk ? i0 + u + 3 : i0 + blk - 1, q1);
                                }
                            }
                        }
                        };
                        bool to_lds = false;
                        if constexpr (DL <= 7) to_lds = (d + 1 == DL);
                        if (to_lds) { fused_pass([&](int j, double v) { W.low[j][p] = v; }); have_dl = true; }       // depth DL: rows 0 ..
                        else fused_pass([&](int j, double v) { dstB[(long long)j * L] = v; });
                        pa_ = p8_set(pa_, d - 1, p);
                        ++d;                                                        // level d+1 is done too
                        pa_ = p8_set(pa_, d - 1, p);
                        continue;
                    }
                    if (is_g) {
                        const int bs = (d <= 5) ? p8_get(pb_, d - 1) : 0;
                        auto g_level = [&](auto ld) {
                            for (int j0 = 0; j0 < S; j0 += 32) {
                                uint32_t wbits; int nb;
                                if (S >= 32) { wbits = beta_ld((S + j0) >> 5, bs); nb = 32; }
                                else { wbits = b0 >> S; nb = S; }
                                for (int u = 0; u < nb; u += WIDE_GBATCH) {     // (g is an add: the loop is memory latency) GBATCH independent load pairs in flight
                                    double xa[WIDE_GBATCH], xb[WIDE_GBATCH];
                                    #pragma unroll
                                    for (int v = 0; v < WIDE_GBATCH; ++v) ld(j0 + u + v, xa[v], xb[v]);
                                    #pragma unroll
                                    for (int v = 0; v < WIDE_GBATCH; ++v) dst[(long long)(j0 + u + v) * L] = es_polar_g(xa[v], xb[v], (wbits >> (u + v)) & 1u);
                                }
                            }
                        };
                        if (d > 1) g_level(ld_slab);
                        else if (a.is_f64) g_level([&](int j, double& pa, double& pb) { pa = llr64[j]; pb = llr64[j + S]; });      // d == 1 (i == 512): the channel LLRs
                        else g_level([&](int j, double& pa, double& pb) { pa = (double)llr32[j]; pb = (double)llr32[j + S]; });
                    } else {
                        // an f level is never the top of a step (the top is the g whose bit was just decided): d >= 2, operands from the slab
                        // three operand pairs in rotation, the loop unrolled by three so that the rotation is a renaming, not a copy (a copy of a
                        // register that a load is still filling waits for the load): the operands of element j + 3 are requested right after
                        // f(j) and used two f evaluations later.  Loads past the end re-read the last element (S >= 8).
                        double a0, b0_, a1, b1_, a2, b2_;
                        ld_slab(0, a0, b0_); ld_slab(1, a1, b1_); ld_slab(2, a2, b2_);
                        for (int j = 0; ; j += 3) {
                            dst[(long long)j * L] = es_polar_f_slg(a0, b0_, tab);
                            if (j + 1 >= S) break;
                            ld_slab(j + 3 < S ? j + 3 : S - 1, a0, b0_);
                            dst[(long long)(j + 1) * L] = es_polar_f_slg(a1, b1_, tab);
                            if (j + 2 >= S) break;
                            ld_slab(j + 4 < S ? j + 4 : S - 1, a1, b1_);
                            dst[(long long)(j + 2) * L] = es_polar_f_slg(a2, b2_, tab);
                            if (j + 3 >= S) break;
                            ld_slab(j + 5 < S ? j + 5 : S - 1, a2, b2_);
                        }
                    }
                    pa_ = p8_set(pa_, d - 1, p);
                }
                // --- depths DL..9 in LDS: level DL from the slab (unless a fused pass has just formed it), the others LDS -> LDS; S = 1024 >> d
                // elements by slot.  (The generic softplus is a cold path after the level, instead of a branch after each evaluation, at every depth
                // but 8: at levels of 8 or 16 elements and at depths 9 and 10.  Depth 8 -- 4 elements -- keeps the branch.)
                auto low_level = [&](auto dc, auto from_slab) {
                    constexpr int d = decltype(dc)::value;
                    constexpr int S = N >> d;
                    constexpr bool SLAB = decltype(from_slab)::value;
                    constexpr bool DEFER = S > 4 || d == 9;                           // all but depth 8
                    constexpr int rs = wide_low_row(DL, d - 1), rd = wide_low_row(DL, d);
                    constexpr int C = S < 4 ? S : 4;                                  // f evaluations per chunk (registers are indexed statically: no private arrays)
                    const int ps = p8_get(pa_, d - 2);                                // slot of my depth d-1 block
                    const double* par = A + (long long)(2 * S) * L + ps;              // (SLAB: depth d-1 at elements [2S, 4S))
                    auto src = [&](int e) -> double { if constexpr (SLAB) return par[(long long)e * L]; else return W.low[rs + e][ps]; };
                    if ((i >> (NLEV - d)) & 1) {
                        double x[2 * S];
                        #pragma unroll
                        for (int u = 0; u < 2 * S; ++u) x[u] = src(u);
                        #pragma unroll
                        for (int j = 0; j < S; ++j) W.low[rd + j][p] = es_polar_g(x[j], x[j + S], (b0 >> (S + j)) & 1u);
                    } else if constexpr (DEFER) {
                        int bad = 0;
                        #pragma unroll 1
                        for (int c = 0; c < S; c += C) {
                            double x[2 * C];
                            #pragma unroll
                            for (int u = 0; u < C; ++u) { x[u] = src(c + u); x[C + u] = src(c + u + S); }
                            #pragma unroll
                            for (int u = 0; u < C; ++u) W.low[rd + c + u][p] = es_polar_f_sl(x[u], x[C + u], tab, &bad);
                        }
                        if (__builtin_amdgcn_ballot_w64(bad != 0) != 0ULL) {          // rare: the level again with the generic form
                            #pragma unroll 1
                            for (int j = 0; j < S; ++j) W.low[rd + j][p] = es_polar_f(src(j), src(j + S), tab);
                        }
                    } else {
                        double x[2 * S];
                        #pragma unroll
                        for (int u = 0; u < 2 * S; ++u) x[u] = src(u);
                        #pragma unroll 2
                        for (int j = 0; j < S; ++j) W.low[rd + j][p] = es_polar_f_slg(x[j], x[j + S], tab);
                    }
                    if constexpr (d <= 8) pa_ = p8_set(pa_, d - 1, p); else pb_ = p8_set(pb_, 5, p);
                };
                using std::integral_constant;
                if (top <= DL && !have_dl) low_level(integral_constant<int, DL>{}, std::true_type{});
                if constexpr (DL < 8) { if (top <= 8) low_level(integral_constant<int, 8>{}, std::false_type{}); }
                if (top <= 9) low_level(integral_constant<int, 9>{}, std::false_type{});
                }
                // --- depth 10: LDS -> register
                {
                    const int ps = p8_get(pb_, 5);
                    const double xa = W.low[lrow(9)][ps], xb = W.low[lrow(9) + 1][ps];
                    if constexpr (ODD) lam = es_polar_g(xa, xb, (b0 >> 1) & 1u);
                    else {                                                // (generic softplus as a cold path, as at depth 9)
                        int bad = 0;
                        const double sh = es_shift_reg();
                        lam = es_polar_f_sl_sp_sh(xa, xb, tab, &sp_diff, &sp_sum, &bad, sh);
                        if (__builtin_amdgcn_ballot_w64(bad != 0) != 0ULL) lam = es_polar_f_sp(xa, xb, tab, &sp_diff, &sp_sum);
                        lp_even = leaf_softplus(lam, sh);
                    }
                }
                dirty = true;
            }

            // --- decision
            const double al = __builtin_fabs(lam);
            const double lp = ODD ? lp_odd : lp_even;               // lp_odd: set when the even sibling was decided
            const uint32_t pref = (lam >= 0.0) ? 1u : 0u;
            uint32_t bit = 0;
            if (frozen) {                                             // fastpolar.py:281-286
                metric = metric + es_leaf_penalty(lp, al, pref, 0u);
                if constexpr (!ODD) lp_odd = sp_sum;                  // sibling g = b + a when this bit is 0
            } else {                                                  // fastpolar.py:288-330
                const bool live = pl < cnt;
                const int nc = 2 * cnt;
                double k0 = live ? metric + es_leaf_penalty(lp, al, pref, 0u) : __builtin_inf();
                double k1 = live ? metric + es_leaf_penalty(lp, al, pref, 1u) : __builtin_inf();
                uint32_t i0 = live ? (uint32_t)(2 * pl) : 0xFFFFu, i1 = live ? (uint32_t)(2 * pl + 1) : 0xFFFFu;   // candidate index within the frame
                const bool wstart = (info_idx & 31) == 0;
                const int keep = nc < a.lsz ? nc : a.lsz;          // a.lsz <= LF: lists of any size run on the next power of two's kernel
                const int myr = pl < keep ? pl : 0;                // dead paths mirror rank 0
                if constexpr (WAVE) {
                    // One wave: the survivor of rank r takes sorted element r and then its parent's state straight from the registers of the
                    // lanes that hold them (ds_bpermute: no LDS storage, no fence -- the lanes of a wave run in lock step).
                    int buf = 0;
                    wide_sort<L, LF>(k0, i0, k1, i1, p, pl, W, buf);
                    auto fetch32 = [](int src, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v); };
                    auto fetch64 = [&](int src, uint64_t v) { return ((uint64_t)fetch32(src, (uint32_t)(v >> 32)) << 32) | fetch32(src, (uint32_t)v); };
                    const int holder = fp0 + (myr >> 1);           // sorted element e sits in lane e / 2 of the frame, half e % 2
                    const uint64_t e0 = fetch64(holder, __builtin_bit_cast(uint64_t, k0)), e1 = fetch64(holder, __builtin_bit_cast(uint64_t, k1));
                    const uint32_t ei = fetch32(holder, (i0 & 0xFFFFu) | (i1 << 16));
                    metric = __builtin_bit_cast(double, (myr & 1) ? e1 : e0);
                    const uint32_t myc = (myr & 1) ? (ei >> 16) : (ei & 0xFFFFu);
                    const int parent = fp0 + ((int)(myc >> 1) & (LF - 1));
                    bit = myc & 1u;
                    const uint64_t t = fetch64(parent, pb_ | ((uint64_t)(wstart ? (uint32_t)pl : anc) << 48));
                    pa_ = fetch64(parent, pa_);
                    pb_ = t & 0xFFFFFFFFFFFFULL;
                    anc = (uint32_t)(t >> 48);
                    b0 = fetch32(parent, b0);
                    hist = (fetch32(parent, wstart ? 0u : hist) << 1) | bit;
                    if constexpr (!ODD) {
                        const uint64_t sd = fetch64(parent, __builtin_bit_cast(uint64_t, sp_diff)), ss = fetch64(parent, __builtin_bit_cast(uint64_t, sp_sum));
                        lp_odd = __builtin_bit_cast(double, bit ? sd : ss);
                    }
                } else {
                // publish what follows a path through the sort
                const int xb = (NBUF == 2) ? (info_idx & 1) : 0;
                if constexpr (!WAVE && NBUF == 1) __syncthreads();         // one buffer: every wave has read the last sort's
                W.pub.xpa[xb][p] = pa_;
                if constexpr (L > 256) W.pub.xpb[xb][p] = wide_ptr_join(pb_, wstart ? (uint32_t)pl : anc);
                else W.pub.xpb[xb][p] = pb_ | ((uint64_t)(wstart ? (uint32_t)pl : anc) << 48);
                W.pub.xb0[xb][p] = b0;
                W.pub.xhist[xb][p] = wstart ? 0u : hist;
                if constexpr (!ODD) { W.pub.xsp[xb][0][p] = sp_diff; W.pub.xsp[xb][1][p] = sp_sum; }
                int buf = 0;
                wide_sort<L, LF>(k0, i0, k1, i1, p, pl, W, buf);
                if constexpr (!WAVE && NBUF == 1) __syncthreads();         // one buffer: every wave has read the last cross-wave stage
                W.pub.skey[buf][2 * p] = k0; W.pub.skey[buf][2 * p + 1] = k1;
                W.pub.sidx[buf][2 * p] = (uint16_t)i0; W.pub.sidx[buf][2 * p + 1] = (uint16_t)i1;
                if constexpr (WAVE) wave_fence_lds(); else __syncthreads();
                const uint32_t myc = W.pub.sidx[buf][2 * fp0 + myr];
                metric = W.pub.skey[buf][2 * fp0 + myr];
                const int parent = fp0 + ((int)(myc >> 1) & (LF - 1));
                bit = myc & 1u;
                pa_ = W.pub.xpa[xb][parent];
                if constexpr (L > 256) wide_ptr_split(W.pub.xpb[xb][parent], pb_, anc);
                else {
                const uint64_t t = W.pub.xpb[xb][parent];
                pb_ = t & 0xFFFFFFFFFFFFULL;
                anc = (uint32_t)(t >> 48);
                }
                b0 = W.pub.xb0[xb][parent];
                hist = (W.pub.xhist[xb][parent] << 1) | bit;
                if constexpr (!ODD) lp_odd = W.pub.xsp[xb][bit ? 0 : 1][parent];
                }
                if ((info_idx & 31) == 31) { TBW[(info_idx >> 5) * L + p] = hist; TBA[(info_idx >> 5) * L + p] = (uint16_t)anc; }
                cnt = keep;
                ++info_idx;
                if constexpr (!WAVE) dirty = false;                // every wave passed the sort's barriers after its reads
            }

            // --- partial sums: fold upward while the node is a right child (fastpolar.py:156-183); each lane its own path
            const int t = ODD ? __builtin_ctz(~(unsigned)i) : 0;   // (an even leaf is a left child: its bit becomes the 1-bit block)
            if (t < NLEV) {
                uint32_t cw = bit;
                const int t5 = t < 5 ? t : 5;
                for (int s = 0; s < t5; ++s) {
                    const int S = 1 << s;
                    const uint32_t left = (b0 >> S) & ((1u << S) - 1u);
                    cw = (left ^ cw) | (cw << S);
                }
                if (t < 5) {
                    const int Sp = 1 << t;
                    const uint32_t mask = ((1u << Sp) - 1u) << Sp;
                    b0 = (b0 & ~mask) | (cw << Sp);
                } else {
                    if (t > 5) {
                        CB[p] = cw;
                        for (int s = 5; s < t; ++s) {
                            const int Wd = 1 << (s - 5);
                            const int bs = p8_get(pb_, NLEV - s - 1);
                            for (int w = 0; w < Wd; ++w) {
                                const uint32_t c0 = CB[w * L + p];
                                const uint32_t lf = beta_ld(Wd + w, bs);
                                CB[(Wd + w) * L + p] = c0;
                                CB[w * L + p] = c0 ^ lf;
                            }
                        }
                    }
                    if (dirty) { group_sync(); dirty = false; }     // the block about to be rewritten may still be being read
                    const int Wp = 1 << (t - 5);
                    if (t == 5) beta_st(1, p, cw);
                    else for (int w = 0; w < Wp; ++w) beta_st(Wp + w, p, CB[w * L + p]);
                    pb_ = p8_set(pb_, NLEV - t - 1, p);
                }
            }
        };
        for (int i = 0; i < N; i += 2) { leaf(std::false_type{}, i); leaf(std::true_type{}, i + 1); }

        // ---------------- final ordering (fastpolar.py:335), trace-back, CRC -- per frame
        group_sync();
        W.low[0][p] = metric;                                       // (the list loop is over: the LLR rows are free; a lane's own cell -- waves that are groups of their own run out of step)
        group_sync();
        int rank = 0;
        for (int k = 0; k < cnt; ++k) {
            const double mk = W.low[0][fp0 + k];
            rank += ((mk < metric) || (mk == metric && k < pl)) ? 1 : 0;
        }
        if constexpr (GK) {
            const int r = a.n_info & 31;                             // a last, partial window: its bits move up to the MSB end like a full one's
            if (r) { TBW[(a.n_info >> 5) * L + p] = hist << (32 - r); TBA[(a.n_info >> 5) * L + p] = (uint16_t)anc; }
            group_sync();
        }
        if (pl < cnt && f_store) {
            uint8_t* out = a.cand_info + (f * a.lsz + rank) * NIB;
            int curp = pl;
            if constexpr (GK) {
                const int nw = (a.n_info + 31) >> 5, nbits = a.n_info - 8, rem = nbits & 7, kc = nbits >> 3;
                uint32_t reg = 0, lo = 0, hi = 0;                    // lo, hi: the two bytes the 8 CRC bits lie in
                #pragma unroll 1
                for (int w = nw - 1; w >= 0; --w) {                  // windows are read last to first (each names its ancestor in the one before) ...
                    const uint32_t wd = TBW[w * L + fp0 + curp];
                    curp = (int)TBA[w * L + fp0 + curp] & (LF - 1);
                    #pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = 4 * w + q;
                        const uint32_t byte = (wd >> (24 - 8 * q)) & 0xffu;
                        if (k == kc) lo = byte; else if (k == kc + 1) hi = byte;
                        if (k < NIB) out[k] = (uint8_t)((rem && k == NIB - 1) ? (byte & (0xffu << (8 - rem))) : byte);
                    }
                }
                #pragma unroll 1
                for (int k = 0; k < kc; ++k) {                       // ... and the CRC runs first to last over the row just written (this lane's own bytes)
                    reg ^= out[k];
                    #pragma unroll
                    for (int b = 0; b < 8; ++b) reg = (reg & 0x80u) ? ((reg << 1) ^ 0x07u) & 0xffu : (reg << 1) & 0xffu;
                }
                for (int b = 0; b < rem; ++b) {
                    reg ^= ((lo >> (7 - b)) & 1u) << 7;
                    reg = (reg & 0x80u) ? ((reg << 1) ^ 0x07u) & 0xffu : (reg << 1) & 0xffu;
                }
                a.cand_metric[f * a.lsz + rank] = metric;
                a.cand_ok[f * a.lsz + rank] = (uint8_t)(reg == ((((lo << 8) | hi) >> (8 - rem)) & 0xffu));
            } else {
            uint32_t wd[MWIN_W];
            #pragma unroll
            for (int w = MWIN_W - 1; w >= 0; --w) {
                wd[w] = TBW[w * L + fp0 + curp];                  // information bits 32w .. 32w+31, first = MSB
                curp = (int)TBA[w * L + fp0 + curp] & (LF - 1);
            }
            uint32_t reg = 0;
            #pragma unroll
            for (int k = 0; k < ES_INFO_BYTES; ++k) {
                const uint32_t byte = (wd[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu;
                out[k] = (uint8_t)byte;
                reg ^= byte;
                #pragma unroll
                for (int b = 0; b < 8; ++b) reg = (reg & 0x80u) ? ((reg << 1) ^ 0x07u) & 0xffu : (reg << 1) & 0xffu;
            }
            a.cand_metric[f * a.lsz + rank] = metric;
            a.cand_ok[f * a.lsz + rank] = (uint8_t)(reg == (wd[MWIN_W - 1] & 0xffu));
            }
        }
        if (pl == 0 && f_store) a.ncand[f] = cnt;
        group_sync();
    }
    // ---- release the slot: every wave's slab stores are done (and performed) before the bit clears.  The fence is agent-scope: on a
    // chip whose XCDs have their own L2 it also writes this XCD's dirty slab lines back, so a late eviction here cannot overwrite
    // what the slot's next owner -- possibly on another XCD -- has written since (an owner only ever reads what it wrote itself).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");          // (release only: an acquire would also invalidate this XCD's L2 under the blocks still running)
    __syncthreads();
    if (p == 0) atomicAnd(&a.slot_bits[slot >> 5], ~(1u << (slot & 31)));
}


// es_ctx::wide_attr_mask bit of an instantiation: capacities 1..256 at bits 0..8 (run-time K: 9..17), 512 and 1024 at 18, 19 (20, 21)
constexpr unsigned wide_attr_bit(int LF, bool GK)
{
    return LF <= 256 ? (unsigned)LF << (GK ? 9 : 0) : 1u << (18 + (LF == 1024 ? 1 : 0) + (GK ? 2 : 0));
}

template <int L, int LF, bool GK = false>
int launch_wide(es_ctx* ctx, WideArgs a, int64_t B, hipStream_t st)
{
    const size_t lds = sizeof(WideLds<L, (LF > 64 ? 2 : 1)>);
    static_assert((sizeof(WideLds<256, 2>) + 1279) / 1280 * 1280 * 3 <= 160 * 1024, "three workgroups per CU at L = 256 (LDS is handed out in 1 280-byte granules)");
    static_assert((sizeof(WideLds<128, 2>) + 1279) / 1280 * 1280 * 6 <= 160 * 1024, "six two-wave workgroups per CU at L = 128");
    static_assert((sizeof(WideLds<512, 2>) + 1279) / 1280 * 1280 <= 160 * 1024 && (sizeof(WideLds<512, 2>) + 1279) / 1280 * 1280 * 2 > 160 * 1024,
                  "one workgroup per CU at L = 512 (wide_cu_lanes counts 512 lanes for it)");
    static_assert((sizeof(WideLds<1024, 2>) + 1279) / 1280 * 1280 <= 160 * 1024, "one workgroup per CU at L = 1024 (single-buffered WidePub)");
    static_assert((sizeof(WideLds<64, 1>) + 1279) / 1280 * 1280 * 4 * WIDE_WPS <= 160 * 1024, "4 x WIDE_WPS one-wave workgroups per CU");
    static_assert((LF & (LF - 1)) == 0, "power of two");
    constexpr unsigned attr_bit = wide_attr_bit(LF, GK);               // one instantiation per list capacity (and per kind of code)
    if (!(ctx->wide_attr_mask & attr_bit)) {                           // per context (= per device): the attribute belongs to the device's copy of the kernel
        ES_HIP_CHECK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&es_scl_wide_kernel<L, LF, GK>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ctx->wide_attr_mask |= attr_bit;
    }
    // One slab slot per resident workgroup.  The slab is sized in lanes (es_scl_wide_scratch_bytes); a block of L lanes gets
    // wide_lanes / L slots out of it.
    constexpr int FRB = L / LF;                                     // frames per block
    const long long blocks = (B + FRB - 1) / FRB;                    // one frame group per wave / block; the hardware keeps <= 3 blocks (L = 128: 5) per CU resident
    if (blocks >= (1LL << 31)) { ctx->err = "es_scl_batch: batch too large for one launch"; return ES_EINVAL; }
    a.slot_bits = ctx->d_wide_slot_bits;
    a.n_slots = (int)(ctx->wide_lanes / L);
    a.slot_words = (a.n_slots + 31) / 32;
    if (a.slot_words > ctx->wide_slot_words) { ctx->err = "es_scl_batch: the lane-per-path slab has more slots than its bitmap"; return ES_EINVAL; }   // (never: es_create sizes both)
    constexpr int shape = 0x30000 | L;                               // slot stride depends on the block's lanes only (one tag per block size)
    { const int rc = es_slab_enter(ctx, 1, shape, true, st); if (rc) return rc; }
    { const int rc = es_launch(ctx, es_scl_wide_kernel<L, LF, GK>, (unsigned)blocks, L, lds, st, a); if (rc) return rc; }
    { const int rc = es_slab_leave(ctx, 1, shape, true, st); if (rc) return rc; }
    return ES_OK;
}

// Arguments of a launch (and its frame counter, when the frames are drawn from one).
int wide_args(es_ctx* ctx, WideArgs& a, const es_scl_io& io, hipStream_t st)
{
    a = WideArgs{};
    a.llr = io.llr; a.is_f64 = (io.dtype == ES_DTYPE_F64); a.B = io.B;
    a.frozen = ctx->frozen; a.data_pos = ctx->d_data_pos; a.exp_tab = ctx->d_exp_tab;
    a.alpha = reinterpret_cast<double*>(ctx->d_wide_scratch);
    a.aux = reinterpret_cast<unsigned char*>(ctx->d_wide_scratch) + (size_t)ctx->wide_lanes * N * sizeof(double);
    a.hard_info = io.hard_info; a.hard_ok = io.hard_ok; a.cand_info = io.cand_info;
    a.cand_metric = io.cand_metric; a.cand_ok = io.cand_ok; a.ncand = io.ncand;
    a.skip_if_hard_ok = io.skip_if_hard_ok;
    a.lsz = io.L;
    a.prio = ctx->scl_prio;
    a.n_info = ctx->n_info; a.info_bytes = (ctx->n_info - 8 + 7) / 8;
    if (io.skip_if_hard_ok) {                                // frames drawn from a counter: see the kernel (settled frames never ride along as idle lanes, as they did in fixed groups)
        if (io.B >= (1LL << 31) - (1LL << 24)) { ctx->err = "es_scl_batch: batch too large for one launch"; return ES_EINVAL; }   // (the counter runs past B by one draw per block)
        const int rc = es_cursor_next(ctx, st, &a.cursor);
        if (rc) return rc;
        ES_HIP_CHECK(ctx, hipMemsetAsync(a.cursor, 0, sizeof(int), st));
    }
    return ES_OK;
}

// The instantiation for a list of L paths: its capacity is the next power of two (this translation unit's share of them).  GK: a code
// other than the reference's own K = 448, on the run-time-K instantiations.
template <bool GK>
int launch_wide_for(es_ctx* ctx, const es_scl_io& io, hipStream_t st)
{
    WideArgs a;
    { const int rc = wide_args(ctx, a, io, st); if (rc) return rc; }
    switch (es_list_cap(io.L)) {
#if ES_WIDE_LARGE_TU
        case 512:  return launch_wide<512, 512, GK>(ctx, a, io.B, st);
        case 1024: return launch_wide<1024, 1024, GK>(ctx, a, io.B, st);
        default: ctx->err = "list_size must be in 1..1024"; return ES_EINVAL;
#else
        case 1:   return launch_wide<64, 1, GK>(ctx, a, io.B, st);
        case 2:   return launch_wide<64, 2, GK>(ctx, a, io.B, st);
        case 4:   return launch_wide<64, 4, GK>(ctx, a, io.B, st);
        case 8:   return launch_wide<64, 8, GK>(ctx, a, io.B, st);
        case 16:  return launch_wide<64, 16, GK>(ctx, a, io.B, st);
        case 32:  return launch_wide<64, 32, GK>(ctx, a, io.B, st);
        case 64:  return launch_wide<64, 64, GK>(ctx, a, io.B, st);
        case 128: return launch_wide<128, 128, GK>(ctx, a, io.B, st);
        case 256: return launch_wide<256, 256, GK>(ctx, a, io.B, st);
        default: ctx->err = "list_size must be in 1..256"; return ES_EINVAL;
#endif
    }
}

#if ES_WIDE_LARGE_TU
}  // namespace

// Lists of 257..1024 paths (es_scl_wide_large.hip): capacities 512 and 1024, one block per CU.
int es_launch_scl_wide_large(es_ctx* ctx, const es_scl_io& io, hipStream_t st)
{
    return ctx->n_info != KINFO ? launch_wide_for<true>(ctx, io, st) : launch_wide_for<false>(ctx, io, st);
}
#else
// Diagnostic: the list decoder's f as its hot loops evaluate it (es_softplus_dev.h, exp table at LDS address 0), for a test against the host.
__global__ __launch_bounds__(256) void es_polar_f_dev_kernel(const double* __restrict__ a, const double* __restrict__ b, long long n,
                                                             const uint64_t* __restrict__ exp_tab, double* __restrict__ out, int* __restrict__ bad)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint64_t* const tab = reinterpret_cast<uint64_t*>(smem_raw);
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_raw != ES_EXP_TAB_LDS_ADDR) __builtin_trap();   // never: no static LDS in this file
    for (int i = threadIdx.x; i < ES_EXP_TAB_WORDS; i += blockDim.x) tab[i] = exp_tab[i];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double sd, ss;
        int bd = 0;
        out[i] = es_polar_f_sl_sp(a[i], b[i], tab, &sd, &ss, &bd);
        out[n + i] = sd;
        out[2 * n + i] = ss;
        bad[i] = bd;
    }
}

}  // namespace

int es_launch_polar_f_dev(es_ctx* ctx, const double* a, const double* b, int64_t n, double* out, int* bad, hipStream_t st)
{
    return es_launch(ctx, es_polar_f_dev_kernel, es_grid(n, 256, ctx->num_cu * 16), 256, ES_EXP_TAB_WORDS * sizeof(uint64_t), st,
                     a, b, (long long)n, ctx->d_exp_tab, out, bad);
}

// Lanes of this file's workgroups one CU holds at most, over the block sizes a context serves (the slab holds a slot per resident
// workgroup): 4 x WIDE_WPS one-wave blocks = WIDE_WPS blocks of 256 lanes = 2 x WIDE_WPS of 128 (768 lanes); ONE block of 512
// lanes (its LDS, checked in launch_wide) or of 1024.
static int wide_cu_lanes(const es_ctx* ctx)
{
    const int small = 4 * WIDE_WPS * 64;
    const int big = ctx->list_size_max > 256 ? es_list_cap(ctx->list_size_max) : 0;
    return big > small ? big : small;
}

// Scratch for this file's kernels: per lane of a resident workgroup 1024 doubles + WIDE_AUX_PER_PATH bytes, for as many lanes as the CUs
// hold at most over the block sizes the context serves (wide_cu_lanes); a block of L lanes takes L of them as one slot.
size_t es_scl_wide_scratch_bytes(const es_ctx* ctx, long long* lanes_out)
{
    if (!ctx->wide_enabled) { *lanes_out = 0; return 0; }
    const long long lanes = (long long)ctx->num_cu * wide_cu_lanes(ctx);
    *lanes_out = lanes;
    return (size_t)lanes * (N * sizeof(double) + (size_t)WIDE_AUX_PER_PATH);
}

int es_launch_scl_wide(es_ctx* ctx, const es_scl_io& io, hipStream_t st)
{
    if (!ctx->d_wide_scratch) { ctx->err = "es_scl_batch: this context has no scratch for the lane-per-path list decoder (list_size_max <= 32 and scl_lanes 1 never requested before es_reserve)"; return ES_EINVAL; }
    if (io.L > ES_MAX_LIST || io.L < 1) { ctx->err = "list_size must be in 1..1024"; return ES_EINVAL; }
    if (io.L > 256) return es_launch_scl_wide_large(ctx, io, st);          // capacities 512 and 1024: a translation unit of their own (es_scl_wide_large.hip)
    return ctx->n_info != KINFO ? launch_wide_for<true>(ctx, io, st) : launch_wide_for<false>(ctx, io, st);
}
#endif
