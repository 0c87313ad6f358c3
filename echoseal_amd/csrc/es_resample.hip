// es_resample.hip -- input conditioning: the polyphase FIR of resample_to (rtwm/utils.py:58-66 =
// scipy.signal.resample_poly -> upfirdn, mode 'constant').  The filter design and padding arithmetic stay on the host
// (they are Python in SciPy); this is upfirdn's inner loop: one lane per output sample, the products x[i] * h[...] added
// to an accumulator that starts at 0, in ascending input index, multiply and add rounded separately, in the arithmetic
// of SciPy's output type (float32 for float32 signals, else float64).  Consecutive lanes read consecutive phases of the
// filter and (nearly) the same input samples: all of it is served from L2.
// Build with -ffp-contract=off.
#include "es_internal.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void es_resample_kernel(const T* __restrict__ x, long long B, long long n_x,
        const T* __restrict__ h_tf, int hpp, int up, int down, long long y0, long long n_out, T* __restrict__ out)
{
    const long long total = B * n_out;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const long long r = g / n_out, k = g - r * n_out;
        const long long yy = y0 + k;
        const long long t = (yy * down) % up, x_idx = (yy * down) / up;
        long long lo = x_idx - hpp + 1, hi = x_idx;
        long long hidx = t * hpp;
        if (lo < 0) { hidx -= lo; lo = 0; }
        if (hi > n_x - 1) hi = n_x - 1;
        const T* xr = x + r * n_x;
        T acc = (T)0;
        for (long long i = lo; i <= hi; ++i) { const T p = xr[i] * h_tf[hidx++]; acc = acc + p; }
        out[g] = acc;
    }
}


// ---- a queue of clips of unequal length and rate in ONE launch (es_resample_ragged_batch) ----------------------------------
// Record r is described by ES_RESAMPLE_DESC_WORDS int64 words (what utils.resample_plan returns, plus where its samples and its filter lie
// in two flat pools).  One workgroup per (record, tile of RS_TILE consecutive outputs): the tile's input window is staged into LDS once with
// coalesced loads (int16 converted there), the rate pair's polyphase table too where it fits (else it is read through L2); lane l computes
// outputs l, l + 256, ... of the tile.  The 64-bit arithmetic of (phase, input index) is done once per tile, for its first output; a lane
// reaches its own output by adding doubled steps (down mod up, down div up) with a carry, in 32 bits, and moves on by the step of 256
// outputs: no division per output.  The arithmetic of one output is es_resample_kernel's: accumulator from +0, products in ascending input
// index, multiply and add rounded separately, in SciPy's output type; float64 is rounded once to float32 on store.
constexpr int RS_TILE = ES_RESAMPLE_TILE;
constexpr int RS_THREADS = 256;
constexpr int RS_WIN_MAX = 4352;                   // window samples in LDS: 1024 outputs at down / up = 4 and 85 taps need 4 181
constexpr int RS_FILT_MAX = 3584;                  // table values in LDS: 44.1 -> 48 kHz has 160 x 21 = 3 360
constexpr int RS_RATE_MAX = 1 << 20;               // up, down above it: the record is refused (32-bit steps inside a tile)
static_assert(RS_TILE % RS_THREADS == 0 && (RS_WIN_MAX + RS_FILT_MAX) * sizeof(double) <= 65536, "tile / LDS geometry");

template <typename S> struct rs_compute { typedef float type; };
template <> struct rs_compute<double> { typedef double type; };
__device__ __forceinline__ float rs_load(const short* p) { return (float)*p / 32768.0f; }
__device__ __forceinline__ float rs_load(const float* p) { return *p; }
__device__ __forceinline__ double rs_load(const double* p) { return *p; }
// LDS is reached through typed pointers only (see rs_tile)
template <typename T> using rs_lds = __attribute__((address_space(3))) T;
__device__ __forceinline__ float rs_load(const rs_lds<float>* p) { return *p; }
__device__ __forceinline__ double rs_load(const rs_lds<double>* p) { return *p; }

// one output: taps m_lo .. m_hi of phase row hp over the window xw (either in LDS or in global memory)
template <typename T, typename XP, typename HP>
__device__ __forceinline__ T rs_dot(XP xw, HP hp, int m_lo, int m_hi)
{
    T acc = (T)0;
    for (int m = m_lo; m <= m_hi; ++m) { const T p = (T)rs_load(xw + m) * hp[m]; acc = acc + p; }
    return acc;
}

// ---- one tile, shared by the ragged and the stream kernel (one body per family) -----------------------------------------
// The body is inlined into thin kernels; its LDS pointers are typed all the same (through a generic pointer the compiler may
// merge neighbouring loads into flat accesses that fault when the address resolves to LDS).

// Where a tile's input window lies.  window(base) -> what rs_dot and the staging loop index by window sample (sample j of the window is
// input index base + j); first(base, neg) -> the lowest window sample that may be read, given the `neg` samples before index 0.
template <typename S> struct rs_clip {                                      // a clip in the sample pool
    const S* x;
    __device__ __forceinline__ const S* window(long long base) const { return x + base; }
    __device__ __forceinline__ int first(long long, int neg) const { return neg; }
};
// a live stream: input index a < n_old lies in the stream's tail row, tail[255 - (n_old - 1 - a)], a >= n_old in the chunk
template <typename S> struct rs_two { const float* tail_end; const S* chunk; int split; };     // window sample j: j < split ? tail_end[j - split] : chunk[j - split]
template <typename S> __device__ __forceinline__ rs_two<S> operator+(rs_two<S> w, int q) { return {w.tail_end, w.chunk, w.split - q}; }
template <typename S> __device__ __forceinline__ float rs_load(rs_two<S> w) { return w.split > 0 ? w.tail_end[-w.split] : rs_load(w.chunk - w.split); }
template <typename S> struct rs_stream {
    const float* tail_end; const S* chunk; long long n_old;                 // tail_end = the tail row + ES_RSTREAM_TAIL
    __device__ __forceinline__ rs_two<S> window(long long base) const
    {
        const long long sp = n_old - base;
        return {tail_end, chunk, (int)(sp > (1ll << 30) ? (1ll << 30) : (sp < -(1ll << 30) ? -(1ll << 30) : sp))};
    }
    __device__ __forceinline__ int first(long long base, int neg) const      // the tail row holds the 255 samples before n_old, no more
    {
        const long long lo = n_old - base - (ES_RSTREAM_TAIL - 1);
        return lo > neg ? (lo > 0x7fffffffll ? 0x7fffffff : (int)lo) : neg;
    }
};

// Outputs yy .. yy + cnt - 1 (indices into the full upfirdn result) of a record of n_in samples, to o[c * out_stride + k], c < rep.
// Block-uniform; ends with a barrier, so the caller may restage the LDS at once.
template <typename T, typename Src>
__device__ __forceinline__ void rs_tile(rs_lds<T>* s_x, rs_lds<T>* s_h, int tid, const Src& src, long long n_in, const T* __restrict__ h,
        int up, int down, int hpp, long long yy, int cnt, float* __restrict__ o, int rep, long long out_stride)
{
    // the tile's first output, in 64 bits, once
    const long long x0 = (yy / up) * down + ((yy % up) * down) / up;        // = yy * down / up without the wide product
    const int t0 = (int)(((yy % up) * down) % up);
    const int dm = down % up, dq = down / up;
    const long long base = x0 - hpp + 1;                                    // input index (record-relative) of window sample 0
    const long long span = ((long long)(cnt - 1) * down + t0) / up + hpp;   // window samples of this tile
    const int neg = src.first(base, base < 0 ? (int)(-base > RS_RATE_MAX ? RS_RATE_MAX : -base) : 0);     // window samples before the record
    const long long last = n_in - 1 - base;                                 // window index of the record's last sample
    const int hi_rel = (int)(last < -1 ? -1 : (last > span - 1 ? span - 1 : last));
    const bool x_lds = span <= RS_WIN_MAX, h_lds = up * hpp <= RS_FILT_MAX;
    const auto xw = src.window(base);
    if (x_lds)
        for (int j = tid; j < (int)span; j += RS_THREADS)
            s_x[j] = (j >= neg && j <= hi_rel) ? (T)rs_load(xw + j) : (T)0;
    if (h_lds)
        for (int j = tid; j < up * hpp; j += RS_THREADS) s_h[j] = h[j];
    __syncthreads();
    // this lane's first output: t0 plus `tid` steps, by doubling
    int p = t0, q = 0, sp = dm, sq = dq;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if ((tid >> b) & 1) { p += sp; q += sq; if (p >= up) { p -= up; ++q; } }
        sq += sq; sp += sp; if (sp >= up) { sp -= up; ++sq; }
    }                                                                       // (sp, sq) is now the step of RS_THREADS outputs
    for (int k = tid; k < cnt; k += RS_THREADS) {
        int m_lo = neg - q; if (m_lo < 0) m_lo = 0;
        int m_hi = hi_rel - q; if (m_hi > hpp - 1) m_hi = hpp - 1;
        T acc;
        if (x_lds) acc = h_lds ? rs_dot<T>(s_x + q, s_h + p * hpp, m_lo, m_hi) : rs_dot<T>(s_x + q, h + p * hpp, m_lo, m_hi);
        else       acc = h_lds ? rs_dot<T>(xw + q, s_h + p * hpp, m_lo, m_hi) : rs_dot<T>(xw + q, h + p * hpp, m_lo, m_hi);
        const float v = (float)acc;
        for (int c = 0; c < rep; ++c) o[c * out_stride + k] = v;
        p += sp; q += sq; if (p >= up) { p -= up; ++q; }
    }
    __syncthreads();                                                        // the next item of this block restages the LDS
}

template <typename S>
__global__ __launch_bounds__(RS_THREADS) void es_resample_ragged_kernel(const S* __restrict__ pool, long long pool_n,
        const typename rs_compute<S>::type* __restrict__ filt, long long filt_n, const long long* __restrict__ desc, long long R, int rep,
        long long tiles_per_rec, float* __restrict__ out, long long out_stride)
{
    typedef typename rs_compute<S>::type T;
    __shared__ T s_x[RS_WIN_MAX];
    __shared__ T s_h[RS_FILT_MAX];
    const int tid = threadIdx.x;
    const long long items = R * tiles_per_rec;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long r = item / tiles_per_rec, tile = item - r * tiles_per_rec;
        const long long* d = desc + r * ES_RESAMPLE_DESC_WORDS;
        long long in_off = d[0], n_in = d[1];
        const long long up_l = d[2], down_l = d[3], h_off = d[4], hpp_l = d[5], y0 = d[6];
        long long n_out = d[7] < out_stride ? d[7] : out_stride;
        const long long k0 = tile * RS_TILE;
        if (k0 >= n_out) continue;                                          // a tile past its record's end leaves at once (block-uniform)
        // a bad descriptor reads nothing outside the pools: samples from the record's own [in_off, in_off + n_in) inside the pool only
        if (in_off < 0 || in_off > pool_n) { in_off = 0; n_in = 0; }
        if (n_in < 0) n_in = 0;
        if (n_in > pool_n - in_off) n_in = pool_n - in_off;
        const S* x = pool + in_off;
        float* o = out + (r * rep) * out_stride + k0;
        const int cnt = (int)(n_out - k0 < RS_TILE ? n_out - k0 : RS_TILE);     // outputs of this tile
        if (up_l == down_l) {                                               // identity: copied (int16 converted), never through the accumulator
            for (int k = tid; k < cnt; k += RS_THREADS) {
                if (k0 + k >= n_in) break;
                const float v = (float)rs_load(x + k0 + k);
                for (int c = 0; c < rep; ++c) o[c * out_stride + k] = v;
            }
            continue;
        }
        if (up_l < 1 || down_l < 1 || up_l > RS_RATE_MAX || down_l > RS_RATE_MAX || hpp_l < 1 || hpp_l > RS_RATE_MAX || y0 < 0 || h_off < 0 ||
            up_l * hpp_l > filt_n - h_off || up_l * hpp_l > (1ll << 30))
            continue;                                                       // no filter inside the pool: nothing is written
        rs_tile<T>((rs_lds<T>*)s_x, (rs_lds<T>*)s_h, tid, rs_clip<S>{x}, n_in, filt + h_off, (int)up_l, (int)down_l, (int)hpp_l, y0 + k0, cnt, o, rep,
                   out_stride);
    }
}

// ---- chunks of live streams at their own rates (es_resample_stream_batch) -------------------------------------------------
// Record r = the chunk x[r][0 : len[r]] of stream sid[r] of a table of S: rate[s] = (up, down, filter offset, hpp, y0), nin[s] = samples
// received before this chunk, tail[s] = the last 256 of them, newest last (+0.0 where there were fewer; the newest 255 are read).  The record's outputs are F(n_old) ..
// F(n_old + len) - 1 of resample_poly over the whole stream (es_rs_finalized): those whose newest input sample has now arrived.  One
// workgroup per (record, tile), rs_tile as above with the window read from tail and chunk.  Everything here is device data: a sid outside
// the table or rate words no filter fits is a record without outputs, len is cut to the chunk row, the count to the output row.
template <typename S>
__global__ __launch_bounds__(RS_THREADS) void es_resample_stream_kernel(const S* __restrict__ x, long long R, long long n_stride,
        const int64_t* __restrict__ sid, const int64_t* __restrict__ len, long long S_tab, const int64_t* __restrict__ rate,
        const float* __restrict__ filt, long long filt_n, const float* __restrict__ tail, const int64_t* __restrict__ nin,
        long long tiles_per_rec, float* __restrict__ out, long long out_stride)
{
    __shared__ float s_x[RS_WIN_MAX];
    __shared__ float s_h[RS_FILT_MAX];
    const int tid = threadIdx.x;
    const long long items = R * tiles_per_rec;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const long long r = item / tiles_per_rec, tile = item - r * tiles_per_rec;
        const long long s = sid[r];
        if (s < 0 || s >= S_tab) continue;                                  // (block-uniform, as every `continue` below)
        long long n = len[r];
        n = n < 0 ? 0 : (n > n_stride ? n_stride : n);
        const int64_t* w = rate + s * ES_RSTREAM_RATE_WORDS;
        const long long up_l = w[0], down_l = w[1], h_off = w[2], hpp_l = w[3], y0 = w[4], n_old = nin[s];
        if (n_old < 0) continue;
        const S* xr = x + r * n_stride;
        float* o = out + r * out_stride;
        const long long k0 = tile * RS_TILE;
        if (up_l == down_l) {                                               // a stream at the target rate: copied (int16 converted)
            const long long cnt = n < out_stride ? n : out_stride;
            for (long long k = k0 + tid; k < cnt && k < k0 + RS_TILE; k += RS_THREADS) o[k] = (float)rs_load(xr + k);
            continue;
        }
        if (up_l < 1 || down_l < 1 || up_l > RS_RATE_MAX || down_l > RS_RATE_MAX || hpp_l < 1 || hpp_l > ES_RSTREAM_TAIL || y0 < 0 ||
            y0 > ES_RSTREAM_Y0_MAX || h_off < 0 || up_l * hpp_l > filt_n - h_off || n_old > (1ll << 62) / up_l - n)
            continue;                                                       // no filter inside the pool, or a position whose n * up leaves 62 bits
        const long long f_old = es_rs_finalized(n_old, up_l, down_l, y0);
        long long n_out = es_rs_finalized(n_old + n, up_l, down_l, y0) - f_old;
        if (n_out > out_stride) n_out = out_stride;
        if (k0 >= n_out) continue;
        const int cnt = (int)(n_out - k0 < RS_TILE ? n_out - k0 : RS_TILE);
        rs_tile<float>((rs_lds<float>*)s_x, (rs_lds<float>*)s_h, tid, rs_stream<S>{tail + s * ES_RSTREAM_TAIL + ES_RSTREAM_TAIL, xr, n_old}, n_old + n,
                       filt + h_off, (int)up_l, (int)down_l, (int)hpp_l, y0 + f_old + k0, cnt, o + k0, 1, out_stride);
    }
}

// The state of the pushed streams after that launch: tail := the last of (tail ++ chunk as float32) -- the row holds ES_RSTREAM_TAIL = 256
// samples, of which the resample kernel reads the newest 255 --, the whole row read before any of it is written (a barrier); nin += len.
// One block of ES_RSTREAM_TAIL threads per record.
template <typename S>
__global__ __launch_bounds__(ES_RSTREAM_TAIL) void es_resample_commit_kernel(const S* __restrict__ x, long long R, long long n_stride,
        const int64_t* __restrict__ sid, const int64_t* __restrict__ len, long long S_tab, float* __restrict__ tail, int64_t* __restrict__ nin)
{
    const long long r = blockIdx.x;
    if (r >= R) return;                                                     // (block-uniform, as the two below)
    const long long s = sid[r];
    if (s < 0 || s >= S_tab) return;
    long long n = len[r];
    n = n < 0 ? 0 : (n > n_stride ? n_stride : n);
    if (n == 0) return;
    float* row = tail + s * ES_RSTREAM_TAIL;
    const long long j = (long long)threadIdx.x + n;                         // index into tail ++ chunk
    const float v = j < ES_RSTREAM_TAIL ? row[j] : (float)rs_load(x + r * n_stride + (j - ES_RSTREAM_TAIL));
    __syncthreads();
    row[threadIdx.x] = v;
    if (threadIdx.x == 0) nin[s] += n;
}

}  // namespace

int es_launch_resample(es_ctx* ctx, const void* x, int dtype, int64_t B, int64_t n_x, const void* h_tf, int hpp, int up, int down,
                       int64_t y0, int64_t n_out, void* out, hipStream_t st)
{
    const unsigned blocks = es_grid(B * n_out, 256, ctx->num_cu * 32);
    if (dtype == ES_DTYPE_F32)
        return es_launch(ctx, es_resample_kernel<float>, blocks, 256, 0, st, (const float*)x, (long long)B,
                         (long long)n_x, (const float*)h_tf, hpp, up, down, (long long)y0, (long long)n_out, (float*)out);
    return es_launch(ctx, es_resample_kernel<double>, blocks, 256, 0, st, (const double*)x, (long long)B,
                     (long long)n_x, (const double*)h_tf, hpp, up, down, (long long)y0, (long long)n_out, (double*)out);
}

int es_launch_resample_ragged(es_ctx* ctx, const es_resample_ragged_args& a, hipStream_t st)
{
    const long long tiles = (a.max_out + RS_TILE - 1) / RS_TILE;
    const unsigned blocks = es_grid(a.R * tiles, 1, 0x7fffffffll);
    if (a.dtype == ES_DTYPE_I16)
        return es_launch(ctx, es_resample_ragged_kernel<short>, blocks, RS_THREADS, 0, st, (const short*)a.pool, (long long)a.pool_n,
                         (const float*)a.filt, (long long)a.filt_n, (const long long*)a.desc, (long long)a.R, a.rep, tiles, a.out,
                         (long long)a.out_stride);
    if (a.dtype == ES_DTYPE_F32)
        return es_launch(ctx, es_resample_ragged_kernel<float>, blocks, RS_THREADS, 0, st, (const float*)a.pool, (long long)a.pool_n,
                         (const float*)a.filt, (long long)a.filt_n, (const long long*)a.desc, (long long)a.R, a.rep, tiles, a.out,
                         (long long)a.out_stride);
    return es_launch(ctx, es_resample_ragged_kernel<double>, blocks, RS_THREADS, 0, st, (const double*)a.pool, (long long)a.pool_n,
                     (const double*)a.filt, (long long)a.filt_n, (const long long*)a.desc, (long long)a.R, a.rep, tiles, a.out,
                     (long long)a.out_stride);
}

int es_launch_resample_stream(es_ctx* ctx, const es_resample_stream_args& a, hipStream_t st)
{
    const long long tiles = (a.max_out + RS_TILE - 1) / RS_TILE;
    const bool i16 = a.dtype == ES_DTYPE_I16;
    if (tiles > 0) {
        const unsigned blocks = es_grid(a.R * tiles, 1, 0x7fffffffll);
        const int rc = i16 ? es_launch(ctx, es_resample_stream_kernel<short>, blocks, RS_THREADS, 0, st, (const short*)a.x, (long long)a.R,
                                       (long long)a.n_stride, a.sid, a.len, (long long)a.S, a.rate, a.filt, (long long)a.filt_n, (const float*)a.tail,
                                       (const int64_t*)a.nin, tiles, a.out, (long long)a.out_stride)
                           : es_launch(ctx, es_resample_stream_kernel<float>, blocks, RS_THREADS, 0, st, (const float*)a.x, (long long)a.R,
                                       (long long)a.n_stride, a.sid, a.len, (long long)a.S, a.rate, a.filt, (long long)a.filt_n, (const float*)a.tail,
                                       (const int64_t*)a.nin, tiles, a.out, (long long)a.out_stride);
        if (rc != ES_OK) return rc;
    }
    if (i16)
        return es_launch(ctx, es_resample_commit_kernel<short>, (unsigned)a.R, ES_RSTREAM_TAIL, 0, st, (const short*)a.x, (long long)a.R,
                         (long long)a.n_stride, a.sid, a.len, (long long)a.S, a.tail, a.nin);
    return es_launch(ctx, es_resample_commit_kernel<float>, (unsigned)a.R, ES_RSTREAM_TAIL, 0, st, (const float*)a.x, (long long)a.R,
                     (long long)a.n_stride, a.sid, a.len, (long long)a.S, a.tail, a.nin);
}
