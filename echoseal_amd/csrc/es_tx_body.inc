// es_tx_body.inc -- the frame generator's symbol kernel, included twice by es_tx.hip: ES_KEYED 0 = es_tx_symbols_kernel (one header PN for
// the batch), ES_KEYED 1 = es_tx_symbols_keyed_kernel (frame f takes its header PN from ring row key[f], bytes 272..287; a key index
// outside [0, N) reads nothing of the ring and gives a header PN of zero bytes).
#if ES_KEYED
__global__ __launch_bounds__(256) void es_tx_symbols_keyed_kernel(const uint8_t* __restrict__ code, const uint8_t* __restrict__ pn_rows,
        const uint32_t* __restrict__ ctr, unsigned long long pre_bits, const uint8_t* __restrict__ ring, long long N,
        const int32_t* __restrict__ key_p, long long B, float* __restrict__ sym)
{
    __shared__ uint8_t hdr_pn[16];
#else
__global__ __launch_bounds__(256) void es_tx_symbols_kernel(const uint8_t* __restrict__ code, const uint8_t* __restrict__ pn_rows,
        const uint32_t* __restrict__ ctr, unsigned long long pre_bits, const uint8_t* __restrict__ hdr_pn_g, long long B,
        float* __restrict__ sym)
{
    __shared__ uint8_t hdr_pn[16];
    if (threadIdx.x < 16) hdr_pn[threadIdx.x] = hdr_pn_g[threadIdx.x];
    __syncthreads();
#endif
    for (long long f = blockIdx.x; f < B; f += gridDim.x) {
#if ES_KEYED
        const long long key = key_p[f];                                                   // block-uniform
        const bool have = key >= 0 && key < N;
        __syncthreads();                                                                  // the previous frame has read its header PN
        if (threadIdx.x < 16) hdr_pn[threadIdx.x] = have ? ring[key * ES_KEYRING_BYTES + ES_RING_HDR_PN + threadIdx.x] : (uint8_t)0;
        __syncthreads();
#endif
        const uint32_t lo16 = ctr[f] & 0xFFFFu;
        const uint8_t* pn = pn_rows + f * ES_PN_BYTES;
        for (int i = threadIdx.x; i < ES_FRAME_LEN; i += 256) {
            float v;
            if (i < ES_PRE_L) {
                v = ((pre_bits >> (63 - i)) & 1ull) ? 1.0f : -1.0f;                       // bit i of the packed MLS, MSB first
            } else if (i < ES_PRE_L + ES_HDR_L) {
                const int k = i - ES_PRE_L;
                const uint32_t hb = (lo16 >> (15 - (k >> 3))) & 1u;                       // 16 bits, each repeated 8 times
                const uint32_t pb = (hdr_pn[k >> 3] >> (7 - (k & 7))) & 1u;
                v = (hb ? 1.0f : -1.0f) * (pb ? 1.0f : -1.0f);
            } else {
                const int k = i - (ES_PRE_L + ES_HDR_L);
                const uint32_t pb = (pn[i >> 3] >> (7 - (i & 7))) & 1u;                   // PN bit 191 + k
                v = (code[f * ES_POLAR_N + k] ? 1.0f : -1.0f) * (pb ? 1.0f : -1.0f);
            }
            sym[f * ES_FRAME_LEN + i] = v;
        }
    }
}
