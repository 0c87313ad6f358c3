// es_seal_body.inc -- the sealing kernel, included twice by es_aead.hip: ES_KEYED 0 = es_aead_seal_kernel (one key, by value),
// ES_KEYED 1 = es_aead_seal_keyed_kernel (blob i under the ChaCha20 key of ring row key_dev[i]; a key index outside [0, N) reads
// nothing of the ring and writes a zero blob).
// SecureChannel.seal (rtwm/crypto.py:33-37): blob = nonce 12 | ChaCha20(counter 1) xor plaintext 27 | Poly1305 tag 16
#if ES_KEYED
__global__ __launch_bounds__(256) void es_aead_seal_keyed_kernel(const uint8_t* __restrict__ ring, long long N,
        const int32_t* __restrict__ key_dev, const uint8_t* __restrict__ nonces, const uint8_t* __restrict__ plain, long long n,
        uint8_t* __restrict__ blobs)
#else
__global__ __launch_bounds__(256) void es_aead_seal_kernel(AeadKey key, const uint8_t* __restrict__ nonces,
        const uint8_t* __restrict__ plain, long long n, uint8_t* __restrict__ blobs)
#endif
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
#if ES_KEYED
        AeadKey key;
        if (!ring_aead_key(ring, N, key_dev, i, key)) {
            for (int b = 0; b < ES_INFO_BYTES; ++b) blobs[i * ES_INFO_BYTES + b] = 0;
            continue;
        }
#endif
        const uint8_t* nb = nonces + i * 12;
        const uint8_t* pb = plain + i * 27;
        uint32_t nonce[3], pt[8];
        #pragma unroll
        for (int w = 0; w < 3; ++w) nonce[w] = (uint32_t)nb[4 * w] | ((uint32_t)nb[4 * w + 1] << 8) | ((uint32_t)nb[4 * w + 2] << 16) | ((uint32_t)nb[4 * w + 3] << 24);
        #pragma unroll
        for (int w = 0; w < 8; ++w) {
            uint32_t v = 0;
            #pragma unroll
            for (int b = 0; b < 4; ++b) { const int o = 4 * w + b; if (o < 27) v |= (uint32_t)pb[o] << (8 * b); }
            pt[w] = v;
        }
        uint32_t ks[16], ct[8];
        chacha20_block(key, 1, nonce, ks);
        #pragma unroll
        for (int w = 0; w < 7; ++w) ct[w] = pt[w] ^ ks[w];
        ct[6] &= 0x00ffffffu; ct[7] = 0;
        chacha20_block(key, 0, nonce, ks);
        Poly P; P.init(ks);
        P.block(ct); P.block(ct + 4);
        const uint32_t lens[4] = {0u, 0u, 27u, 0u};
        P.block(lens);
        uint32_t tag[4];
        P.finish(ks, tag);
        uint8_t* out = blobs + i * ES_INFO_BYTES;
        for (int b = 0; b < 12; ++b) out[b] = nb[b];
        for (int b = 0; b < 27; ++b) out[12 + b] = (uint8_t)(ct[b >> 2] >> (8 * (b & 3)));
        for (int b = 0; b < 16; ++b) out[39 + b] = (uint8_t)(tag[b >> 2] >> (8 * (b & 3)));
    }
}
