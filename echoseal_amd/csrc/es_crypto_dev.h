// es_crypto_dev.h -- the integer primitives of the key / PN / hop schedule, shared by es_sched.hip (one key per launch, expanded on
// the host) and es_keyring.hip (keys as device data): SHA-256 compression (FIPS 180-4), the AES-128 block (FIPS 197) and the one
// BLAKE2s compression (RFC 7693) that turns the PRNG seed into the AES sub-key.  Device code only.  Every array index is a
// compile-time constant after unrolling, so message schedules and states stay in registers (no private memory).
#ifndef ES_CRYPTO_DEV_H
#define ES_CRYPTO_DEV_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __attribute__((address_space(3))) const uint8_t es_lds_cu8;

__device__ __forceinline__ uint32_t ror32(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

__constant__ uint32_t c_K256[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

__constant__ uint32_t c_IV256[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};

#define ES_SHA_ROUND(kw)                                                                                                  \
    {                                                                                                                     \
        const uint32_t t1 = h + (ror32(e, 6) ^ ror32(e, 11) ^ ror32(e, 25)) + ((e & f) ^ (~e & g)) + (kw);                \
        const uint32_t t2 = (ror32(a, 2) ^ ror32(a, 13) ^ ror32(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));                  \
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;                                                \
    }

// one block: w[16] = the big-endian message words (clobbered).  Sixteen rounds at a time are unrolled, so w[] is indexed by constants.
__device__ __forceinline__ void sha256_compress(uint32_t st[8], uint32_t w[16])
{
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    #pragma unroll
    for (int i = 0; i < 16; ++i) ES_SHA_ROUND(c_K256[i] + w[i])
    #pragma unroll 1
    for (int o = 16; o < 64; o += 16) {
        #pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint32_t s0 = ror32(w15, 7) ^ ror32(w15, 18) ^ (w15 >> 3);
            const uint32_t s1 = ror32(w2, 17) ^ ror32(w2, 19) ^ (w2 >> 10);
            w[i] = w[i] + s0 + w[(i + 9) & 15] + s1;
            ES_SHA_ROUND(c_K256[o + i] + w[i])
        }
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

// HMAC-SHA256 of a message that fits one block after each pad block: w[0 .. msg_words) = the message (big-endian words, whole words
// only), from the states after the inner / outer pad blocks -> tag words in out[8].
__device__ __forceinline__ void hmac256_short(const uint32_t ipad[8], const uint32_t opad[8], uint32_t w[16], int msg_words, uint32_t out[8])
{
    uint32_t st[8];
    #pragma unroll
    for (int t = 0; t < 8; ++t) st[t] = ipad[t];
    #pragma unroll
    for (int t = 0; t < 15; ++t) if (t == msg_words) w[t] = 0x80000000u; else if (t > msg_words) w[t] = 0;
    w[15] = (uint32_t)(64 + 4 * msg_words) * 8;
    sha256_compress(st, w);
    #pragma unroll
    for (int t = 0; t < 8; ++t) w[t] = st[t];
    w[8] = 0x80000000u;
    #pragma unroll
    for (int t = 9; t < 15; ++t) w[t] = 0;
    w[15] = (64 + 32) * 8;
    #pragma unroll
    for (int t = 0; t < 8; ++t) out[t] = opad[t];
    sha256_compress(out, w);
}

__device__ __forceinline__ uint32_t xtime4(uint32_t x)      // xtime on four packed bytes
{
    return ((x & 0x7f7f7f7fu) << 1) ^ (((x >> 7) & 0x01010101u) * 0x1bu);
}

// One AES-128 block.  Columns are big-endian words: byte (row 0) in bits 31..24.  rk = the 44 round-key words (any indexable
// object: kernel arguments, or a per-lane register array with ROUNDS_UNROLLED = 10 so that it is indexed by constants),
// sbox = the S-box in LDS.
template <int ROUNDS_UNROLLED, typename RK, typename SB>
__device__ __forceinline__ void aes128_encrypt(const RK& rk, SB sbox, uint32_t s[4])
{
    #pragma unroll
    for (int c = 0; c < 4; ++c) s[c] ^= rk[c];
    #pragma unroll ROUNDS_UNROLLED
    for (int r = 1; r <= 10; ++r) {
        uint32_t t[4];
        #pragma unroll
        for (int c = 0; c < 4; ++c) {                              // SubBytes + ShiftRows
            t[c] = ((uint32_t)sbox[s[c] >> 24] << 24) | ((uint32_t)sbox[(s[(c + 1) & 3] >> 16) & 255] << 16) |
                   ((uint32_t)sbox[(s[(c + 2) & 3] >> 8) & 255] << 8) | (uint32_t)sbox[s[(c + 3) & 3] & 255];
        }
        if (r < 10) {
            #pragma unroll
            for (int c = 0; c < 4; ++c) {                          // MixColumns on a packed column
                const uint32_t a = t[c], x2 = xtime4(a);
                const uint32_t x3 = x2 ^ a;
                // out_row_i = 2 a_i ^ 3 a_{i+1} ^ a_{i+2} ^ a_{i+3}; rotating left by 8 brings a_{i+1} to row i
                t[c] = x2 ^ ((x3 << 8) | (x3 >> 24)) ^ ((a << 16) | (a >> 16)) ^ ((a << 24) | (a >> 8));
            }
        }
        #pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = t[c] ^ rk[4 * r + c];
    }
}

// AES-128 key expansion of the big-endian key words rk[0..3] into rk[4..43] (FIPS 197 5.2), unrolled: rk stays in registers.
template <typename SB>
__device__ __forceinline__ void aes128_expand(uint32_t rk[44], SB sbox)
{
    uint32_t rcon = 1;
    #pragma unroll
    for (int i = 4; i < 44; ++i) {
        uint32_t t = rk[i - 1];
        if ((i & 3) == 0) {
            t = (t << 8) | (t >> 24);                              // RotWord, then SubWord and the round constant
            t = ((uint32_t)sbox[t >> 24] << 24) | ((uint32_t)sbox[(t >> 16) & 255] << 16) | ((uint32_t)sbox[(t >> 8) & 255] << 8) | (uint32_t)sbox[t & 255];
            t ^= rcon << 24;
            rcon = ((rcon << 1) ^ ((rcon >> 7) * 0x1bu)) & 255u;
        }
        rk[i] = rk[i - 4] ^ t;
    }
}

#define ES_B2_G(a, b, c, d, x, y)                     \
    a = a + b + (x); d = ror32(d ^ a, 16);            \
    c = c + d;       b = ror32(b ^ c, 12);            \
    a = a + b + (y); d = ror32(d ^ a, 8);             \
    c = c + d;       b = ror32(b ^ c, 7);
#define ES_B2_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15)                     \
    ES_B2_G(v[0], v[4], v[8], v[12], m[s0], m[s1])   ES_B2_G(v[1], v[5], v[9], v[13], m[s2], m[s3])           \
    ES_B2_G(v[2], v[6], v[10], v[14], m[s4], m[s5])  ES_B2_G(v[3], v[7], v[11], v[15], m[s6], m[s7])          \
    ES_B2_G(v[0], v[5], v[10], v[15], m[s8], m[s9])  ES_B2_G(v[1], v[6], v[11], v[12], m[s10], m[s11])        \
    ES_B2_G(v[2], v[7], v[8], v[13], m[s12], m[s13]) ES_B2_G(v[3], v[4], v[9], v[14], m[s14], m[s15])

// hashlib.blake2s(seed32, digest_size=16, person=b"EchoSeal").digest() as four little-endian words: unkeyed, sequential mode,
// one (final) compression of the 32-byte input; the 8-byte personalisation is words 6, 7 of the parameter block (RFC 7693 2.5, 3.2).
__device__ __forceinline__ void blake2s_sub_key(const uint32_t seed_le[8], uint32_t out_le[4])
{
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    uint32_t hs[8], v[16], m[16];
    #pragma unroll
    for (int i = 0; i < 8; ++i) hs[i] = iv[i];
    hs[0] ^= 0x01010000u | 16u;                                    // digest 16 bytes, no key, fanout 1, depth 1
    hs[6] ^= 0x6f686345u;                                          // "Echo"
    hs[7] ^= 0x6c616553u;                                          // "Seal"
    #pragma unroll
    for (int i = 0; i < 8; ++i) { m[i] = seed_le[i]; m[8 + i] = 0; v[i] = hs[i]; v[8 + i] = iv[i]; }
    v[12] ^= 32u;                                                  // bytes hashed so far
    v[14] ^= 0xFFFFFFFFu;                                          // last block
    ES_B2_ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
    ES_B2_ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
    ES_B2_ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
    ES_B2_ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
    ES_B2_ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
    ES_B2_ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
    ES_B2_ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
    ES_B2_ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
    ES_B2_ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
    ES_B2_ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
    #pragma unroll
    for (int i = 0; i < 4; ++i) out_le[i] = hs[i] ^ v[i] ^ v[8 + i];
}

}  // namespace
#endif
