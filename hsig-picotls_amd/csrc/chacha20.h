/*
 * chacha20.h -- the ChaCha20 block function of RFC 8439 §2.3 (20 rounds, 32-bit block counter, 96-bit nonce), written for
 * host and device: chacha_kernel.hip runs exactly this function, and tests/test_chacha_poly_native.py compiles it on the
 * host and checks it against the RFC's vectors.  The state lives in sixteen named words, never in an array a lane could
 * index at run time (that would be scratch memory on the GPU).
 */
#pragma once

#include <stdint.h>

/* the function qualifier shared with gf128.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define CHACHA_FN GF128_FN

namespace ptls_hip {

/* a ChaCha20 state or one 64-byte keystream block: word i = bytes 4i .. 4i + 3, little-endian */
struct ChaChaBlock {
    uint32_t x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11, x12, x13, x14, x15;
};

/* key (8 little-endian words) and nonce (3 little-endian words) of one ChaCha20 context */
struct ChaChaKey {
    uint32_t k0, k1, k2, k3, k4, k5, k6, k7;
    uint32_t n0, n1, n2;
};

CHACHA_FN uint32_t chacha_rotl(uint32_t v, int n)
{
    return (v << n) | (v >> (32 - n));
}

#define PTLS_HIP_CHACHA_QR(a, b, c, d)                                                                                             \
    do {                                                                                                                           \
        a += b;                                                                                                                    \
        d = chacha_rotl(d ^ a, 16);                                                                                                \
        c += d;                                                                                                                    \
        b = chacha_rotl(b ^ c, 12);                                                                                                \
        a += b;                                                                                                                    \
        d = chacha_rotl(d ^ a, 8);                                                                                                 \
        c += d;                                                                                                                    \
        b = chacha_rotl(b ^ c, 7);                                                                                                 \
    } while (0)

/* keystream block `counter` of (key, nonce): RFC 8439 §2.3.1 */
CHACHA_FN ChaChaBlock chacha20_block(const ChaChaKey &k, uint32_t counter)
{
    const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;
    ChaChaBlock s{c0, c1, c2, c3, k.k0, k.k1, k.k2, k.k3, k.k4, k.k5, k.k6, k.k7, counter, k.n0, k.n1, k.n2};
#pragma unroll 1 /* ten double rounds as a loop: unrolled, every call site would carry about a thousand instructions */
    for (int i = 0; i < 10; ++i) {
        PTLS_HIP_CHACHA_QR(s.x0, s.x4, s.x8, s.x12);
        PTLS_HIP_CHACHA_QR(s.x1, s.x5, s.x9, s.x13);
        PTLS_HIP_CHACHA_QR(s.x2, s.x6, s.x10, s.x14);
        PTLS_HIP_CHACHA_QR(s.x3, s.x7, s.x11, s.x15);
        PTLS_HIP_CHACHA_QR(s.x0, s.x5, s.x10, s.x15);
        PTLS_HIP_CHACHA_QR(s.x1, s.x6, s.x11, s.x12);
        PTLS_HIP_CHACHA_QR(s.x2, s.x7, s.x8, s.x13);
        PTLS_HIP_CHACHA_QR(s.x3, s.x4, s.x9, s.x14);
    }
    return ChaChaBlock{s.x0 + c0,    s.x1 + c1,    s.x2 + c2,    s.x3 + c3,    s.x4 + k.k0,  s.x5 + k.k1,
                       s.x6 + k.k2,  s.x7 + k.k3,  s.x8 + k.k4,  s.x9 + k.k5,  s.x10 + k.k6, s.x11 + k.k7,
                       s.x12 + counter, s.x13 + k.n0, s.x14 + k.n1, s.x15 + k.n2};
}

#undef PTLS_HIP_CHACHA_QR

/* picotls's per-record nonce (ptls_aead__build_iv, lib/picotls.c:6492-6506): the static IV with bytes 4..11 XORed with the
 * big-endian sequence number.  iv0..iv2 are the IV's little-endian words. */
CHACHA_FN void chacha_nonce(ChaChaKey &k, uint32_t iv0, uint32_t iv1, uint32_t iv2, uint64_t seq)
{
    const uint32_t hi = (uint32_t)(seq >> 32), lo = (uint32_t)seq;
    k.n0 = iv0;
    k.n1 = iv1 ^ ((hi >> 24) | ((hi >> 8) & 0xff00u) | ((hi << 8) & 0xff0000u) | (hi << 24));
    k.n2 = iv2 ^ ((lo >> 24) | ((lo >> 8) & 0xff00u) | ((lo << 8) & 0xff0000u) | (lo << 24));
}

} // namespace ptls_hip
