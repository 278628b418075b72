/*
 * quic_keys.h -- the arithmetic of QUIC key derivation (RFC 9001 §5.1, §5.2, §6; RFC 9369 §3.3), written for host and
 * device: quic_keys.hip runs exactly these functions with one thread per connection (or per side of a connection),
 * keyset.cpp hashes the Initial salt's pads with them on the host, and tests/test_quic_keys_native.py compiles them with
 * g++ and checks them against Python's hmac / hashlib.
 *
 *   SHA-256 / SHA-384 block functions (FIPS 180-4), the message schedule as 16 words under compile-time indices
 *   HMAC with a cached pad state (RFC 2104): the inner and outer state after the key block, hashed once per key
 *   HKDF-Extract and HKDF-Expand-Label (RFC 5869, RFC 8446 §7.1) as picotls computes them (ptls_hkdf_extract,
 *     ptls_hkdf_expand_label, lib/picotls.c): with L <= Nh an Expand-Label is ONE HMAC over
 *     BE16(L) || u8(6 + |label|) || "tls13 " || label || u8(0) || u8(1), which fits one block of either hash
 *   the per-connection routines: keys from a traffic secret (with or without the key update), keys of one side from a
 *     Destination Connection ID
 *
 * Digests stay in words from one HMAC to the next (a digest is the next key block's leading words as it stands), the labels
 * are compile-time tables of words, and no byte array is indexed at run time.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

/* the function qualifier shared with gf128.h, chacha20.h and quic.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define HKDF_FN GF128_FN

namespace ptls_hip {

/* ---------------- the two hashes ---------------- */

/* SHA-256 (FIPS 180-4 §6.2): 32-bit words, 64-byte blocks */
struct HkSha256 {
    typedef uint32_t word;
    static constexpr int WORD_BYTES = 4, BLOCK_BYTES = 64, DIGEST_BYTES = 32, DIGEST_WORDS = 8;
};

/* (the functions of a hash are overloads on its tag type, not members: the qualifier may itself say `static`) */
HKDF_FN uint32_t hk_ror(uint32_t x, int n)
{
    return (x >> n) | (x << (32 - n));
}

HKDF_FN void hk_init(HkSha256, uint32_t h[8])
{
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
}

/* h absorbs one block given as 16 big-endian words; w is consumed */
HKDF_FN void hk_compress(HkSha256, uint32_t h[8], uint32_t w[16])
{
    typedef uint32_t word;
    static constexpr word K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
        0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
        0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
        0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
        0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
        0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    word a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        if (i >= 16) {
            const word w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (hk_ror(w15, 7) ^ hk_ror(w15, 18) ^ (w15 >> 3)) + w[(i + 9) & 15] + (hk_ror(w2, 17) ^ hk_ror(w2, 19) ^ (w2 >> 10));
        }
        const word t1 = k + (hk_ror(e, 6) ^ hk_ror(e, 11) ^ hk_ror(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const word t2 = (hk_ror(a, 2) ^ hk_ror(a, 13) ^ hk_ror(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        k = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += k;
}

/* SHA-384 = SHA-512 with its own initial value, the first six words of the state (FIPS 180-4 §6.4, §6.5): 64-bit words,
 * 128-byte blocks */
struct HkSha384 {
    typedef uint64_t word;
    static constexpr int WORD_BYTES = 8, BLOCK_BYTES = 128, DIGEST_BYTES = 48, DIGEST_WORDS = 6;
};

HKDF_FN uint64_t hk_ror(uint64_t x, int n)
{
    return (x >> n) | (x << (64 - n));
}

HKDF_FN void hk_init(HkSha384, uint64_t h[8])
{
    h[0] = 0xcbbb9d5dc1059ed8ull, h[1] = 0x629a292a367cd507ull, h[2] = 0x9159015a3070dd17ull, h[3] = 0x152fecd8f70e5939ull;
    h[4] = 0x67332667ffc00b31ull, h[5] = 0x8eb44a8768581511ull, h[6] = 0xdb0c2e0d64f98fa7ull, h[7] = 0x47b5481dbefa4fa4ull;
}

HKDF_FN void hk_compress(HkSha384, uint64_t h[8], uint64_t w[16])
{
    typedef uint64_t word;
    static constexpr word K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
        0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
        0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
        0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
        0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
        0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
        0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    word a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], k = h[7];
#pragma unroll
    for (int i = 0; i < 80; ++i) {
        if (i >= 16) {
            const word w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            w[i & 15] += (hk_ror(w15, 1) ^ hk_ror(w15, 8) ^ (w15 >> 7)) + w[(i + 9) & 15] + (hk_ror(w2, 19) ^ hk_ror(w2, 61) ^ (w2 >> 6));
        }
        const word t1 = k + (hk_ror(e, 14) ^ hk_ror(e, 18) ^ hk_ror(e, 41)) + ((e & f) ^ (~e & g)) + K[i] + w[i & 15];
        const word t2 = (hk_ror(a, 28) ^ hk_ror(a, 34) ^ hk_ror(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
        k = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += k;
}

/* ---------------- HMAC with a cached pad state (RFC 2104) ---------------- */

/* the hash state after the block key ^ ipad and after the block key ^ opad: every HMAC under the key starts from them */
template <class H> struct HkPads {
    typename H::word in[8], out[8];
};

/* key = the DIGEST_WORDS leading words of the key block, the rest of the block zero (a digest used as the next key) */
template <class H> HKDF_FN void hk_hmac_key(HkPads<H> &p, const typename H::word key[8])
{
    typedef typename H::word word;
    const word ipad = (word)0x3636363636363636ull, opad = (word)0x5c5c5c5c5c5c5c5cull;
    word w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        w[i] = (i < H::DIGEST_WORDS ? key[i] : 0) ^ ipad;
    hk_init(H(), p.in);
    hk_compress(H(), p.in, w);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        w[i] = (i < H::DIGEST_WORDS ? key[i] : 0) ^ opad;
    hk_init(H(), p.out);
    hk_compress(H(), p.out, w);
}

/* HMAC of a message of one block: w = the message with its 0x80 terminator, zero-filled; msg_len (<= BLOCK_BYTES - 1 -
 * 2 * WORD_BYTES) goes into the length word here.  w is consumed; the digest is out[0 .. DIGEST_WORDS). */
template <class H> HKDF_FN void hk_hmac_block(const HkPads<H> &p, typename H::word w[16], uint32_t msg_len, typename H::word out[8])
{
    typedef typename H::word word;
    word hi[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        hi[i] = p.in[i], out[i] = p.out[i];
    w[15] = (word)(8u * ((uint32_t)H::BLOCK_BYTES + msg_len));
    hk_compress(H(), hi, w);
#pragma unroll
    for (int i = 0; i < 15; ++i)
        w[i] = i < H::DIGEST_WORDS ? hi[i] : i == H::DIGEST_WORDS ? (word)1 << (8 * H::WORD_BYTES - 1) : 0;
    w[15] = (word)(8u * (uint32_t)(H::BLOCK_BYTES + H::DIGEST_BYTES));
    hk_compress(H(), out, w);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        hi[i] = 0;
}

/* ---------------- HKDF-Expand-Label ---------------- */

/* an Expand-Label message as words: BE16(0) || u8(6 + |label|) || "tls13 " || label || u8(0) || u8(1) || 0x80, big-endian,
 * zero-filled; n = its bytes without the terminator.  The output length is added by the caller (hk_expand_label). */
struct HkLabel {
    uint32_t w[6];
    uint32_t n;
};
constexpr int HK_LABEL_MAX = 12; /* 2 + 1 + 6 + 12 + 1 + 1 + 1 (the terminator) = the 24 bytes of w */

constexpr HkLabel hk_make_label(const char *label)
{
    uint8_t b[24] = {};
    int len = 0;
    while (label[len] != 0)
        ++len;
    int n = 2;
    b[n++] = (uint8_t)(6 + len);
    const char prefix[6] = {'t', 'l', 's', '1', '3', ' '};
    for (int i = 0; i < 6; ++i)
        b[n++] = (uint8_t)prefix[i];
    for (int i = 0; i < len && i < HK_LABEL_MAX; ++i)
        b[n++] = (uint8_t)label[i];
    b[n++] = 0; /* empty context */
    b[n++] = 1; /* HKDF-Expand counter T(1) */
    b[n] = 0x80;
    HkLabel r = {};
    for (int i = 0; i < 6; ++i)
        r.w[i] = (uint32_t)b[4 * i] << 24 | (uint32_t)b[4 * i + 1] << 16 | (uint32_t)b[4 * i + 2] << 8 | b[4 * i + 3];
    r.n = (uint32_t)n;
    return r;
}

/* the labels of the derivations below: index 0 = the step that replaces the secret, 1..3 = key, iv, hp */
enum { HK_STEP_SECRET = 0, HK_STEP_KEY = 1, HK_STEP_IV = 2, HK_STEP_HP = 3 };
/* the first step of a derivation: none, the key update ("<p> ku"), or the Initial secret of one side */
enum { HK_FIRST_NONE = 0, HK_FIRST_KU = 1, HK_FIRST_CLIENT = 2, HK_FIRST_SERVER = 3 };

/* label of step `step`; v2 != 0: the "quicv2 " prefix of RFC 9369 (the Initial "client in" / "server in" have no prefix) */
HKDF_FN HkLabel hk_quic_label(int v2, int first, int step)
{
    static constexpr HkLabel T[2][4] = {
        {hk_make_label("quic ku"), hk_make_label("quic key"), hk_make_label("quic iv"), hk_make_label("quic hp")},
        {hk_make_label("quicv2 ku"), hk_make_label("quicv2 key"), hk_make_label("quicv2 iv"), hk_make_label("quicv2 hp")}};
    static constexpr HkLabel IN[2] = {hk_make_label("client in"), hk_make_label("server in")};
    if (step == HK_STEP_SECRET && first >= HK_FIRST_CLIENT)
        return IN[first - HK_FIRST_CLIENT];
    return T[v2 != 0 ? 1 : 0][step];
}

/* out[0 .. DIGEST_WORDS) = HKDF-Expand-Label(key of p, label, "", outlen); the caller uses the leading outlen bytes */
template <class H> HKDF_FN void hk_expand_label(const HkPads<H> &p, const HkLabel &l, uint32_t outlen, typename H::word out[8])
{
    typedef typename H::word word;
    word w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        w[i] = 0;
    const uint32_t w0 = l.w[0] | outlen << 16;
    if (H::WORD_BYTES == 4) {
        w[0] = (word)w0;
#pragma unroll
        for (int i = 1; i < 6; ++i)
            w[i] = (word)l.w[i];
    } else {
        w[0] = (word)((uint64_t)w0 << 32 | l.w[1]);
        w[1] = (word)((uint64_t)l.w[2] << 32 | l.w[3]);
        w[2] = (word)((uint64_t)l.w[4] << 32 | l.w[5]);
    }
    hk_hmac_block<H>(p, w, l.n, out);
}

/* ---------------- bytes <-> words (compile-time word indices) ---------------- */

/* a digest's DIGEST_WORDS words from its DIGEST_BYTES big-endian bytes */
template <class H> HKDF_FN void hk_load(typename H::word h[8], const uint8_t *src)
{
    typedef typename H::word word;
#pragma unroll
    for (int i = 0; i < H::DIGEST_WORDS; ++i) {
        word v = 0;
#pragma unroll
        for (int j = 0; j < H::WORD_BYTES; ++j)
            v = (word)(v << 8) | src[H::WORD_BYTES * i + j];
        h[i] = v;
    }
}

/* the leading nbytes (at most DIGEST_BYTES) of a digest to dst */
template <class H> HKDF_FN void hk_store(uint8_t *dst, const typename H::word h[8], uint32_t nbytes)
{
#pragma unroll
    for (int j = 0; j < H::DIGEST_BYTES; ++j)
        if ((uint32_t)j < nbytes)
            dst[j] = (uint8_t)(h[j / H::WORD_BYTES] >> (8 * (H::WORD_BYTES - 1 - j % H::WORD_BYTES)));
}

/* ---------------- per connection ---------------- */

/* The keys of one traffic secret (words in `secret`, which is consumed and zeroed).
 *   first == HK_FIRST_NONE:   key / iv / hp = Expand-Label(secret, "<p> key" / "<p> iv" / "<p> hp")   (RFC 9001 §5.1)
 *   first == HK_FIRST_KU:     secret = Expand-Label(secret, "<p> ku", "", Nh) first (§6); it goes to secret_out
 *   first == HK_FIRST_CLIENT / _SERVER: secret = Expand-Label(secret, "client in" / "server in", "", Nh) first (§5.2)
 * with <p> = "quic" or, v2 != 0, "quicv2".  key and hp get key_size bytes, iv 12; secret_out (Nh bytes), hp may be null.
 * The pads of a secret are hashed once and serve every label under it: 2 + 2 * labels compression calls per secret.  The
 * steps run as one loop (not unrolled), so the kernel holds each of the four compression calls once. */
template <class H>
HKDF_FN void hk_quic_keys(typename H::word secret[8], int first, int v2, uint32_t key_size, uint8_t *secret_out, uint8_t *key,
                          uint8_t *iv, uint8_t *hp)
{
    typedef typename H::word word;
    HkPads<H> p;
#pragma unroll 1
    for (int step = first != HK_FIRST_NONE ? HK_STEP_SECRET : HK_STEP_KEY; step <= HK_STEP_HP; ++step) {
        if (step <= HK_STEP_KEY)
            hk_hmac_key<H>(p, secret); /* the secret as it came, or the one step 0 has just made */
        const uint32_t outlen = step == HK_STEP_SECRET ? (uint32_t)H::DIGEST_BYTES : step == HK_STEP_IV ? 12u : key_size;
        word out[8];
        hk_expand_label<H>(p, hk_quic_label(v2, first, step), outlen, out);
        if (step == HK_STEP_SECRET) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                secret[i] = out[i];
            if (secret_out != nullptr)
                hk_store<H>(secret_out, out, (uint32_t)H::DIGEST_BYTES);
        } else {
            uint8_t *dst = step == HK_STEP_KEY ? key : step == HK_STEP_IV ? iv : hp;
            if (dst != nullptr)
                hk_store<H>(dst, out, outlen);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            out[i] = 0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        secret[i] = 0, p.in[i] = 0, p.out[i] = 0;
}

/* the same from a secret of DIGEST_BYTES bytes */
template <class H>
HKDF_FN void hk_quic_keys_from_secret(const uint8_t *secret, int update, int v2, uint32_t key_size, uint8_t *secret_out,
                                      uint8_t *key, uint8_t *iv, uint8_t *hp)
{
    typename H::word s[8] = {};
    hk_load<H>(s, secret);
    hk_quic_keys<H>(s, update ? HK_FIRST_KU : HK_FIRST_NONE, v2, key_size, secret_out, key, iv, hp);
}

constexpr uint32_t HK_DCID_STRIDE = 20; /* RFC 9000 §17.2: a connection ID is at most 20 bytes */
constexpr size_t HK_SALT_MAX = 64;      /* an HMAC key of up to one SHA-256 block is used as it stands */

/* The pads of the Initial salt (salt_len <= HK_SALT_MAX), the HMAC key of every connection's HKDF-Extract: hashed once per
 * call, on the host.  (Indexes the salt at run time: not for a kernel.) */
inline void hk_salt_pads(HkPads<HkSha256> &p, const uint8_t *salt, size_t salt_len)
{
    uint32_t wi[16], wo[16];
    for (int i = 0; i < 16; ++i) {
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j)
            v = v << 8 | ((size_t)(4 * i + j) < salt_len ? salt[4 * i + j] : 0u);
        wi[i] = v ^ 0x36363636u;
        wo[i] = v ^ 0x5c5c5c5cu;
    }
    hk_init(HkSha256(), p.in);
    hk_compress(HkSha256(), p.in, wi);
    hk_init(HkSha256(), p.out);
    hk_compress(HkSha256(), p.out, wo);
}

/* The Initial keys of one side of one connection (RFC 9001 §5.2; always AES-128-GCM with SHA-256):
 * initial = HKDF-Extract(salt, dcid), then as hk_quic_keys with "client in" (server == 0) or "server in".  dcid points at
 * HK_DCID_STRIDE readable bytes of which the leading dcid_len (<= 20) are the connection ID. */
HKDF_FN void hk_quic_initial_keys(const HkPads<HkSha256> &salt, const uint8_t *dcid, uint32_t dcid_len, int server, int v2,
                                  uint8_t *key, uint8_t *iv, uint8_t *hp)
{
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        w[i] = 0;
#pragma unroll
    for (int j = 0; j <= (int)HK_DCID_STRIDE; ++j) { /* byte j of the block: the ID, then the terminator */
        const uint32_t b = (uint32_t)j < dcid_len ? (uint32_t)dcid[j < (int)HK_DCID_STRIDE ? j : 0] : (uint32_t)j == dcid_len ? 0x80u : 0u;
        w[j / 4] |= b << (8 * (3 - j % 4));
    }
    uint32_t initial[8];
    hk_hmac_block<HkSha256>(salt, w, dcid_len, initial); /* HKDF-Extract = HMAC(salt, ikm) */
    hk_quic_keys<HkSha256>(initial, server ? HK_FIRST_SERVER : HK_FIRST_CLIENT, v2, 16, nullptr, key, iv, hp);
}

} // namespace ptls_hip
