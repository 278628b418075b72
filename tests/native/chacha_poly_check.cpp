// Host check of csrc/chacha20.h and csrc/poly1305.h (tests/test_chacha_poly_native.py): the functions chacha_kernel.hip
// runs, compiled with g++.  The RFC 8439 §2.3.2 block, every Poly1305 vector of Appendix A.3 (#1 - #11: the only inputs
// that reach an accumulator >= p, all-ones carry chains and the clamp), and the (r, s, message, tag) triples of the data file
// given as argv[1], folded serially and through the kernel's lane split for G = 1, 4, 16, 64.
// File: records of r[16] s[16] len[u32 LE] msg[len] tag[16].  Prints "ok <n>" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define GF128_FN static inline
#include "chacha20.h"
#include "poly1305.h"
using namespace ptls_hip;

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static Poly block_of(const uint8_t *p, size_t n)  // n = 16: a whole block; n < 16: the final block's 0x01 rule
{
    uint8_t b[16] = {0};
    memcpy(b, p, n);
    if (n < 16)
        b[n] = 1;
    return poly_limbs(le32(b), le32(b + 4), le32(b + 8), le32(b + 12), n == 16 ? 1 : 0);
}

static void finish(Poly acc, const uint8_t *s, uint8_t tag[16])
{
    uint32_t t[4];
    poly_finish(acc, le32(s), le32(s + 4), le32(s + 8), le32(s + 12), t[0], t[1], t[2], t[3]);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            tag[4 * i + j] = (uint8_t)(t[i] >> (8 * j));
}

static void mac_serial(const uint8_t *r, const uint8_t *s, const uint8_t *m, size_t len, uint8_t tag[16])
{
    const Poly r1 = poly_clamp_r(le32(r), le32(r + 4), le32(r + 8), le32(r + 12));
    Poly acc = poly_zero();
    for (size_t o = 0; o < len; o += 16)
        acc = poly_step(acc, block_of(m + o, len - o < 16 ? len - o : 16), r1);
    finish(acc, s, tag);
}

// the kernel's split: the first `pre` whole blocks play the AAD, then whole 64-byte chunks over G lanes, then the rest serially
static void mac_lanes(int G, int log2g, size_t pre, const uint8_t *r, const uint8_t *s, const uint8_t *m, size_t len, uint8_t tag[16])
{
    const Poly r1 = poly_clamp_r(le32(r), le32(r + 4), le32(r + 8), le32(r + 12));
    const Poly r2 = poly_mul(r1, r1), r3 = poly_mul(r2, r1), r4 = poly_mul(r2, r2);
    Poly rG = r4;
    for (int b = 0; b < log2g; ++b)
        rG = poly_mul(rG, rG);
    const uint8_t *data = m + 16 * pre;
    const size_t dlen = len - 16 * pre;
    const uint32_t nfull = (uint32_t)(dlen / 64), T = nfull / G + 1, pad = T * G - nfull;
    std::vector<Poly> acc(G, poly_zero());
    for (size_t i = 0; i < pre; ++i)
        acc[pad - 1] = poly_step(acc[pad - 1], block_of(m + 16 * i, 16), r1);
    for (uint32_t t = 0; t < T; ++t)
        for (uint32_t l = 0; l < (uint32_t)G; ++l) {
            const uint32_t q = t * G + l;
            if (q < pad)
                continue;
            const uint8_t *c = data + 64 * (size_t)(q - pad);
            acc[l] = poly_chunk(acc[l], rG, block_of(c, 16), block_of(c + 16, 16), block_of(c + 32, 16), block_of(c + 48, 16), r1,
                                r2, r3, r4);
        }
    Poly sq = r4;
    for (int b = 0; b < log2g; ++b) {
        std::vector<Poly> t(G);
        for (int l = 0; l < G; ++l)
            t[l] = poly_combine_stage(acc[l], sq, (uint32_t)l, b);
        for (int l = 0; l < G; ++l)
            acc[l] = poly_add(t[l], t[l ^ (1 << b)]);
        sq = poly_mul(sq, sq);
    }
    for (int l = 1; l < G; ++l)
        if (memcmp(&acc[l], &acc[0], sizeof(Poly)) != 0) {
            memset(tag, 0xee, 16);  // every lane must hold the same sum
            return;
        }
    Poly a = acc[0];
    for (size_t o = 64 * (size_t)nfull; o < dlen; o += 16)
        a = poly_step(a, block_of(data + o, dlen - o < 16 ? dlen - o : 16), r1);
    finish(a, s, tag);
}

static int hexv(const char *h, std::vector<uint8_t> &out)
{
    out.clear();
    for (; h[0] && h[1]; h += 2) {
        unsigned v;
        if (sscanf(h, "%2x", &v) != 1)
            return -1;
        out.push_back((uint8_t)v);
    }
    return 0;
}

struct A3 {
    const char *key, *msg, *tag;
};

// RFC 8439 Appendix A.3, test vectors #1 - #11 (key = r || s)
static const char *TEXT_IETF =
    "416e79207375626d697373696f6e20746f20746865204945544620696e74656e6465642062792074686520436f6e7472696275746f7220666f72207075"
    "626c69636174696f6e20617320616c6c206f722070617274206f6620616e204945544620496e7465726e65742d4472616674206f722052464320616e6420"
    "616e792073746174656d656e74206d6164652077697468696e2074686520636f6e74657874206f6620616e204945544620616374697669747920697320"
    "636f6e7369646572656420616e20224945544620436f6e747269627574696f6e222e20537563682073746174656d656e747320696e636c756465206f72"
    "616c2073746174656d656e747320696e20494554462073657373696f6e732c2061732077656c6c206173207772697474656e20616e6420656c65637472"
    "6f6e696320636f6d6d756e69636174696f6e73206d61646520617420616e792074696d65206f7220706c6163652c20776869636820617265206164647265"
    "7373656420746f";
static const char *TEXT_JABBER =
    "2754776173206272696c6c69672c20616e642074686520736c6974687920746f7665730a446964206779726520616e642067696d626c6520696e207468"
    "6520776162653a0a416c6c206d696d737920776572652074686520626f726f676f7665732c0a416e6420746865206d6f6d65207261746873206f757467"
    "726162652e";

int main(int argc, char **argv)
{
    // RFC 8439 §2.3.2
    {
        ChaChaKey k{0x03020100, 0x07060504, 0x0b0a0908, 0x0f0e0d0c, 0x13121110, 0x17161514, 0x1b1a1918, 0x1f1e1d1c,
                    0x09000000, 0x4a000000, 0x00000000};
        const ChaChaBlock b = chacha20_block(k, 1);
        const uint32_t want[16] = {0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                                   0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2};
        const uint32_t got[16] = {b.x0, b.x1, b.x2, b.x3, b.x4, b.x5, b.x6, b.x7, b.x8, b.x9, b.x10, b.x11, b.x12, b.x13, b.x14, b.x15};
        if (memcmp(want, got, sizeof(want)) != 0) {
            printf("chacha20 block (RFC 8439 2.3.2) differs\n");
            return 1;
        }
        // the record nonce: IV 00 01 .. 0b, seq 0x0102030405060708
        ChaChaKey n{};
        chacha_nonce(n, 0x03020100, 0x07060504, 0x0b0a0908, 0x0102030405060708ull);
        if (n.n0 != 0x03020100 || n.n1 != (0x07060504u ^ 0x04030201u) || n.n2 != (0x0b0a0908u ^ 0x08070605u)) {
            printf("record nonce differs\n");
            return 1;
        }
    }
    const A3 a3[11] = {
        {"0000000000000000000000000000000000000000000000000000000000000000",
         "00000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000",
         "00000000000000000000000000000000"},
        {"0000000000000000000000000000000036e5f6b5c5e06070f0efca96227a863e", TEXT_IETF, "36e5f6b5c5e06070f0efca96227a863e"},
        {"36e5f6b5c5e06070f0efca96227a863e00000000000000000000000000000000", TEXT_IETF, "f3477e7cd95417af89a6b8794c310cf0"},
        {"1c9240a5eb55d38af333888604f6b5f0473917c1402b80099dca5cbc207075c0", TEXT_JABBER, "4541669a7eaaee61e708dc7cbcc5eb62"},
        {"0200000000000000000000000000000000000000000000000000000000000000", "ffffffffffffffffffffffffffffffff",
         "03000000000000000000000000000000"},
        {"02000000000000000000000000000000ffffffffffffffffffffffffffffffff", "02000000000000000000000000000000",
         "03000000000000000000000000000000"},
        {"0100000000000000000000000000000000000000000000000000000000000000",
         "fffffffffffffffffffffffffffffffff0ffffffffffffffffffffffffffffff11000000000000000000000000000000",
         "05000000000000000000000000000000"},
        {"0100000000000000000000000000000000000000000000000000000000000000",
         "fffffffffffffffffffffffffffffffffbfefefefefefefefefefefefefefefe01010101010101010101010101010101",
         "00000000000000000000000000000000"},
        {"0200000000000000000000000000000000000000000000000000000000000000", "fdffffffffffffffffffffffffffffff",
         "faffffffffffffffffffffffffffffff"},
        {"0100000000000000040000000000000000000000000000000000000000000000",
         "e33594d7505e43b900000000000000003394d7505e4379cd01000000000000000000000000000000000000000000000001000000000000000000000000000000",
         "14000000000000005500000000000000"},
        {"0100000000000000040000000000000000000000000000000000000000000000",
         "e33594d7505e43b900000000000000003394d7505e4379cd010000000000000000000000000000000000000000000000",
         "13000000000000000000000000000000"},
    };
    static const int GS[4] = {1, 4, 16, 64}, LG[4] = {0, 2, 4, 6};
    for (int i = 0; i < 11; ++i) {
        std::vector<uint8_t> key, msg, want;
        if (hexv(a3[i].key, key) || hexv(a3[i].msg, msg) || hexv(a3[i].tag, want) || key.size() != 32 || want.size() != 16) {
            printf("A.3 #%d: bad vector text\n", i + 1);
            return 1;
        }
        uint8_t tag[16];
        mac_serial(key.data(), key.data() + 16, msg.data(), msg.size(), tag);
        if (memcmp(tag, want.data(), 16) != 0) {
            printf("A.3 #%d: serial tag differs\n", i + 1);
            return 1;
        }
        for (int g = 0; g < 4; ++g) {
            mac_lanes(GS[g], LG[g], 0, key.data(), key.data() + 16, msg.data(), msg.size(), tag);
            if (memcmp(tag, want.data(), 16) != 0) {
                printf("A.3 #%d: lane-split tag differs at G=%d\n", i + 1, GS[g]);
                return 1;
            }
        }
    }
    if (argc < 2) {
        printf("ok 0\n");
        return 0;
    }
    FILE *f = fopen(argv[1], "rb");
    if (f == nullptr) {
        printf("cannot open %s\n", argv[1]);
        return 1;
    }
    size_t n = 0;
    uint8_t hdr[36];
    while (fread(hdr, 1, 36, f) == 36) {
        const uint32_t len = le32(hdr + 32);
        std::vector<uint8_t> msg(len);
        uint8_t want[16], tag[16];
        if ((len != 0 && fread(msg.data(), 1, len, f) != len) || fread(want, 1, 16, f) != 16) {
            printf("triple %zu: truncated file\n", n);
            return 1;
        }
        mac_serial(hdr, hdr + 16, msg.data(), len, tag);
        if (memcmp(tag, want, 16) != 0) {
            printf("triple %zu (len %u): serial tag differs\n", n, len);
            return 1;
        }
        for (int g = 0; g < 4; ++g) {
            const size_t pre = (len / 16) < (n % 3) ? 0 : n % 3;
            mac_lanes(GS[g], LG[g], pre, hdr, hdr + 16, msg.data(), len, tag);
            if (memcmp(tag, want, 16) != 0) {
                printf("triple %zu (len %u): lane-split tag differs at G=%d\n", n, len, GS[g]);
                return 1;
            }
        }
        ++n;
    }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
