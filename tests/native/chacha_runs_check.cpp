// Host check of csrc/chacha_runs.h (tests/test_chacha_runs_native.py): the piece map and the quad transpose of
// chacha_runs_kernel.hip, compiled with g++, for G = 4, 16, 64 and every nfull = 0 .. 3 G + 5 (every pad 1 .. G, one to four
// trips):
//   (a) the pieces all lanes move over all trips are exactly the 16-byte pieces of [0, 64 nfull), each once;
//   (b) per trip and instruction the lanes that move a piece form one range, their offsets rising by 16 per lane;
//   (c) after the transpose (runs_send / runs_recv, the rule the kernel's DPP stages apply) a lane with a block holds its four
//       pieces in order, the block is the one at place lambda(l), runs_piece_lane / _slot say where each piece went, and a
//       second transpose puts every piece back where it was loaded (the stores write the runs the loads read);
//   (d) the (r, s, message, tag) triples of the data file given as argv[1], folded through that deal: pieces fetched by the
//       map, transposed, hashed by the lane that owns them, the sums moved by runs_acc_source and joined by the combination
//       of poly1305.h, the rest serially.  File: records of r[16] s[16] len[u32 LE] msg[len] tag[16].
// Prints "ok <n>" or the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define GF128_FN static inline
#include "chacha_runs.h"
using namespace ptls_hip;

static const uint32_t NONE = 0xffffffffu;

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

static Poly block_of(const uint8_t *p, size_t n)  // n = 16: a whole block; n < 16: the final block's 0x01 rule
{
    uint8_t b[16] = {0};
    memcpy(b, p, n);
    if (n < 16)
        b[n] = 1;
    return poly_limbs(le32(b), le32(b + 4), le32(b + 8), le32(b + 12), n == 16 ? 1 : 0);
}

// one word per lane and register: the two stages as the kernel runs them, every lane sending before any receives
struct Regs {
    uint32_t v[4];
};

static void trade(std::vector<Regs> &r, int lo, int hi, int b)
{
    std::vector<uint32_t> give(r.size());
    for (size_t l = 0; l < r.size(); ++l)
        give[l] = runs_send(r[l].v[lo], r[l].v[hi], (uint32_t)l, b);
    for (size_t l = 0; l < r.size(); ++l)
        runs_recv(r[l].v[lo], r[l].v[hi], (uint32_t)l, b, give[l ^ ((size_t)1 << b)]);
}

static void transpose(std::vector<Regs> &r)
{
    trade(r, 0, 1, 0);
    trade(r, 2, 3, 0);
    trade(r, 0, 2, 1);
    trade(r, 1, 3, 1);
}

// the piece ids (offset / 16, or NONE) the G lanes load in trip t
static std::vector<Regs> load_ids(uint32_t G, uint32_t nfull, uint32_t t)
{
    std::vector<Regs> r(G);
    for (uint32_t l = 0; l < G; ++l)
        for (uint32_t j = 0; j < 4; ++j) {
            const int64_t off = runs_piece_off(G, nfull, t, j, l);
            r[l].v[j] = off < 0 ? NONE : (uint32_t)(off / 16);
        }
    return r;
}

static int check_map(uint32_t G, uint32_t nfull)
{
    const uint32_t T = runs_trips(G, nfull), pad = runs_pad(G, nfull);
    if (T != nfull / G + 1 || pad < 1 || pad > G || T * G - pad != nfull)
        return printf("G=%u nfull=%u: trips %u pad %u\n", G, nfull, T, pad), 1;
    std::vector<int> seen(4 * (size_t)nfull, 0);
    for (uint32_t t = 0; t < T; ++t) {
        for (uint32_t j = 0; j < 4; ++j) {
            int64_t prev = -1;
            bool started = false;
            for (uint32_t l = 0; l < G; ++l) {
                const int64_t off = runs_piece_off(G, nfull, t, j, l);
                if (off < 0) {
                    if (off != -1 || started || t != 0)  // (b) only leading lanes of trip 0 move nothing
                        return printf("G=%u nfull=%u t=%u j=%u l=%u: a hole in the run\n", G, nfull, t, j, l), 1;
                    continue;
                }
                if ((off & 15) != 0 || off + 16 > 64 * (int64_t)nfull)  // (a) inside the whole blocks
                    return printf("G=%u nfull=%u t=%u j=%u l=%u: offset %lld outside\n", G, nfull, t, j, l, (long long)off), 1;
                if (started && off != prev + 16)  // (b) one contiguous run
                    return printf("G=%u nfull=%u t=%u j=%u l=%u: offset %lld after %lld\n", G, nfull, t, j, l, (long long)off,
                                  (long long)prev), 1;
                started = true;
                prev = off;
                ++seen[(size_t)(off / 16)];
            }
        }
        // (c)
        const std::vector<Regs> loaded = load_ids(G, nfull, t);
        std::vector<Regs> r = loaded;
        transpose(r);
        for (uint32_t l = 0; l < G; ++l) {
            for (uint32_t j = 0; j < 4; ++j)
                if (r[runs_piece_lane(l, j)].v[runs_piece_slot(l)] != loaded[l].v[j])
                    return printf("G=%u nfull=%u t=%u: piece of lane %u instruction %u is not where the map says\n", G, nfull, t, l, j), 1;
            const uint32_t lam = runs_lambda(G, l);
            if (lam >= G || runs_lambda_inv(G, lam) != l || runs_acc_source(G, lam) != l)
                return printf("G=%u: lambda(%u) = %u does not invert\n", G, l, lam), 1;
            const bool has = t * G + lam >= pad;
            if (has != runs_has_block(G, nfull, t, l))
                return printf("G=%u nfull=%u t=%u l=%u: has_block\n", G, nfull, t, l), 1;
            if (!has)
                continue;
            const uint32_t blk = runs_block(G, nfull, t, l);
            if (blk != t * G + lam - pad || blk >= nfull)
                return printf("G=%u nfull=%u t=%u l=%u: block %u\n", G, nfull, t, l, blk), 1;
            for (uint32_t s = 0; s < 4; ++s)
                if (r[l].v[s] != 4 * blk + s)
                    return printf("G=%u nfull=%u t=%u l=%u: slot %u holds piece %u, not %u\n", G, nfull, t, l, s, r[l].v[s], 4 * blk + s), 1;
        }
        transpose(r);
        for (uint32_t l = 0; l < G; ++l)
            if (memcmp(&r[l], &loaded[l], sizeof(Regs)) != 0)
                return printf("G=%u nfull=%u t=%u l=%u: the second transpose does not undo the first\n", G, nfull, t, l), 1;
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1)  // (a)
            return printf("G=%u nfull=%u: piece %zu moved %d times\n", G, nfull, i, seen[i]), 1;
    return 0;
}

static void finish(Poly acc, const uint8_t *s, uint8_t tag[16])
{
    uint32_t t[4];
    poly_finish(acc, le32(s), le32(s + 4), le32(s + 8), le32(s + 12), t[0], t[1], t[2], t[3]);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            tag[4 * i + j] = (uint8_t)(t[i] >> (8 * j));
}

// the runs kernel's split: the first `pre` whole blocks play the AAD, then whole 64-byte chunks over G lanes, the rest serially
static void mac_runs(uint32_t G, int log2g, size_t pre, const uint8_t *r, const uint8_t *s, const uint8_t *m, size_t len, uint8_t tag[16])
{
    const Poly r1 = poly_clamp_r(le32(r), le32(r + 4), le32(r + 8), le32(r + 12));
    const Poly r2 = poly_mul(r1, r1), r3 = poly_mul(r2, r1), r4 = poly_mul(r2, r2);
    Poly rG = r4;
    for (int b = 0; b < log2g; ++b)
        rG = poly_mul(rG, rG);
    const uint8_t *data = m + 16 * pre;
    const size_t dlen = len - 16 * pre;
    const uint32_t nfull = (uint32_t)(dlen / 64), T = runs_trips(G, nfull), pad = runs_pad(G, nfull);
    std::vector<Poly> acc(G, poly_zero());
    for (uint32_t l = 0; l < G; ++l)
        if (runs_lambda(G, l) == pad - 1)
            for (size_t i = 0; i < pre; ++i)
                acc[l] = poly_step(acc[l], block_of(m + 16 * i, 16), r1);
    for (uint32_t t = 0; t < T; ++t) {
        std::vector<Regs> v = load_ids(G, nfull, t);
        transpose(v);
        for (uint32_t l = 0; l < G; ++l) {
            if (!runs_has_block(G, nfull, t, l))
                continue;
            Poly b[4];
            for (int q = 0; q < 4; ++q) {
                if (v[l].v[q] == NONE) {
                    memset(tag, 0xdd, 16);  // a lane with a block must hold four pieces
                    return;
                }
                b[q] = block_of(data + 16 * (size_t)v[l].v[q], 16);
            }
            acc[l] = poly_chunk(acc[l], rG, b[0], b[1], b[2], b[3], r1, r2, r3, r4);
        }
    }
    std::vector<Poly> moved(G);
    for (uint32_t mth = 0; mth < G; ++mth)
        moved[mth] = acc[runs_acc_source(G, mth)];
    acc = moved;
    Poly sq = r4;
    for (int b = 0; b < log2g; ++b) {
        std::vector<Poly> t(G);
        for (uint32_t l = 0; l < G; ++l)
            t[l] = poly_combine_stage(acc[l], sq, l, b);
        for (uint32_t l = 0; l < G; ++l)
            acc[l] = poly_add(t[l], t[l ^ (1u << b)]);
        sq = poly_mul(sq, sq);
    }
    for (uint32_t l = 1; l < G; ++l)
        if (memcmp(&acc[l], &acc[0], sizeof(Poly)) != 0) {
            memset(tag, 0xee, 16);  // every lane must hold the same sum
            return;
        }
    Poly a = acc[0];
    for (size_t o = 64 * (size_t)nfull; o < dlen; o += 16)
        a = poly_step(a, block_of(data + o, dlen - o < 16 ? dlen - o : 16), r1);
    finish(a, s, tag);
}

int main(int argc, char **argv)
{
    static const uint32_t GS[3] = {4, 16, 64};
    static const int LG[3] = {2, 4, 6};
    for (int g = 0; g < 3; ++g)
        for (uint32_t nfull = 0; nfull <= 3 * GS[g] + 5; ++nfull)
            if (check_map(GS[g], nfull))
                return 1;
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
            fclose(f);
            return 1;
        }
        for (int g = 0; g < 3; ++g) {
            const size_t pre = (len / 16) < (n % 3) ? 0 : n % 3;
            mac_runs(GS[g], LG[g], pre, hdr, hdr + 16, msg.data(), len, tag);
            if (memcmp(tag, want, 16) != 0) {
                printf("triple %zu (len %u): runs-split tag differs at G=%u\n", n, len, GS[g]);
                fclose(f);
                return 1;
            }
        }
        ++n;
    }
    fclose(f);
    printf("ok %zu\n", n);
    return 0;
}
