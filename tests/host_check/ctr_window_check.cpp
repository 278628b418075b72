/*
 * ctr_window_check.cpp -- CPU check of csrc/ctr_window.h (the counter-mode window constants of the batch kernel) against
 * plain FIPS-197 rounds built on the oracle's AES (oracle/aesgcm_oracle.c).  Stand-alone (own main, no GPU, no HIP):
 * tests/test_ctr_window_host.py compiles and runs it, with AddressSanitizer + UndefinedBehaviorSanitizer.
 *
 * For PAIRS random (key, nonce) pairs of each key size and every block counter 2 .. 65535:
 *   - the state after round 2 from the window form equals two plain rounds (SubBytes, ShiftRows, MixColumns,
 *     AddRoundKey byte by byte), with the window constants refreshed exactly where the kernel refreshes them: a lane
 *     steps its counter by KP * G = 2 .. 64 per iteration from any starting phase, takes its first iteration's constants
 *     from the record's (ctr_window) and steps them (ctr_window_step, from the previous iteration's counter) whenever
 *     ctr_window_crossed(counter, step), and also where it did not cross (another lane of its wave did);
 *   - windows visited out of order (random jumps, refreshed when the held window differs) give the right state too;
 *   - constants of another window give a wrong state (the check can see a missed refresh);
 *   - on a sample of counters the remaining rounds (the oracle's, from the round-2 state) give the oracle's ciphertext.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ctr_window.h"

extern "C" {
#include "aesgcm_oracle.h"
}

using namespace ptls_hip;

static uint8_t sbox[256];
static uint32_t T0[256];

static uint8_t xtime(uint8_t a)
{
    return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0));
}

struct HostTab {
    template <int K>
    uint32_t t0(uint32_t x) const
    {
        return T0[(x >> (8 * K)) & 255u];
    }
    template <int K>
    uint32_t t2(uint32_t x) const
    {
        const uint32_t v = T0[(x >> (8 * K)) & 255u];
        return (v << 16) | (v >> 16);
    }
};

/* one plain round on state bytes s[4 * col + row] with the 16 round-key bytes k */
static void plain_round(uint8_t s[16], const uint8_t *k)
{
    uint8_t t[16];
    for (int c = 0; c < 4; ++c)
        for (int row = 0; row < 4; ++row)
            t[4 * c + row] = sbox[s[4 * ((c + row) & 3) + row]];
    for (int c = 0; c < 4; ++c) {
        const uint8_t a0 = t[4 * c], a1 = t[4 * c + 1], a2 = t[4 * c + 2], a3 = t[4 * c + 3], all = a0 ^ a1 ^ a2 ^ a3;
        s[4 * c + 0] = (uint8_t)(a0 ^ all ^ xtime(a0 ^ a1));
        s[4 * c + 1] = (uint8_t)(a1 ^ all ^ xtime(a1 ^ a2));
        s[4 * c + 2] = (uint8_t)(a2 ^ all ^ xtime(a2 ^ a3));
        s[4 * c + 3] = (uint8_t)(a3 ^ all ^ xtime(a3 ^ a0));
    }
    for (int i = 0; i < 16; ++i)
        s[i] ^= k[i];
}

static uint32_t le32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

static uint32_t bswap(uint32_t x)
{
    return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static long failed = 0, checks = 0;

static void expect(bool ok, const char *what, int key_len, int pair, uint32_t ctr, uint32_t step)
{
    ++checks;
    if (!ok && failed++ < 10)
        std::fprintf(stderr, "FAIL %s: key_len %d pair %d counter %u step %u\n", what, key_len, pair, ctr, step);
}

int main(int argc, char **argv)
{
    const int PAIRS = argc > 1 ? std::atoi(argv[1]) : 32;
    /* the oracle's S-box: one round as the last one (no MixColumns) under all-zero round keys is SubBytes + ShiftRows */
    {
        const uint8_t zero_rk[32] = {0};
        for (int x = 0; x < 256; ++x) {
            uint8_t in[16] = {0}, out[16];
            in[0] = (uint8_t)x;
            oracle_aes_encrypt(zero_rk, 1, in, out);
            sbox[x] = out[0];
        }
        for (int x = 0; x < 256; ++x) {
            const uint8_t s = sbox[x], s2 = xtime(s), s3 = (uint8_t)(s2 ^ s);
            T0[x] = (uint32_t)s2 | ((uint32_t)s << 8) | ((uint32_t)s << 16) | ((uint32_t)s3 << 24);
        }
        if (sbox[0] != 0x63 || sbox[0x53] != 0xed) { /* FIPS-197 Figure 7 */
            std::fprintf(stderr, "S-box extraction failed\n");
            return 2;
        }
    }
    const HostTab tab;
    std::vector<uint32_t> ref(65536 * 4);
    for (int key_len = 16; key_len <= 32; key_len += 16) {
        for (int pair = 0; pair < PAIRS; ++pair) {
            uint8_t key[32], nonce[12], rkb[240];
            for (int i = 0; i < 32; ++i)
                key[i] = (uint8_t)rng();
            for (int i = 0; i < 12; ++i)
                nonce[i] = (uint8_t)rng();
            const int rounds = oracle_aes_expand(key, (size_t)key_len, rkb);
            uint32_t rk[60];
            for (int i = 0; i < 4 * (rounds + 1); ++i)
                rk[i] = le32(rkb + 4 * i);
            const uint32_t n0 = le32(nonce), n1 = le32(nonce + 4), n2 = le32(nonce + 8);
            const CtrConst cc = ctr_const(tab, rk, n0, n1, n2);

            /* reference: two plain rounds of every counter block */
            for (uint32_t ctr = 2; ctr < 65536; ++ctr) {
                uint8_t s[16];
                std::memcpy(s, nonce, 12);
                s[12] = 0, s[13] = 0, s[14] = (uint8_t)(ctr >> 8), s[15] = (uint8_t)ctr;
                for (int i = 0; i < 16; ++i)
                    s[i] ^= rkb[i];
                plain_round(s, rkb + 16);
                plain_round(s, rkb + 32);
                for (int c = 0; c < 4; ++c)
                    ref[4 * ctr + c] = le32(s + 4 * c);
            }
            auto same = [&](uint32_t ctr, const uint32_t (&s)[4]) {
                return s[0] == ref[4 * ctr] && s[1] == ref[4 * ctr + 1] && s[2] == ref[4 * ctr + 2] && s[3] == ref[4 * ctr + 3];
            };

            /* the kernel's walk: every step KP * G, every starting phase; refresh at the first iteration and at a crossing */
            for (uint32_t step = 2; step <= 64; step *= 2) {
                for (uint32_t first = 2; first < 2 + step; ++first) {
                    CtrWin w = {0, 0, 0, 0}, ws = {0, 0, 0, 0};
                    for (uint32_t ctr = first; ctr < 65536; ctr += step) {
                        const uint32_t cw = bswap(ctr);
                        if (ctr == first) { /* the kernel's first iteration: from the record's constants */
                            w = ws = ctr_window(tab, cc, cw);
                        } else if (ctr_window_crossed(ctr, step)) {
                            w = ctr_window(tab, cc, cw);
                            /* the kernel's loop: stepped from the previous iteration's counter, with k11 and r03 only */
                            ws = ctr_window_step(tab, cc.k11, cc.r03, ws, bswap(ctr - step), cw);
                        } else if (((ctr / step) & 7u) == 0) {
                            /* another lane of the wave crossed: this lane steps too, which must change nothing */
                            ws = ctr_window_step(tab, cc.k11, cc.r03, ws, bswap(ctr - step), cw);
                        }
                        uint32_t s[4];
                        ctr_rounds12_window(tab, cc, w, cw, s);
                        expect(same(ctr, s), "walk", key_len, pair, ctr, step);
                        ctr_rounds12_window(tab, cc, ws, cw, s);
                        expect(same(ctr, s), "stepped walk", key_len, pair, ctr, step);
                    }
                }
            }
            /* a walk that starts in the middle of a window (a lane whose first data block is not block 0) */
            for (uint32_t first = 100; first < 65536; first += 4099) {
                CtrWin w = {0, 0, 0, 0};
                const uint32_t step = 8;
                for (uint32_t ctr = first, it = 0; ctr < 65536 && it < 200; ctr += step, ++it) {
                    const uint32_t cw = bswap(ctr);
                    if (it == 0 || ctr_window_crossed(ctr, step))
                        w = ctr_window(tab, cc, cw);
                    uint32_t s[4];
                    ctr_rounds12_window(tab, cc, w, cw, s);
                    expect(same(ctr, s), "mid-window start", key_len, pair, ctr, step);
                }
            }
            /* windows out of order: random jumps, refreshed when the held window is not the counter's */
            {
                CtrWin w = {0, 0, 0, 0};
                uint32_t held = 0xffffffffu;
                for (int j = 0; j < 20000; ++j) {
                    const uint32_t ctr = 2 + (uint32_t)(rng() % 65534u);
                    const uint32_t cw = bswap(ctr);
                    if (ctr_window_of(ctr) != held) {
                        w = ctr_window(tab, cc, cw);
                        held = ctr_window_of(ctr);
                    }
                    uint32_t s[4];
                    ctr_rounds12_window(tab, cc, w, cw, s);
                    expect(same(ctr, s), "jump", key_len, pair, ctr, 0);
                }
            }
            /* a missed refresh is visible: another window's constants give another state */
            for (uint32_t ctr = 300; ctr < 65536; ctr += 1021) {
                const CtrWin w = ctr_window(tab, cc, bswap(ctr - 256));
                uint32_t s[4];
                ctr_rounds12_window(tab, cc, w, bswap(ctr), s);
                expect(!same(ctr, s), "stale window must differ", key_len, pair, ctr, 0);
            }
            /* the remaining rounds on a sample: the oracle continues from the round-2 state (its first step XORs a round
             * key in, so round key 2 is XORed out first) and must reach its own ciphertext of the whole block */
            for (uint32_t ctr = 2; ctr < 65536; ctr += 257) {
                const CtrWin w = ctr_window(tab, cc, bswap(ctr));
                uint32_t s[4];
                ctr_rounds12_window(tab, cc, w, bswap(ctr), s);
                uint8_t mid[16], got[16], want[16], blk[16];
                for (int c = 0; c < 4; ++c)
                    for (int k = 0; k < 4; ++k)
                        mid[4 * c + k] = (uint8_t)((s[c] >> (8 * k)) ^ rkb[32 + 4 * c + k]);
                oracle_aes_encrypt(rkb + 32, rounds - 2, mid, got);
                std::memcpy(blk, nonce, 12);
                blk[12] = 0, blk[13] = 0, blk[14] = (uint8_t)(ctr >> 8), blk[15] = (uint8_t)ctr;
                oracle_aes_encrypt(rkb, rounds, blk, want);
                expect(std::memcmp(got, want, 16) == 0, "whole block", key_len, pair, ctr, 0);
            }
        }
    }
    std::printf("ctr_window_check: %s (%ld failed of %ld checks, %d pairs per key size)\n", failed ? "FAILED" : "ok", failed, checks,
                PAIRS);
    return failed ? 1 : 0;
}
