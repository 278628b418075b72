/*
 * quic_phase_check.cpp -- stand-alone CPU check of hsig-picotls_amd/csrc/quic_phase.h, the code quic_phase_kernel.hip runs:
 * the generation chosen by Key Phase bit, the key slot, what an opened packet means for its connection, and the state after a
 * commit.  No GPU, no HIP call.
 *
 * tests/test_quic_phase_native.py writes the cases from the plain-Python model (tests/quic_phase_ref.py):
 *     G <first> <masked> <m0> <pn> <gen> <first_pn> <key> <stride> <want first> <want gen_out> <want slot>
 *     C <result> <gen_out> <gen> <want class 0 none | 1 current | 2 next>
 *     A <gen> <first_pn> <min_next> <min_cur> <want gen> <want first_pn> <want updated 0|1>
 * Every state sits alone in an exactly-sized allocation.  Prints "ok <cases>" and exits 0, or the first difference and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#define GF128_FN static inline
#include "quic_phase.h"

using namespace ptls_hip;

static size_t g_line = 0;

#define CHECK(cond, ...)                                                                                                           \
    do {                                                                                                                           \
        if (!(cond)) {                                                                                                             \
            std::printf("line %zu: %s: ", g_line, #cond);                                                                          \
            std::printf(__VA_ARGS__);                                                                                              \
            std::printf("\n");                                                                                                     \
            std::exit(1);                                                                                                          \
        }                                                                                                                          \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: quic_phase_check CASES\n");
        return 2;
    }
    static_assert(sizeof(ptls_hip_quic_keyphase_t) == 16, "the state is 16 bytes");
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(f, line)) {
        ++g_line;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'G') {
            unsigned long long first, masked, m0, pn, gen, first_pn, key, stride, w_first, w_gen, w_slot;
            in >> first >> masked >> m0 >> pn >> gen >> first_pn >> key >> stride >> w_first >> w_gen >> w_slot;
            CHECK(!in.fail(), "malformed G line");
            auto *st = new ptls_hip_quic_keyphase_t{first_pn, (uint32_t)gen, 0};
            const uint32_t fb = quic_phase_first_byte((uint32_t)first, masked != 0, (uint32_t)m0);
            const uint32_t g = quic_phase_gen(fb, pn, st->gen, st->first_pn);
            const uint32_t slot = quic_phase_slot((uint32_t)key, (uint32_t)stride, g);
            delete st;
            CHECK(fb == w_first, "first byte %u, the model %llu", fb, w_first);
            CHECK(g == w_gen, "generation %u, the model %llu", g, w_gen);
            CHECK(slot == w_slot, "slot %u, the model %llu", slot, w_slot);
        } else if (kind == 'C') {
            unsigned long long result, gen_out, gen;
            int want;
            in >> result >> gen_out >> gen >> want;
            CHECK(!in.fail(), "malformed C line");
            const int got = quic_phase_class(result, (uint32_t)gen_out, (uint32_t)gen);
            CHECK(got == want, "class %d, the model %d", got, want);
        } else if (kind == 'A') {
            unsigned long long gen, first_pn, min_next, min_cur, w_gen, w_first_pn, w_upd;
            in >> gen >> first_pn >> min_next >> min_cur >> w_gen >> w_first_pn >> w_upd;
            CHECK(!in.fail(), "malformed A line");
            auto *st = new ptls_hip_quic_keyphase_t{first_pn, (uint32_t)gen, 0};
            quic_phase_apply(st, min_next, min_cur);
            const ptls_hip_quic_keyphase_t got = *st;
            delete st;
            CHECK(got.gen == w_gen && got.first_pn == w_first_pn && got.reserved == 0, "state {%u, %llu}, the model {%llu, %llu}", got.gen,
                  (unsigned long long)got.first_pn, w_gen, w_first_pn);
            CHECK(quic_phase_updates(min_next) == (w_upd != 0), "updated flag");
        } else {
            CHECK(false, "unknown case kind");
        }
        ++cases;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
