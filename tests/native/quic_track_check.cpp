/*
 * quic_track_check.cpp -- stand-alone CPU check of hsig-picotls_amd/csrc/quic_track.h, the code quic_track_kernel.hip runs:
 * what a packet number is against a space's state, the state after a call, and the table that finds a call's duplicates.
 * No GPU, no HIP call.  The three passes of the kernels are walked here single-threaded, with plain loads and stores where
 * the kernels use atomics, in forward and in backward packet order: both must give the model's outcome.
 *
 * tests/test_quic_track_native.py writes the cases from the plain-Python model (tests/quic_track_ref.py):
 *     O <pn> <next> <window> <want 0 none | 2 duplicate | 3 too old>
 *     T <count> <expected entries> <m>  <next window> x 3 count  <expected> x entries  <conn type result pn> x m
 *       <want verdict> x m  <want next window> x 3 count  <want expected> x entries  <n touched> <touched> x n
 *     P <keys> <collide 0|1>      the probe functions alone: `keys` (a power of two) keys, three positions each, into a table
 *                                 that is then exactly half full; with collide, every key starts at the same slot
 * Every array sits in an exactly-sized allocation.  Prints "ok <cases>" and exits 0, or the first difference and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define GF128_FN static inline
#include "quic_track.h"

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

typedef unsigned long long ull;

struct HostOps {
    static uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired)
    {
        const uint32_t old = *p;
        if (old == expected)
            *p = desired;
        return old;
    }
    static void min(uint32_t *p, uint32_t v)
    {
        if (v < *p)
            *p = v;
    }
};

struct Packet {
    uint32_t conn, type;
    uint64_t result, pn;
};

struct Keys {
    const std::vector<Packet> &pk;
    uint64_t count;
    uint64_t place_of(uint32_t j) const { return quic_track_place(pk[j].result, pk[j].conn, count, pk[j].type); }
    bool same(uint32_t occ, uint64_t place, uint64_t pn) const { return occ < pk.size() && pk[occ].pn == pn && place_of(occ) == place; }
};

struct Outcome {
    std::vector<uint32_t> verdict, touched;
    std::vector<ptls_hip_quic_pnspace_t> spaces;
    std::vector<uint64_t> expected;
};

static Outcome run_call(uint64_t count, std::vector<ptls_hip_quic_pnspace_t> spaces, std::vector<uint64_t> expected,
                        const std::vector<Packet> &pk, bool backward)
{
    const size_t m = pk.size();
    const Keys keys{pk, count};
    const uint64_t slots = quic_track_slots(m);
    std::vector<uint32_t> table(slots, QTK_EMPTY);
    std::vector<uint64_t> acc(6 * count, 0);
    Outcome out;
    out.verdict.assign(m, 0xdddddddd);
    for (size_t k = 0; k < m; ++k) { /* the claim pass */
        const uint32_t j = (uint32_t)(backward ? m - 1 - k : k);
        const uint64_t place = keys.place_of(j);
        if (place == UINT64_MAX)
            continue;
        if (quic_track_old(pk[j].pn, spaces[place].next, spaces[place].window) != PTLS_HIP_QUIC_PN_NONE)
            continue;
        CHECK(quic_track_claim<HostOps>(table.data(), slots, j, place, pk[j].pn, keys), "no slot for position %u", j);
        if (pk[j].pn + 1 > acc[2 * place])
            acc[2 * place] = pk[j].pn + 1;
    }
    for (size_t k = 0; k < m; ++k) { /* the verdict pass */
        const uint32_t j = (uint32_t)(backward ? m - 1 - k : k);
        uint32_t v = PTLS_HIP_QUIC_PN_NONE;
        const uint64_t place = keys.place_of(j);
        if (place != UINT64_MAX) {
            const ptls_hip_quic_pnspace_t st = spaces[place];
            v = quic_track_old(pk[j].pn, st.next, st.window);
            if (v == PTLS_HIP_QUIC_PN_NONE) {
                const uint32_t first = quic_track_find(table.data(), slots, place, pk[j].pn, keys);
                CHECK(first != QTK_EMPTY, "position %u is not in the table", j);
                if (first == j) {
                    v = PTLS_HIP_QUIC_PN_NEW;
                    acc[2 * place + 1] |= quic_track_bit(quic_track_next(st.next, acc[2 * place]), pk[j].pn);
                } else {
                    v = PTLS_HIP_QUIC_PN_DUPLICATE;
                }
            }
        }
        out.verdict[j] = v;
    }
    for (uint64_t c = 0; c < count; ++c) { /* the apply pass */
        bool any = false;
        for (uint64_t p = 3 * c; p < 3 * c + 3; ++p) {
            if (acc[2 * p] == 0)
                continue;
            any = true;
            quic_track_apply(&spaces[p], acc[2 * p], acc[2 * p + 1]);
            if (p < expected.size())
                expected[p] = spaces[p].next;
        }
        if (any)
            out.touched.push_back((uint32_t)c);
    }
    out.spaces = spaces;
    out.expected = expected;
    return out;
}

static void probe_case(uint64_t nkeys, bool collide)
{
    /* keys (place, pn): found by walking pn upwards until enough of them start where the case wants them */
    const uint64_t slots = quic_track_slots(nkeys);
    CHECK(slots == 2 * nkeys, "%llu keys are not a power of two", (ull)nkeys);
    std::vector<Packet> pk;
    std::vector<uint64_t> key_pn;
    const uint64_t home = quic_track_first(5, 0, slots);
    for (uint64_t pn = 0; key_pn.size() < nkeys; ++pn)
        if (!collide || quic_track_first(5, pn, slots) == home)
            key_pn.push_back(pn);
    /* three positions per key: position j holds key (7 j) mod nkeys (7 is odd: every key three times in 3 nkeys positions) */
    for (uint64_t j = 0; j < 3 * nkeys; ++j)
        pk.push_back(Packet{1, QP_ONE_RTT, 20, key_pn[(7 * j) % nkeys]});
    const Keys keys{pk, 2};
    for (int backward = 0; backward < 2; ++backward) {
        std::vector<uint32_t> table(slots, QTK_EMPTY);
        for (uint64_t k = 0; k < pk.size(); ++k) {
            const uint32_t j = (uint32_t)(backward ? pk.size() - 1 - k : k);
            CHECK(quic_track_claim<HostOps>(table.data(), slots, j, 5, pk[j].pn, keys), "no slot for position %u", j);
        }
        uint64_t used = 0;
        for (uint32_t occ : table)
            used += occ != QTK_EMPTY;
        CHECK(used == nkeys && 2 * used == slots, "%llu of %llu slots used", (ull)used, (ull)slots);
        for (uint32_t j = 0; j < pk.size(); ++j) {
            uint32_t lowest = j;
            for (uint32_t i = 0; i < j; ++i)
                if (pk[i].pn == pk[j].pn) {
                    lowest = i;
                    break;
                }
            const uint32_t got = quic_track_find(table.data(), slots, 5, pk[j].pn, keys);
            CHECK(got == lowest, "position %u: the table holds %u, the lowest is %u", j, got, lowest);
        }
        /* keys that never entered: another place with a number that did, a number that did not; the walk ends */
        CHECK(quic_track_find(table.data(), slots, 4, key_pn[0], keys) == QTK_EMPTY, "a key of another place was found");
        CHECK(quic_track_find(table.data(), slots, 5, key_pn.back() + 1, keys) == QTK_EMPTY, "an absent number was found");
    }
    if (collide) { /* a full table of other keys: both walks end after `slots` steps */
        std::vector<uint32_t> full(slots, 0u);
        CHECK(!quic_track_claim<HostOps>(full.data(), slots, 1, 4, 12345, keys), "a full table took a position");
        CHECK(quic_track_find(full.data(), slots, 4, 12345, keys) == QTK_EMPTY, "a full table held an absent key");
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: quic_track_check CASES\n");
        return 2;
    }
    static_assert(sizeof(ptls_hip_quic_pnspace_t) == 16, "the state is 16 bytes");
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(f, line)) {
        ++g_line;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'O') {
            ull pn, next, window, want;
            in >> pn >> next >> window >> want;
            CHECK(!in.fail(), "malformed O line");
            auto *st = new ptls_hip_quic_pnspace_t{next, window};
            const uint32_t got = quic_track_old(pn, st->next, st->window);
            delete st;
            CHECK(got == want, "verdict %u, the model %llu", got, want);
        } else if (kind == 'T') {
            ull count, entries, m, a, b, c, d;
            in >> count >> entries >> m;
            CHECK(!in.fail() && count >= 1, "malformed T line");
            std::vector<ptls_hip_quic_pnspace_t> spaces, want_spaces;
            std::vector<uint64_t> expected, want_expected;
            std::vector<Packet> pk;
            std::vector<uint32_t> want_verdict, want_touched;
            for (ull k = 0; k < 3 * count; ++k) {
                in >> a >> b;
                spaces.push_back(ptls_hip_quic_pnspace_t{a, b});
            }
            for (ull k = 0; k < entries; ++k) {
                in >> a;
                expected.push_back(a);
            }
            for (ull k = 0; k < m; ++k) {
                in >> a >> b >> c >> d;
                pk.push_back(Packet{(uint32_t)a, (uint32_t)b, c, d});
            }
            for (ull k = 0; k < m; ++k) {
                in >> a;
                want_verdict.push_back((uint32_t)a);
            }
            for (ull k = 0; k < 3 * count; ++k) {
                in >> a >> b;
                want_spaces.push_back(ptls_hip_quic_pnspace_t{a, b});
            }
            for (ull k = 0; k < entries; ++k) {
                in >> a;
                want_expected.push_back(a);
            }
            ull n = 0;
            in >> n;
            for (ull k = 0; k < n; ++k) {
                in >> a;
                want_touched.push_back((uint32_t)a);
            }
            CHECK(!in.fail(), "malformed T line");
            for (int backward = 0; backward < 2; ++backward) {
                const Outcome got = run_call(count, spaces, expected, pk, backward != 0);
                for (size_t j = 0; j < m; ++j)
                    CHECK(got.verdict[j] == want_verdict[j], "packet %zu: verdict %u, the model %u (backward %d)", j, got.verdict[j],
                          want_verdict[j], backward);
                for (size_t p = 0; p < 3 * count; ++p)
                    CHECK(got.spaces[p].next == want_spaces[p].next && got.spaces[p].window == want_spaces[p].window,
                          "space %zu: {%llu, %llx}, the model {%llu, %llx} (backward %d)", p, (ull)got.spaces[p].next,
                          (ull)got.spaces[p].window, (ull)want_spaces[p].next, (ull)want_spaces[p].window, backward);
                CHECK(got.expected == want_expected, "the expected-pn table differs (backward %d)", backward);
                CHECK(got.touched == want_touched, "the touched list differs (backward %d)", backward);
            }
        } else if (kind == 'P') {
            ull nkeys, collide;
            in >> nkeys >> collide;
            CHECK(!in.fail() && nkeys >= 1, "malformed P line");
            probe_case(nkeys, collide != 0);
        } else {
            CHECK(false, "unknown case kind");
        }
        ++cases;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
