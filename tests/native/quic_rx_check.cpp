/*
 * quic_rx_check.cpp -- stand-alone CPU check of the device-side receive step's arithmetic (hsig-picotls_amd/csrc/quic_rx.h,
 * the code quic_rx_kernel.hip runs) and of the host planning it feeds: planner.cpp (choose_lanes / choose_chacha_lanes, their
 * cores over sums, build_chunks) and slice_plan.cpp's quic_records, linked in as they are (no HIP call is made; fail() and
 * g_err, engine.cpp's, are defined here).
 *
 * tests/test_quic_rx_native.py writes the cases from the plain-Python model (tests/quic_rx_ref.py):
 *     S <buf_len> <out_len> <nslots> <hp_nslots> <type_mask> <has_info> <pkt_off> <data_off> <pkt_len> <key> <hp_key>
 *       <pn_offset> <type> <want 0|1>                                                      the select rule on one descriptor
 *     L <ncu> <n> <ghash> <blocks64> <runs> <max16> <lanes> <chacha_lanes>                 a packet list: the model's sums and lanes
 *       then n lines <pkt_len> <pn_offset> <key>, then one line of n positions: the model's plan order
 * For an L case the sums come from quic_rx.h's terms added up as the stats kernel adds them (integers), the lanes from the
 * cores over those sums AND from choose_lanes / choose_chacha_lanes over the records quic_records makes of the packets (what
 * ptls_hip_quic_batch_new plans from): all must equal the model's.  The order comes from a stable sort by quic_rx_sort_key
 * AND from build_chunks at SPARSE_LANES over those records: both must equal the model's.
 * Prints "ok <cases>" and exits 0, or the first difference and exits 1.
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <sstream>
#include <string>
#include <vector>

#include "host.h"

#define GF128_FN static inline
#include "quic_rx.h"

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

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
        std::fprintf(stderr, "usage: quic_rx_check CASES\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(f, line)) {
        ++g_line;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'S') {
            QuicRxLimits l{};
            unsigned long long pkt_off, data_off, pkt_len, key, hp_key, pn_offset, type, want;
            in >> l.buf_len >> l.out_len >> l.nslots >> l.hp_nslots >> l.type_mask >> l.has_info >> pkt_off >> data_off >> pkt_len >> key >>
                hp_key >> pn_offset >> type >> want;
            CHECK(!in.fail(), "malformed S line");
            /* the descriptor alone in an exactly-sized allocation */
            auto *p = new ptls_hip_quic_packet_t();
            p->pkt_off = pkt_off, p->data_off = data_off, p->pkt_len = (uint32_t)pkt_len, p->key = (uint32_t)key;
            p->hp_key = (uint32_t)hp_key, p->pn_offset = (uint16_t)pn_offset;
            const bool got = quic_rx_selectable(*p, (uint32_t)type, l);
            delete p;
            CHECK(got == (want != 0), "selectable gives %d, the model %llu", (int)got, want);
        } else if (kind == 'L') {
            unsigned ncu;
            size_t n;
            unsigned long long w_ghash, w_blocks, w_runs, w_max16;
            int w_lanes, w_chacha;
            in >> ncu >> n >> w_ghash >> w_blocks >> w_runs >> w_max16 >> w_lanes >> w_chacha;
            CHECK(!in.fail() && n != 0, "malformed L line");
            std::vector<ptls_hip_quic_packet_t> pk(n);
            for (size_t i = 0; i < n; ++i) {
                CHECK((bool)std::getline(f, line), "missing packet line");
                ++g_line;
                std::istringstream pin(line);
                unsigned long long pkt_len, pn_offset, key;
                pin >> pkt_len >> pn_offset >> key;
                CHECK(!pin.fail(), "malformed packet line");
                pk[i] = ptls_hip_quic_packet_t{};
                pk[i].pkt_off = 64 * i, pk[i].data_off = 64 * i + pn_offset + 1;
                pk[i].pkt_len = (uint32_t)pkt_len, pk[i].pn_offset = (uint16_t)pn_offset, pk[i].key = pk[i].hp_key = (uint32_t)key;
            }
            std::vector<uint32_t> w_order(n);
            CHECK((bool)std::getline(f, line), "missing order line");
            ++g_line;
            std::istringstream oin(line);
            for (size_t i = 0; i < n; ++i)
                oin >> w_order[i];
            CHECK(!oin.fail(), "malformed order line");

            /* the sums as the stats kernel takes them */
            uint64_t st[QRX_NSTATS] = {};
            for (size_t j = 0; j < n; ++j) {
                st[QRX_STAT_GHASH] += quic_rx_ghash_elems(pk[j]);
                st[QRX_STAT_BLOCKS64] += quic_rx_len(pk[j]) / 64u;
                if (j != 0 && pk[j - 1].key != pk[j].key)
                    ++st[QRX_STAT_RUNS];
                st[QRX_STAT_MAX16] = std::max<uint64_t>(st[QRX_STAT_MAX16], quic_rx_len(pk[j]) >> 4);
            }
            CHECK(st[QRX_STAT_GHASH] == w_ghash && st[QRX_STAT_BLOCKS64] == w_blocks && st[QRX_STAT_RUNS] + 1 == w_runs &&
                      st[QRX_STAT_MAX16] == w_max16,
                  "sums %llu %llu %llu %llu", (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2] + 1,
                  (unsigned long long)st[3]);
            const int lanes = choose_lanes_from((double)st[QRX_STAT_GHASH], n, (size_t)st[QRX_STAT_RUNS] + 1, ncu);
            const int chacha = choose_chacha_lanes_from((double)st[QRX_STAT_BLOCKS64], n, ncu);
            /* what ptls_hip_quic_batch_new plans from */
            std::vector<ptls_hip_record_t> recs;
            std::vector<ptls_hip_supp_t> supp;
            quic_records(pk.data(), n, true, recs, supp);
            for (ptls_hip_record_t &r : recs)
                r.in_off |= 1u;
            const int h_lanes = choose_lanes(recs.data(), n, ncu), h_chacha = choose_chacha_lanes(recs.data(), n, ncu);
            CHECK(lanes == w_lanes && h_lanes == w_lanes, "lanes: from sums %d, host planner %d, model %d", lanes, h_lanes, w_lanes);
            CHECK(chacha == w_chacha && h_chacha == w_chacha, "chacha lanes: from sums %d, host planner %d, model %d", chacha, h_chacha,
                  w_chacha);
            /* the plan order */
            std::vector<uint32_t> order(n);
            std::iota(order.begin(), order.end(), 0u);
            std::stable_sort(order.begin(), order.end(),
                             [&](uint32_t x, uint32_t y) { return quic_rx_sort_key(pk[x]) < quic_rx_sort_key(pk[y]); });
            std::vector<Chunk> ch;
            std::vector<uint32_t> h_order;
            bool aligned = true;
            build_chunks(recs.data(), n, SPARSE_LANES, ncu, ch, h_order, aligned);
            CHECK(ch.size() == 1 && ch[0].first == 0 && ch[0].count == n && ch[0].key == 0xffffffffu && ch[0].flags == 0 && !aligned,
                  "build_chunks' chunk");
            for (size_t t = 0; t < n; ++t) {
                CHECK(quic_rx_sort_key(pk[t]) <= QRX_KEY_MAX, "sort key of %zu", t);
                CHECK(order[t] == w_order[t] && h_order[t] == w_order[t], "order[%zu]: by sort key %u, build_chunks %u, model %u", t,
                      order[t], h_order[t], w_order[t]);
            }
        } else {
            CHECK(false, "unknown case kind");
        }
        ++cases;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
