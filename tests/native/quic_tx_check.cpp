/*
 * quic_tx_check.cpp -- stand-alone CPU check of hsig-picotls_amd/csrc/quic_tx.h, the code quic_tx_kernel.hip runs: the packet
 * number of a request, its encoded length, the refusals, the header bytes, the key slot and the descriptors of a sent packet,
 * and the state after a call.  No GPU, no HIP call.  The passes of the kernels are walked here single-threaded, with plain
 * loads and stores where the kernels use atomics, in forward and in backward request order: both must give the model's
 * outcome.
 *
 * tests/test_quic_tx_native.py writes the cases from the plain-Python model (tests/quic_tx_ref.py):
 *     L <pn> <largest_acked> <min_len> <want length, 0: none>
 *     C <count> <stride> <hp slots> <in_len> <buf_len> <pn_len> <has rx> <n>
 *       <next_pn largest_acked gen dcid_len flags dcid-hex(40) rx_gen> x count   <data_off pkt_off conn len> x n
 *       <want status pn pkt_len slot header-hex|-> x n   <want next_pn gen> x count
 * Every array sits in an exactly-sized allocation, a sent packet's header in one of exactly its length.  Prints "ok <cases>"
 * and exits 0, or the first difference and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define GF128_FN static inline
#include "quic_tx.h"

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

struct Want {
    uint32_t status;
    uint64_t pn;
    uint32_t pkt_len;
    long long slot;
    std::vector<uint8_t> header;
    bool sent;
};

static std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < s.size(); i += 2)
        out.push_back((uint8_t)std::strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

static std::vector<uint32_t> exclusive_scan(const std::vector<uint32_t> &flags, uint32_t *total)
{
    std::vector<uint32_t> out(flags.size());
    uint32_t sum = 0;
    for (size_t j = 0; j < flags.size(); ++j) {
        out[j] = sum;
        sum += flags[j];
    }
    *total = sum;
    return out;
}

static void run_call(const QuicTxLimits &lim, const std::vector<ptls_hip_quic_txconn_t> &before, const std::vector<uint32_t> &rx_gen,
                     const std::vector<ptls_hip_quic_txreq_t> &reqs, const std::vector<Want> &want,
                     const std::vector<std::pair<uint64_t, uint32_t>> &want_after, bool backward)
{
    const size_t n = reqs.size();
    std::vector<ptls_hip_quic_txconn_t> conns = before;
    const auto at = [&](size_t k) { return backward ? n - 1 - k : k; };
    const auto is_head = [&](size_t j) { return j == 0 || reqs[j - 1].conn != reqs[j].conn; };
    const auto gen_of = [&](uint32_t c) { return quic_tx_gen(conns[c].gen, lim.has_rx_phase != 0, lim.has_rx_phase != 0 ? rx_gen[c] : 0u); };
    /* the head pass */
    std::vector<uint32_t> first(lim.nconn, QTX_NO_POS), flags(n);
    for (size_t k = 0; k < n; ++k) {
        const size_t j = at(k);
        flags[j] = is_head(j) ? 1u : 0u;
        if (flags[j] != 0 && reqs[j].conn < lim.nconn && (uint32_t)j < first[reqs[j].conn])
            first[reqs[j].conn] = (uint32_t)j;
    }
    uint32_t nruns = 0;
    const std::vector<uint32_t> run_of = exclusive_scan(flags, &nruns);
    /* the runs pass */
    std::vector<uint32_t> run_start(nruns + 1, 0xdddddddd);
    for (size_t k = 0; k < n; ++k) {
        const size_t j = at(k);
        if (is_head(j))
            run_start[run_of[j]] = (uint32_t)j;
        if (j + 1 == n)
            run_start[nruns] = (uint32_t)n;
    }
    /* the select pass */
    std::vector<uint32_t> status(n, 0xdddddddd), pkt_len(n, 0xdddddddd), sent(n);
    std::vector<uint64_t> pn_out(n, 0xdddddddddddddddd);
    uint64_t sums[QTX_NSTATS] = {};
    for (size_t k = 0; k < n; ++k) {
        const size_t j = at(k);
        const ptls_hip_quic_txreq_t r = reqs[j];
        QuicTxVerdict v{PTLS_HIP_QUIC_TX_NO_CONN, 0, 0};
        uint64_t pn = UINT64_MAX;
        if (r.conn < lim.nconn) {
            const uint32_t run = run_of[j] - (is_head(j) ? 0u : 1u);
            const uint32_t h = run_start[run];
            if (first[r.conn] != h) {
                v.status = PTLS_HIP_QUIC_TX_SPLIT;
            } else {
                pn = quic_tx_pn(conns[r.conn].next_pn, j - h);
                v = quic_tx_judge(r, pn, conns[r.conn].largest_acked, conns[r.conn].dcid_len, lim);
            }
        }
        status[j] = v.status, pn_out[j] = pn, pkt_len[j] = v.pkt_len;
        sent[j] = v.status == PTLS_HIP_QUIC_TX_SENT ? 1u : 0u;
        if (sent[j] != 0)
            sums[QTX_STAT_COUNT] += 1, sums[QTX_STAT_BYTES] += v.pkt_len, sums[QTX_STAT_BLOCKS64] += r.len / 64u;
    }
    uint32_t m = 0;
    const std::vector<uint32_t> pos = exclusive_scan(sent, &m);
    CHECK(m == sums[QTX_STAT_COUNT], "%u sent flags, a count of %llu", m, (ull)sums[QTX_STAT_COUNT]);
    /* the build pass */
    std::vector<ptls_hip_quic_packet_t> packed(m);
    std::vector<ptls_hip_record_t> recs(m);
    std::vector<ptls_hip_supp_t> supp(m);
    std::vector<uint32_t> keys(m);
    std::vector<std::vector<uint8_t>> headers(n);
    for (size_t k = 0; k < n; ++k) {
        const size_t j = at(k);
        if (status[j] != PTLS_HIP_QUIC_TX_SENT)
            continue;
        const ptls_hip_quic_txreq_t r = reqs[j];
        const uint32_t dcid_len = conns[r.conn].dcid_len;
        const uint32_t pn_len = pkt_len[j] - 1u - dcid_len - r.len - QTX_TAG;
        const uint32_t gen = gen_of(r.conn);
        std::vector<uint8_t> &hdr = headers[j];
        hdr.assign(1u + dcid_len + pn_len, 0xdd);
        hdr[0] = (uint8_t)quic_tx_first_byte(conns[r.conn].flags, gen, pn_len);
        for (uint32_t i = 0; i < QTX_MAX_DCID; ++i)
            if (i < dcid_len)
                hdr[1u + i] = conns[r.conn].dcid[i];
        for (uint32_t i = 0; i < 4; ++i)
            if (i < pn_len)
                hdr[1u + dcid_len + i] = (uint8_t)quic_tx_pn_byte(pn_out[j], pn_len, i);
        const ptls_hip_quic_packet_t p = quic_tx_packet(r, pn_out[j], pn_len, pkt_len[j], dcid_len, quic_tx_slot(r.conn, lim.stride, gen));
        packed[pos[j]] = p;
        recs[pos[j]] = quic_tx_record(p);
        supp[pos[j]] = quic_tx_supp(p, pos[j]);
        keys[pos[j]] = quic_tx_sort_key(r.len);
    }
    /* the apply pass */
    for (size_t k = 0; k < n; ++k) {
        const size_t j = at(k);
        const uint32_t conn = reqs[j].conn;
        if (conn >= lim.nconn || !is_head(j) || first[conn] != (uint32_t)j)
            continue;
        const uint32_t len = run_start[run_of[j] + 1u] - (uint32_t)j;
        const uint32_t gen = gen_of(conn);
        conns[conn].next_pn = quic_tx_pn(conns[conn].next_pn, len);
        conns[conn].gen = gen;
        first[conn] = QTX_NO_POS;
    }
    /* against the model */
    uint64_t bytes = 0;
    for (size_t j = 0; j < n; ++j) {
        const Want &w = want[j];
        CHECK(status[j] == w.status && pn_out[j] == w.pn && pkt_len[j] == w.pkt_len,
              "request %zu: status %u pn %llu pkt_len %u, the model %u %llu %u (backward %d)", j, status[j], (ull)pn_out[j], pkt_len[j],
              w.status, (ull)w.pn, w.pkt_len, (int)backward);
        if (!w.sent)
            continue;
        bytes += w.pkt_len;
        CHECK(headers[j] == w.header, "request %zu: the header differs (backward %d)", j, (int)backward);
        const ptls_hip_quic_packet_t &p = packed[pos[j]];
        const ptls_hip_record_t &rec = recs[pos[j]];
        const ptls_hip_supp_t &sp = supp[pos[j]];
        const size_t hl = w.header.size();
        CHECK((long long)p.key == w.slot && p.hp_key == reqs[j].conn && p.pn == w.pn && p.pkt_len == w.pkt_len &&
                  p.pkt_off == reqs[j].pkt_off && p.data_off == reqs[j].data_off && (size_t)p.pn_offset + p.pn_len == hl &&
                  p.pn_len == (w.header[0] & 3u) + 1u && p.flags == 0,
              "request %zu: the packed descriptor differs", j);
        CHECK(rec.in_off == reqs[j].data_off && rec.out_off == reqs[j].pkt_off + hl && rec.aad_off == reqs[j].pkt_off && rec.seq == w.pn &&
                  rec.len == reqs[j].len && rec.aad_len == hl && (long long)rec.key == w.slot && rec.flags == 0,
              "request %zu: the record differs", j);
        CHECK(sp.sample_off == reqs[j].pkt_off + p.pn_offset + 4u && sp.mask_off == 16ull * pos[j] && sp.hp_key == reqs[j].conn &&
                  sp.flags == PTLS_HIP_SUPP_ENABLE && sp.sample_off + 16 <= reqs[j].pkt_off + w.pkt_len,
              "request %zu: the header-protection descriptor differs", j);
        CHECK(keys[pos[j]] == 4095u - (reqs[j].len >> 4) && keys[pos[j]] < 4096u, "request %zu: sort key %u", j, keys[pos[j]]);
    }
    CHECK(bytes == sums[QTX_STAT_BYTES], "the sum of pkt_len is %llu, the model's %llu", (ull)sums[QTX_STAT_BYTES], (ull)bytes);
    for (size_t c = 0; c < conns.size(); ++c) {
        ptls_hip_quic_txconn_t w = before[c];
        w.next_pn = want_after[c].first, w.gen = want_after[c].second;
        CHECK(std::memcmp(&w, &conns[c], sizeof(w)) == 0, "connection %zu: next_pn %llu gen %u, the model %llu %u (backward %d)", c,
              (ull)conns[c].next_pn, conns[c].gen, (ull)w.next_pn, w.gen, (int)backward);
    }
    for (uint32_t f : first)
        CHECK(f == QTX_NO_POS, "the scratch is not reset");
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: quic_tx_check CASES\n");
        return 2;
    }
    static_assert(sizeof(ptls_hip_quic_txconn_t) == 48 && sizeof(ptls_hip_quic_txreq_t) == 24, "the state is 48 bytes, a request 24");
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(f, line)) {
        ++g_line;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        if (kind == 'L') {
            ull pn, la, min_len, want;
            in >> pn >> la >> min_len >> want;
            CHECK(!in.fail(), "malformed L line");
            const uint32_t got = quic_tx_pn_len(pn, la, (uint32_t)min_len);
            CHECK(got == want, "length %u, the model %llu", got, want);
        } else if (kind == 'C') {
            ull count, stride, hp, in_len, buf_len, pn_len, has_rx, n;
            in >> count >> stride >> hp >> in_len >> buf_len >> pn_len >> has_rx >> n;
            CHECK(!in.fail() && count >= 1, "malformed C line");
            QuicTxLimits lim{};
            lim.in_len = in_len, lim.buf_len = buf_len;
            lim.nconn = (uint32_t)std::min(std::min(count, stride), hp);
            lim.stride = (uint32_t)stride, lim.min_pn_len = (uint32_t)pn_len, lim.has_rx_phase = (uint32_t)has_rx;
            std::vector<ptls_hip_quic_txconn_t> conns(count);
            std::vector<uint32_t> rx_gen(count);
            for (ull c = 0; c < count; ++c) {
                ull next, la, gen, dl, fl, rg;
                std::string hex;
                in >> next >> la >> gen >> dl >> fl >> hex >> rg;
                CHECK(!in.fail() && hex.size() == 40, "malformed connection %llu", c);
                ptls_hip_quic_txconn_t t;
                std::memset(&t, 0xee, sizeof(t)); /* (the reserved bytes too: they must come back) */
                t.next_pn = next, t.largest_acked = la, t.gen = (uint32_t)gen, t.dcid_len = (uint8_t)dl, t.flags = (uint8_t)fl;
                const std::vector<uint8_t> d = unhex(hex);
                std::memcpy(t.dcid, d.data(), 20);
                conns[c] = t;
                rx_gen[c] = (uint32_t)rg;
            }
            std::vector<ptls_hip_quic_txreq_t> reqs(n);
            for (ull j = 0; j < n; ++j) {
                ull a, b, c, d;
                in >> a >> b >> c >> d;
                reqs[j] = ptls_hip_quic_txreq_t{a, b, (uint32_t)c, (uint32_t)d};
            }
            std::vector<Want> want(n);
            for (ull j = 0; j < n; ++j) {
                ull st, pn, pl;
                long long slot;
                std::string hex;
                in >> st >> pn >> pl >> slot >> hex;
                want[j] = Want{(uint32_t)st, pn, (uint32_t)pl, slot, hex == "-" ? std::vector<uint8_t>() : unhex(hex), hex != "-"};
            }
            std::vector<std::pair<uint64_t, uint32_t>> after(count);
            for (ull c = 0; c < count; ++c) {
                ull next, gen;
                in >> next >> gen;
                after[c] = {next, (uint32_t)gen};
            }
            CHECK(!in.fail(), "malformed C line");
            for (int backward = 0; backward < 2; ++backward)
                run_call(lim, conns, rx_gen, reqs, want, after, backward != 0);
        } else {
            CHECK(false, "unknown case kind");
        }
        ++cases;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
