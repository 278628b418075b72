/*
 * quic_ack_check.cpp -- stand-alone CPU check of hsig-picotls_amd/csrc/quic_ack.h, the code quic_ack_kernel.hip runs: the
 * status and the frame length of a list entry, the frame's bytes, and the send request.  No GPU, no HIP call.  The two passes
 * of the kernels are walked here single-threaded with a plain prefix sum between them, in forward and in backward entry order:
 * both must give the model's outcome.
 *
 * tests/test_quic_ack_native.py writes the cases from the plain-Python model (tests/quic_ack_ref.py):
 *     F <next> <window> <delay> <max_ranges> <want status> <want frame, hex, or ->      one entry of a table of one connection
 *     C <count> <space> <delay> <max_ranges> <in_off> <pkt_base> <pkt_stride> <n>  <next window> x 3 count  <conn> x n
 *       <want status> x n  <want off> x n  <want len> x n  <n reqs> <data_off pkt_off conn len> x n reqs  <want frames, hex, or ->
 * Every array sits in an exactly-sized allocation, a frame buffer in one of exactly the wanted bytes.  Prints "ok <cases>" and
 * exits 0, or the first difference and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define GF128_FN static inline
#include "quic_ack.h"

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

static std::vector<uint8_t> unhex(const std::string &h)
{
    std::vector<uint8_t> out;
    if (h == "-")
        return out;
    for (size_t i = 0; i + 1 < h.size(); i += 2)
        out.push_back((uint8_t)std::strtoul(h.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

struct Call {
    uint64_t count, delay, in_off, pkt_base, pkt_stride;
    uint32_t space, max_ranges;
    std::vector<ptls_hip_quic_pnspace_t> spaces;
    std::vector<uint32_t> list;
};

struct Outcome {
    std::vector<uint32_t> status, off, len;
    std::vector<ptls_hip_quic_txreq_t> reqs;
    std::vector<uint8_t> frames;
};

/* the kernels' two passes; `bytes`: what the model wants the frames to take (the buffer holds exactly that) */
static Outcome run_call(const Call &c, size_t bytes, bool backward)
{
    const size_t n = c.list.size();
    std::vector<uint32_t> lens(n), flags(n);
    for (size_t k = 0; k < n; ++k) {
        const size_t j = backward ? n - 1 - k : k;
        ptls_hip_quic_pnspace_t st;
        uint32_t len;
        (void)quic_ack_judge(c.spaces.data(), c.count, c.space, c.list[j], c.delay, c.max_ranges, &st, &len);
        lens[j] = len;
        flags[j] = len != 0;
    }
    uint64_t total = 0, frames = 0; /* the scan levels: exclusive prefixes in place */
    for (size_t j = 0; j < n; ++j) {
        const uint32_t l = lens[j], f = flags[j];
        lens[j] = (uint32_t)total, flags[j] = (uint32_t)frames;
        total += l, frames += f;
    }
    CHECK(total == bytes, "the lengths sum to %llu, the model's frames take %zu", (ull)total, bytes);
    Outcome o;
    o.status.resize(n), o.off.resize(n), o.len.resize(n);
    o.reqs.resize(frames);
    o.frames.assign(bytes, 0xA5);
    for (size_t k = 0; k < n; ++k) {
        const size_t j = backward ? n - 1 - k : k;
        ptls_hip_quic_pnspace_t st;
        uint32_t len;
        o.status[j] = quic_ack_judge(c.spaces.data(), c.count, c.space, c.list[j], c.delay, c.max_ranges, &st, &len);
        o.off[j] = lens[j];
        o.len[j] = len;
        if (o.status[j] == PTLS_HIP_QUIC_ACK_OK) {
            CHECK((size_t)lens[j] + len <= bytes, "entry %zu: a frame of %u at %u leaves the buffer", j, len, lens[j]);
            const uint32_t wrote = quic_ack_write(o.frames.data() + lens[j], st.next, st.window, c.delay, c.max_ranges);
            CHECK(wrote == len, "entry %zu: %u bytes written, %u sized", j, wrote, len);
            CHECK(flags[j] < frames, "entry %zu: position %u of %llu", j, flags[j], (ull)frames);
            o.reqs[flags[j]] = quic_ack_request(c.in_off, lens[j], c.pkt_base, c.pkt_stride, flags[j], c.list[j], len);
        }
    }
    return o;
}

static void check_call(std::istringstream &in, const Call &c)
{
    const size_t n = c.list.size();
    Outcome want;
    want.status.resize(n), want.off.resize(n), want.len.resize(n);
    for (auto *v : {&want.status, &want.off, &want.len})
        for (uint32_t &x : *v)
            in >> x;
    size_t nreq = 0;
    in >> nreq;
    want.reqs.resize(nreq);
    for (auto &r : want.reqs) {
        ull a, b;
        in >> a >> b >> r.conn >> r.len;
        r.data_off = a, r.pkt_off = b;
    }
    std::string hex;
    in >> hex;
    CHECK(!in.fail(), "a short line");
    want.frames = unhex(hex);
    for (int backward = 0; backward < 2; ++backward) {
        const Outcome got = run_call(c, want.frames.size(), backward != 0);
        for (size_t j = 0; j < n; ++j) {
            CHECK(got.status[j] == want.status[j], "entry %zu (%d): status %u, want %u", j, backward, got.status[j], want.status[j]);
            CHECK(got.off[j] == want.off[j], "entry %zu (%d): offset %u, want %u", j, backward, got.off[j], want.off[j]);
            CHECK(got.len[j] == want.len[j], "entry %zu (%d): length %u, want %u", j, backward, got.len[j], want.len[j]);
        }
        CHECK(got.reqs.size() == nreq, "%zu requests, want %zu", got.reqs.size(), nreq);
        for (size_t k = 0; k < nreq; ++k) {
            const ptls_hip_quic_txreq_t &g = got.reqs[k], &w = want.reqs[k];
            CHECK(g.data_off == w.data_off && g.pkt_off == w.pkt_off && g.conn == w.conn && g.len == w.len,
                  "request %zu (%d): {%llu %llu %u %u}, want {%llu %llu %u %u}", k, backward, (ull)g.data_off, (ull)g.pkt_off, g.conn, g.len,
                  (ull)w.data_off, (ull)w.pkt_off, w.conn, w.len);
        }
        for (size_t b = 0; b < want.frames.size(); ++b)
            CHECK(got.frames[b] == want.frames[b], "frame byte %zu (%d): %02x, want %02x", b, backward, got.frames[b], want.frames[b]);
    }
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::printf("usage: quic_ack_check <cases>\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0;
    while (std::getline(f, line)) {
        ++g_line;
        if (line.empty())
            continue;
        std::istringstream in(line);
        char kind = 0;
        in >> kind;
        Call c{};
        if (kind == 'F') {
            ull next, window, delay;
            uint32_t want_status;
            std::string hex;
            in >> next >> window >> delay >> c.max_ranges >> want_status >> hex;
            CHECK(!in.fail(), "a short line");
            c.count = 1, c.delay = delay;
            c.spaces.assign(3, ptls_hip_quic_pnspace_t{(uint64_t)next, (uint64_t)window});
            c.list.assign(1, 0);
            const std::vector<uint8_t> want = unhex(hex);
            const Outcome got = run_call(c, want.size(), false);
            CHECK(got.status[0] == want_status, "status %u, want %u", got.status[0], want_status);
            CHECK(got.len[0] == want.size() && got.off[0] == 0, "length %u at %u, want %zu at 0", got.len[0], got.off[0], want.size());
            CHECK(got.reqs.size() == (want.empty() ? 0u : 1u), "%zu requests", got.reqs.size());
            for (size_t b = 0; b < want.size(); ++b)
                CHECK(got.frames[b] == want[b], "frame byte %zu: %02x, want %02x", b, got.frames[b], want[b]);
            if (want_status == PTLS_HIP_QUIC_ACK_OK)
                CHECK(want.size() >= 5 && want.size() <= PTLS_HIP_QUIC_ACK_MAX, "a frame of %zu bytes", want.size());
        } else if (kind == 'C') {
            ull delay, in_off, pkt_base, pkt_stride;
            size_t n = 0;
            in >> c.count >> c.space >> delay >> c.max_ranges >> in_off >> pkt_base >> pkt_stride >> n;
            c.delay = delay, c.in_off = in_off, c.pkt_base = pkt_base, c.pkt_stride = pkt_stride;
            c.spaces.resize(3 * c.count);
            for (auto &s : c.spaces) {
                ull a, b;
                in >> a >> b;
                s.next = a, s.window = b;
            }
            c.list.resize(n);
            for (uint32_t &x : c.list)
                in >> x;
            CHECK(!in.fail(), "a short line");
            check_call(in, c);
        } else {
            CHECK(false, "unknown case kind '%c'", kind);
        }
        ++cases;
    }
    std::printf("ok %zu\n", cases);
    return 0;
}
