/*
 * quic_slice_check.cpp -- the copy transport's planning of QUIC packet slices (hsig-picotls_amd/csrc/slice_plan.cpp:
 * quic_records, plan_quic_slice over plan_copy_order / plan_copy_slice) on the CPU, built with plain g++ and linked with
 * slice_plan.cpp alone (no HIP call is made; fail() and g_err, engine.cpp's, are defined here).
 *
 * tests/test_quic_slice_plan_native.py writes the cases and its own model of the plan, the greedy cut:
 *     C <id> <S|O> <slice_bytes> <n> <slices, or -1: the plan is refused> <first packet of the refused slice>
 *     <pkt_off> <data_off> <pkt_len> <pn_offset> <pn_len> <flags>      n lines
 *     <end of slice 0> <end of slice 1> ...                            one line (refused: the slices before the refusal)
 * This program plans every case as pipeline.cpp does, compares the cut and checks, per slice, on byte maps of the caller's
 * buffers:
 *   both   the staging limits (input and output span, packets per slice, gap pieces, gap bytes); slice-local offsets
 *          (packets, records, samples) equal the caller's modulo 16 and lie inside the staging; the records and
 *          header-protection descriptors are the packets';
 *   seal   the header pieces are exactly each packet's pn_offset + pn_len bytes, placed at the packet's start; the
 *          copies back cover every byte of the slice's packets, no byte of another slice's packet, and every other
 *          byte they cover is a gap filled from the same byte of the caller's buffer;
 *   open   the same for the plaintext areas at their pn_len = 1 length; the last 3 bytes of every area are staged from
 *          the caller's buffer at their place; the header return names every packet's pkt_off and pn_offset.
 * Prints "ok <cases> <slices>" or the first failure.
 */
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "host.h"

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

static long g_case = -1;
static size_t g_slice = 0;

#define CHECK(cond, ...)                                                                                                           \
    do {                                                                                                                           \
        if (!(cond)) {                                                                                                             \
            std::printf("FAIL case %ld slice %zu: %s: ", g_case, g_slice, #cond);                                                  \
            std::printf(__VA_ARGS__);                                                                                              \
            std::printf("\n");                                                                                                     \
            std::exit(1);                                                                                                          \
        }                                                                                                                          \
    } while (0)

struct Case {
    bool open;
    size_t slice_bytes;
    long nslices;
    size_t refused_at;
    std::vector<ptls_hip_quic_packet_t> pkts;
    std::vector<size_t> ends;
};

/* the bytes the slice owns in the output buffer: seal the packet, open the plaintext area */
static Span owned(const Case &c, const ptls_hip_quic_packet_t &p)
{
    if (!c.open)
        return Span{p.pkt_off, p.pkt_off + p.pkt_len};
    return Span{p.data_off, p.data_off + (p.pkt_len - p.pn_offset - 17u)};
}

static size_t check_case(const Case &c)
{
    const size_t n = c.pkts.size(), max_recs = c.slice_bytes / 16 + 1, staging = c.slice_bytes + 64;
    const ModeInfo m(c.open ? PIPE_QUIC_OPEN : PIPE_QUIC_SEAL);
    std::vector<ptls_hip_record_t> recs;
    std::vector<ptls_hip_supp_t> supp;
    quic_records(c.pkts.data(), n, c.open, recs, supp);
    CHECK(recs.size() == n && supp.size() == (c.open ? 0 : n), "quic_records sizes");
    CopyOrder ord;
    plan_copy_order(recs.data(), n, m, ord);
    /* who owns each output byte: the slice of the model's cut, or -1 */
    uint64_t extent = 0;
    for (const auto &p : c.pkts)
        extent = std::max(extent, owned(c, p).hi);
    std::vector<int32_t> owner(extent, -1);
    for (size_t k = 0, i = 0; k < c.ends.size(); i = c.ends[k++]) /* (a refused call: the slices before the refusal) */
        for (size_t t = i; t < c.ends[k]; ++t)
            for (uint64_t b = owned(c, c.pkts[t]).lo; b < owned(c, c.pkts[t]).hi; ++b)
                owner[b] = (int32_t)k;
    QuicSlicePlan pl;
    size_t k = 0;
    for (size_t i = 0; i < n; i = pl.s.j, ++k) {
        g_slice = k;
        const int rc = plan_quic_slice(c.pkts.data(), recs.data(), c.open ? nullptr : supp.data(), n, i, m, c.slice_bytes, max_recs, ord, pl);
        if (rc != 0) {
            CHECK(rc == PTLS_HIP_EINVAL && c.nslices < 0 && i == c.refused_at, "refused at %zu (%s), the model says %ld slices, refusal at %zu",
                  i, g_err.c_str(), c.nslices, c.refused_at);
            CHECK(g_err.find("does not fit") != std::string::npos, "%s", g_err.c_str());
            return k;
        }
        const SlicePlan &s = pl.s;
        CHECK(k < c.ends.size() && s.j == c.ends[k], "slice ends at %zu, the model says %zu", s.j, k < c.ends.size() ? c.ends[k] : 0);
        const size_t cnt = s.j - i;
        /* staging limits */
        CHECK(cnt >= 1 && cnt <= slot_max_masks(c.slice_bytes), "%zu packets", cnt);
        CHECK(s.in.hi - s.in.lo <= c.slice_bytes && s.out.hi - s.out.lo <= c.slice_bytes, "spans %llu %llu",
              (unsigned long long)(s.in.hi - s.in.lo), (unsigned long long)(s.out.hi - s.out.lo));
        CHECK(s.in_base % 16 == 0 && s.out_base % 16 == 0 && s.in.lo - s.in_base < 16 && s.out.lo - s.out_base < 16, "bases");
        CHECK(s.aad.lo == 0 && s.aad.hi == 0 && s.mask_dst.empty(), "no AAD buffer and no mask leaves the slot");
        CHECK(s.gaps.size() == s.gap_src.size() && s.gaps.size() <= 2 * max_recs && s.gaps.size() >= cnt, "%zu gap pieces", s.gaps.size());
        CHECK(pl.pkts.size() == cnt && s.recs.size() == cnt && s.supp.size() == (c.open ? 0 : cnt), "descriptor counts");
        uint64_t staged = 0;
        for (size_t g = 0; g < s.gaps.size(); ++g) {
            CHECK(s.gaps[g].src == staged && s.gaps[g].len == s.gap_src[g].hi - s.gap_src[g].lo && s.gaps[g].len != 0, "gap piece %zu", g);
            CHECK(s.gaps[g].dst == s.gap_src[g].lo - s.out_base && s.gap_src[g].lo >= s.out.lo && s.gap_src[g].hi <= s.out.hi,
                  "gap piece %zu is placed where it came from, inside the output span", g);
            staged += s.gaps[g].len;
        }
        CHECK(staged <= c.slice_bytes, "%llu bytes of gap staging", (unsigned long long)staged);
        const size_t ngap = s.gaps.size() - cnt; /* the gaps proper come first, then one piece per packet */
        const uint64_t pkt_base = c.open ? s.in_base : s.out_base, data_base = c.open ? s.out_base : s.in_base;
        for (size_t t = 0; t < cnt; ++t) {
            const ptls_hip_quic_packet_t &p = c.pkts[i + t], &q = pl.pkts[t];
            const ptls_hip_record_t &r = s.recs[t];
            const uint32_t pn_len = c.open ? 1u : p.pn_len, hl = p.pn_offset + pn_len;
            /* slice-local packet descriptor: the caller's alignment modulo 16, inside the staging */
            CHECK(q.pkt_off == p.pkt_off - pkt_base && q.data_off == p.data_off - data_base, "packet %zu offsets", i + t);
            CHECK((q.pkt_off - p.pkt_off) % 16 == 0 && (q.data_off - p.data_off) % 16 == 0, "packet %zu alignment", i + t);
            CHECK(q.pkt_off + p.pkt_len <= staging && q.data_off + (p.pkt_len - hl - 16) <= staging, "packet %zu leaves the staging", i + t);
            CHECK(q.pkt_len == p.pkt_len && q.pn == p.pn && q.key == p.key && q.hp_key == p.hp_key && q.pn_offset == p.pn_offset &&
                      q.pn_len == p.pn_len && q.flags == p.flags,
                  "packet %zu fields", i + t);
            /* the record the kernel reads (open: provisional, quic_unprotect_kernel rewrites it from q) */
            CHECK(r.aad_off == q.pkt_off && r.aad_len == hl && r.len == p.pkt_len - hl - 16 && r.seq == p.pn && r.key == p.key && r.flags == 0,
                  "record %zu", i + t);
            CHECK(c.open ? (r.in_off == q.pkt_off + hl && r.out_off == q.data_off) : (r.in_off == q.data_off && r.out_off == q.pkt_off + hl),
                  "record %zu offsets", i + t);
            const GapPiece &g = s.gaps[ngap + t];
            const Span &gs = s.gap_src[ngap + t];
            if (!c.open) {
                CHECK(s.supp[t].sample_off == q.pkt_off + p.pn_offset + 4u && s.supp[t].mask_off == 16 * t && s.supp[t].hp_key == p.hp_key &&
                          s.supp[t].flags == PTLS_HIP_SUPP_ENABLE,
                      "header-protection descriptor %zu", i + t);
                CHECK(gs.lo == p.pkt_off && g.len == hl && g.dst == q.pkt_off, "header piece of packet %zu", i + t);
            } else {
                const Span a = owned(c, p);
                CHECK(a.hi - a.lo >= 3 && gs.lo == a.hi - 3 && g.len == 3 && g.dst == q.data_off + (a.hi - a.lo) - 3, "tail of packet %zu", i + t);
                CHECK(pl.hdr_dst.size() == cnt && pl.hdr_dst[t].off == p.pkt_off && pl.hdr_dst[t].pn_offset == p.pn_offset,
                      "header return of packet %zu", i + t);
            }
        }
        if (!c.open)
            CHECK(pl.hdr_dst.empty(), "a seal slice returns no headers");
        /* the copies back over the byte map */
        std::vector<uint8_t> filled(s.out.hi - s.out.lo, 0), covered(s.out.hi - s.out.lo, 0);
        for (size_t g = 0; g < ngap; ++g)
            for (uint64_t b = s.gap_src[g].lo; b < s.gap_src[g].hi; ++b) {
                CHECK(owner[b] != (int32_t)k && !filled[b - s.out.lo], "gap byte %llu", (unsigned long long)b);
                filled[b - s.out.lo] = 1;
            }
        for (size_t q = 0; q < s.pieces.size(); ++q) {
            const Span &pc = s.pieces[q];
            CHECK(pc.lo < pc.hi && pc.lo >= s.out.lo && pc.hi <= s.out.hi && (q == 0 || pc.lo > s.pieces[q - 1].hi), "piece %zu", q);
            for (uint64_t b = pc.lo; b < pc.hi; ++b) {
                covered[b - s.out.lo] = 1;
                if (owner[b] == (int32_t)k)
                    continue;
                CHECK(owner[b] < 0, "the copy back writes byte %llu of slice %d", (unsigned long long)b, owner[b]);
                CHECK(filled[b - s.out.lo], "the copy back writes byte %llu, which is neither the slice's nor a filled gap", (unsigned long long)b);
            }
        }
        for (uint64_t b = s.out.lo; b < s.out.hi; ++b) {
            CHECK(owner[b] != (int32_t)k || covered[b - s.out.lo], "byte %llu of the slice is not copied back", (unsigned long long)b);
            CHECK(!filled[b - s.out.lo] || covered[b - s.out.lo], "gap byte %llu is filled but not copied back", (unsigned long long)b);
        }
    }
    CHECK(c.nslices >= 0 && k == (size_t)c.nslices, "%zu slices, the model says %ld", k, c.nslices);
    return k;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: quic_slice_check CASES\n");
        return 2;
    }
    std::ifstream f(argv[1]);
    std::string line;
    size_t cases = 0, slices = 0;
    while (std::getline(f, line)) {
        if (line.empty())
            continue;
        std::istringstream hs(line);
        char tag, mode;
        size_t n;
        Case c;
        hs >> tag >> g_case >> mode >> c.slice_bytes >> n >> c.nslices >> c.refused_at;
        if (!hs || tag != 'C' || (mode != 'S' && mode != 'O')) {
            std::fprintf(stderr, "bad case line: %s\n", line.c_str());
            return 2;
        }
        c.open = mode == 'O';
        c.pkts.resize(n);
        for (size_t t = 0; t < n; ++t) {
            std::getline(f, line);
            std::istringstream ps(line);
            unsigned long long pkt_off, data_off;
            unsigned pkt_len, pn_offset, pn_len, flags;
            ps >> pkt_off >> data_off >> pkt_len >> pn_offset >> pn_len >> flags;
            if (!ps) {
                std::fprintf(stderr, "bad packet line: %s\n", line.c_str());
                return 2;
            }
            ptls_hip_quic_packet_t p{};
            p.pkt_off = pkt_off, p.data_off = data_off, p.pkt_len = pkt_len;
            p.pn = 1000 + t, p.key = (uint32_t)(t % 7), p.hp_key = (uint32_t)(t % 5);
            p.pn_offset = (uint16_t)pn_offset, p.pn_len = (uint8_t)pn_len, p.flags = (uint8_t)flags;
            c.pkts[t] = p;
        }
        std::getline(f, line);
        std::istringstream es(line);
        for (size_t e; es >> e;)
            c.ends.push_back(e);
        g_slice = 0;
        slices += check_case(c);
        ++cases;
    }
    std::printf("ok %zu %zu\n", cases, slices);
    return 0;
}
