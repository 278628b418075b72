/*
 * host_check.cpp -- the engine's host code under AddressSanitizer + UndefinedBehaviorSanitizer (the
 * reference's CI runs its tests the same way, /root/reference/.github/workflows/ci.yml:24-25).
 *
 * Built by `make -C hsig-picotls_amd asan` against the host units compiled with -fsanitize=address,undefined (the device
 * code objects are the product's, unchanged) and run by tests/test_host_sanitizers.py on a machine WITHOUT a GPU.  It
 * drives every host path that reads caller or wire bytes without needing a device:
 *   - ptls_hip_tls13_parse on 100 000 random and damaged record streams (parse_record / parse_record_header,
 *     lib/picotls.c:5020-5062), with every produced descriptor checked to lie inside the stream;
 *   - ptls_hip_tls13_frame / _wire_size on random message lists (buffer_push_encrypted_records, :747-794);
 *   - the launch planner (choose_lanes / build_chunks / plan_grid) on random descriptor sets, every plan checked to be a
 *     permutation in key runs;
 *   - ptls_hip_partition_bytes on random lengths and part counts;
 *   - the copy transport's slice plans (plan_copy_order / plan_copy_slice, slice_plan.cpp) on a thousand random layouts --
 *     the four modes, records in and out of output order, with and without header-protection descriptors in three mask
 *     layouts, 64 KiB and 1 MiB slices -- every slice's cut, spans, descriptors, copies back, gaps and mask places
 *     checked against the layout, and the two refusals;
 *   - the argument checks of the C ABI with NULL / out-of-range arguments, and the plugin's setup_crypto without a device
 *     (it must fail cleanly: no CPU fallback);
 *   - with a gfx950 device (argument "device", run on the GPU box): the host pipelines over random layouts -- both
 *     transports, records in and out of output order, 1-64-byte gaps, exactly-sized heap buffers -- sealed and opened
 *     back, every record compared with the CPU oracle (oracle/aesgcm_oracle.c, test infrastructure) and every byte
 *     between records checked unchanged: the slicing, gap-planning and descriptor code of pipeline.cpp under the
 *     sanitizers (the kernels are the product's).
 * Any sanitizer report aborts the process (-fno-sanitize-recover, halt_on_error); the exit status is 0 only when every
 * check held.  Test infrastructure only: nothing here ships.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>

#include "host.h"
#include "aesgcm_oracle.h"

static int failures = 0;
#define CHECK(c)                                                                                                                   \
    do {                                                                                                                           \
        if (!(c)) {                                                                                                                \
            fprintf(stderr, "host_check: %s:%d: %s\n", __FILE__, __LINE__, #c);                                                  \
            ++failures;                                                                                                            \
        }                                                                                                                          \
    } while (0)

/* a valid TLS 1.3 application-data stream (random ciphertext bytes: the parse does not decrypt), record starts in `starts` */
static std::vector<uint8_t> valid_stream(std::mt19937_64 &rng, std::vector<size_t> &starts)
{
    std::vector<uint8_t> w;
    const int nrec = 1 + (int)(rng() % 6);
    for (int r = 0; r < nrec; ++r) {
        const size_t len = 16 + (rng() % 4 == 0 ? rng() % (16384 + 256 - 15) : rng() % 400);
        starts.push_back(w.size());
        w.push_back(0x17);
        w.push_back(0x03);
        w.push_back(0x03);
        w.push_back((uint8_t)(len >> 8));
        w.push_back((uint8_t)len);
        for (size_t i = 0; i < len; ++i)
            w.push_back((uint8_t)rng());
    }
    return w;
}

static void damage(std::mt19937_64 &rng, std::vector<uint8_t> &w, const std::vector<size_t> &starts)
{
    const int n = 1 + (int)(rng() % 3);
    for (int d = 0; d < n; ++d) {
        const size_t rec = starts.empty() ? 0 : starts[rng() % starts.size()];
        switch (rng() % 7) {
        case 0: /* truncate */
            w.resize(w.empty() ? 0 : rng() % (w.size() + 1));
            break;
        case 1: /* a length field */
            if (rec + 5 <= w.size()) {
                const uint16_t L = (uint16_t)(rng() % 4 == 0 ? rng() : ((size_t)w[rec + 3] << 8 | w[rec + 4]) + (rng() % 41) - 20);
                w[rec + 3] = (uint8_t)(L >> 8);
                w[rec + 4] = (uint8_t)L;
            }
            break;
        case 2: /* the edges of the length checks */
            if (rec + 5 <= w.size()) {
                static const uint16_t edge[] = {0, 1, 15, 16, 17, 16384 + 256, 16384 + 257, 65535};
                const uint16_t L = edge[rng() % 8];
                w[rec + 3] = (uint8_t)(L >> 8);
                w[rec + 4] = (uint8_t)L;
            }
            break;
        case 3: /* a type byte */
            if (rec < w.size())
                w[rec] = (uint8_t)rng();
            break;
        case 4: /* garbage appended */
            for (size_t i = rng() % 40; i > 0; --i)
                w.push_back((uint8_t)rng());
            break;
        case 5: /* version bytes */
            if (rec + 3 <= w.size())
                w[rec + 1 + rng() % 2] = (uint8_t)rng();
            break;
        default: /* a random byte anywhere */
            if (!w.empty())
                w[rng() % w.size()] = (uint8_t)rng();
            break;
        }
    }
}

static void check_parse(std::mt19937_64 &rng, int streams)
{
    std::vector<ptls_hip_record_t> recs;
    for (int s = 0; s < streams; ++s) {
        std::vector<size_t> starts;
        std::vector<uint8_t> w = valid_stream(rng, starts);
        if (s % 8 != 0)
            damage(rng, w, starts);
        /* the stream in an exactly-sized heap buffer, so that a read one byte past it is an ASan report */
        uint8_t *buf = w.empty() ? nullptr : static_cast<uint8_t *>(malloc(w.size()));
        if (buf != nullptr)
            memcpy(buf, w.data(), w.size());
        const size_t cap = 1 + rng() % 8;
        recs.assign(cap, ptls_hip_record_t{});
        size_t nrecs = 0, consumed = 0;
        const uint64_t wire_off = rng() % 1000, out_base = rng() % 1000, seq = rng() % 100;
        const int rc = ptls_hip_tls13_parse(buf, w.size(), wire_off, 3, seq, out_base, recs.data(), cap, &nrecs, &consumed);
        CHECK(rc == 0 || rc == PTLS_HIP_TLS13_DECODE_ERROR || rc == PTLS_HIP_TLS13_SHORT_RECORD);
        CHECK(nrecs <= cap && consumed <= w.size());
        uint64_t pos = 0, out = out_base;
        for (size_t k = 0; k < nrecs; ++k) {
            const ptls_hip_record_t &r = recs[k];
            CHECK(r.aad_off == wire_off + pos && r.aad_len == 5 && r.in_off == r.aad_off + 5 && r.out_off == out);
            CHECK(r.in_off - wire_off + r.len + 16 <= w.size() && r.seq == seq + k && r.key == 3);
            CHECK(buf[pos] == 0x17 && buf[pos + 1] == 3 && buf[pos + 2] == 3);
            CHECK(((size_t)buf[pos + 3] << 8 | buf[pos + 4]) == (size_t)r.len + 16 && r.len + 16 <= PTLS_HIP_TLS13_MAX_ENCRYPTED);
            out += r.len;
            pos += 5 + r.len + 16;
        }
        CHECK(pos == consumed);
        free(buf);
    }
    /* argument checks */
    size_t n = 0, c = 0;
    CHECK(ptls_hip_tls13_parse(nullptr, 5, 0, 0, 0, 0, recs.data(), 1, &n, &c) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_tls13_parse(nullptr, 0, 0, 0, 0, 0, nullptr, 0, &n, &c) == 0 && n == 0 && c == 0);
    CHECK(ptls_hip_tls13_parse("\x17", 1, 0, 0, 0, 0, nullptr, 4, &n, &c) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_tls13_parse("\x17", 1, 0, 0, 0, 0, recs.data(), 1, nullptr, &c) == PTLS_HIP_EINVAL);
}

static void check_frame(std::mt19937_64 &rng, int lists)
{
    for (int l = 0; l < lists; ++l) {
        std::vector<ptls_hip_tls13_message_t> msgs(rng() % 6);
        uint64_t in = 0, out = 0;
        for (auto &m : msgs) {
            m = ptls_hip_tls13_message_t{};
            m.len = (uint32_t)(rng() % 4 == 0 ? rng() % 70000 : rng() % 2000);
            m.in_off = in;
            m.out_off = out;
            m.seq = rng() % 1000;
            m.key = (uint32_t)(rng() % 4);
            m.type = 23;
            in += m.len;
            out += ptls_hip_tls13_wire_size(m.len);
        }
        const size_t need = ptls_hip_tls13_frame(msgs.data(), msgs.size(), nullptr, 0);
        const size_t cap = need == 0 ? 0 : rng() % (need + 1);
        std::vector<ptls_hip_record_t> recs(cap);
        CHECK(ptls_hip_tls13_frame(msgs.data(), msgs.size(), cap ? recs.data() : nullptr, cap) == need);
        uint64_t wire_end = 0;
        for (size_t k = 0; k < cap; ++k)
            wire_end = std::max<uint64_t>(wire_end, recs[k].out_off + recs[k].len + 16);
        CHECK(wire_end <= out);
    }
}

static void check_planner(std::mt19937_64 &rng, int sets)
{
    std::vector<Chunk> ch;
    std::vector<uint32_t> order;
    for (int s = 0; s < sets; ++s) {
        const size_t n = rng() % 3000;
        std::vector<ptls_hip_record_t> recs(n);
        uint32_t key = 0;
        for (size_t i = 0; i < n; ++i) {
            if (rng() % (1 + rng() % 200) == 0)
                key = (uint32_t)(rng() % 70000);
            recs[i] = ptls_hip_record_t{};
            recs[i].len = (uint32_t)(rng() % 4 == 0 ? rng() % 16385 : rng() % 1400);
            recs[i].aad_len = (uint32_t)(rng() % 40);
            recs[i].in_off = rng() % (1u << 30);
            recs[i].out_off = rng() % (1u << 30);
            recs[i].aad_off = rng() % (1u << 20);
            recs[i].key = key;
        }
        /* three sets in four have every offset on a multiple of 16, one of those but a single offset of one record */
        if (s % 4 != 0)
            for (auto &r : recs)
                r.in_off &= ~15ull, r.out_off &= ~15ull, r.aad_off &= ~15ull;
        if (s % 4 == 1 && n != 0) {
            ptls_hip_record_t &r = recs[rng() % n];
            (rng() % 3 == 0 ? r.in_off : rng() % 2 == 0 ? r.out_off : r.aad_off) |= 1 + rng() % 15;
        }
        const unsigned ncu = 1 + (unsigned)(rng() % 300);
        /* offsets_aligned is what build_chunks reports, for a batch-kernel lane count and for the sparse form */
        for (const int l : {4, (int)SPARSE_LANES}) {
            bool al = !offsets_aligned(recs.data(), n);
            build_chunks(recs.data(), n, l, ncu, ch, order, al);
            CHECK(al == offsets_aligned(recs.data(), n));
            CHECK(al == (n == 0 || (s % 4 != 0 && s % 4 != 1)));
        }
        const int lanes = choose_lanes(recs.data(), n, ncu);
        CHECK(lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == SPARSE_LANES);
        bool aligned = false;
        build_chunks(recs.data(), n, lanes, ncu, ch, order, aligned);
        std::vector<uint8_t> seen(n, 0);
        size_t covered = 0;
        for (const Chunk &c : ch) {
            CHECK((size_t)c.first + c.count <= n);
            for (uint32_t t = c.first; t < c.first + c.count && t < n; ++t) {
                CHECK(order[t] < n);
                if (order[t] < n) {
                    CHECK(!seen[order[t]]);
                    seen[order[t]] = 1;
                    CHECK(lanes == SPARSE_LANES || recs[order[t]].key == c.key);
                }
            }
            covered += c.count;
        }
        CHECK(covered == n);
        CHECK(plan_grid(n, ch.size(), lanes, ncu) <= std::max<unsigned>(ncu, 1));
    }
}

static void check_partition(std::mt19937_64 &rng, int sets)
{
    for (int s = 0; s < sets; ++s) {
        const size_t n = rng() % 500, parts = 1 + rng() % 12;
        std::vector<ptls_hip_record_t> recs(n);
        for (auto &r : recs) {
            r = ptls_hip_record_t{};
            r.len = (uint32_t)(rng() % 3 == 0 ? 0 : rng() % 20000);
        }
        std::vector<size_t> b(parts + 1, ~(size_t)0);
        CHECK(ptls_hip_partition_bytes(n ? recs.data() : nullptr, n, parts, b.data()) == 0);
        CHECK(b[0] == 0 && b[parts] == n);
        for (size_t p = 0; p < parts; ++p)
            CHECK(b[p] <= b[p + 1]);
    }
    size_t b[3];
    CHECK(ptls_hip_partition_bytes(nullptr, 5, 2, b) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_partition_bytes(nullptr, 0, 0, b) == PTLS_HIP_EINVAL);
}

/* ---- the copy transport's slice plans (slice_plan.cpp): what the host places where ---- */

/* a random record list like pipeline_trial's: records of 0-2 000 bytes, 1-64-byte gaps in the output (`holes`: now and
 * then one of GAP_SPLIT or more), in output order or shuffled, the AAD where the mode keeps it */
struct Layout {
    std::vector<ptls_hip_record_t> recs;
    std::vector<ptls_hip_supp_t> supp;
    uint64_t out_sz;
};

static Layout random_layout(std::mt19937_64 &rng, size_t n, PipeMode mode, bool shuffled, bool holes, int mask_layout, size_t hp_nslots,
                            uint32_t max_len = 2000)
{
    const ModeInfo m(mode);
    Layout L;
    L.recs.resize(n);
    uint64_t in = 0, out = 0, aad = 0;
    for (size_t i = 0; i < n; ++i) {
        ptls_hip_record_t &r = L.recs[i] = ptls_hip_record_t{};
        r.len = (uint32_t)(rng() % (max_len + 1));
        r.seq = 1000 + i;
        r.key = (uint32_t)((i * 3) / n);
        in += rng() % 4;
        out += 1 + rng() % 64 + (holes && rng() % 50 == 0 ? GAP_SPLIT + rng() % 4096 : 0);
        if (m.aad_in_out || m.aad_in_in) { /* the 5-byte header in front of the record, on the wire side */
            uint64_t &wire = m.aad_in_out ? out : in;
            r.aad_off = wire;
            r.aad_len = 5;
            wire += 5;
        } else {
            r.aad_off = aad + rng() % 4;
            r.aad_len = (uint32_t)(rng() % 41);
            aad = r.aad_off + r.aad_len;
        }
        r.in_off = in;
        r.out_off = out;
        in += r.len + m.tag_in;
        out += r.len + m.tag_out;
    }
    L.out_sz = out + 1 + rng() % 64;
    if (mask_layout >= 0) { /* masks packed in record order / packed in reverse / strided at odd offsets */
        L.supp.resize(n);
        for (size_t i = 0; i < n; ++i) {
            ptls_hip_supp_t &sp = L.supp[i] = ptls_hip_supp_t{};
            sp.flags = rng() % 4 != 0 ? PTLS_HIP_SUPP_ENABLE : 0;
            sp.hp_key = (uint32_t)(rng() % (hp_nslots + 2)); /* some outside the keyset: skipped by the kernel */
            sp.sample_off = L.recs[i].out_off + rng() % (L.recs[i].len + 1);
            sp.mask_off = mask_layout == 0 ? 16 * i : mask_layout == 1 ? 16 * (n - 1 - i) : 48 * i + 7;
        }
    }
    if (shuffled) {
        std::vector<size_t> perm(n);
        for (size_t i = 0; i < n; ++i)
            perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        Layout S = L;
        for (size_t k = 0; k < n; ++k) {
            S.recs[k] = L.recs[perm[k]];
            if (!L.supp.empty())
                S.supp[k] = L.supp[perm[k]];
        }
        return S;
    }
    return L;
}

/* the output byte ranges of a record, from the mode's definition */
static std::vector<Span> out_parts(const ptls_hip_record_t &r, const ModeInfo &m)
{
    std::vector<Span> v;
    if (m.aad_in_out && r.aad_len != 0)
        v.push_back(Span{r.aad_off, r.aad_off + r.aad_len});
    if (r.len + m.tag_out != 0)
        v.push_back(Span{r.out_off, r.out_off + r.len + m.tag_out});
    return v;
}

/* the spans records [a, b) need in the input, output and AAD staging */
static void staged_spans(const std::vector<ptls_hip_record_t> &recs, size_t a, size_t b, const ModeInfo &m, Span &in, Span &out, Span &ad)
{
    in = out = ad = Span{UINT64_MAX, 0};
    auto add = [](Span &s, uint64_t lo, uint64_t hi) { s = Span{std::min(s.lo, lo), std::max(s.hi, hi)}; };
    for (size_t t = a; t < b; ++t) {
        const ptls_hip_record_t &r = recs[t];
        add(in, r.in_off, r.in_off + r.len + m.tag_in);
        add(out, r.out_off, r.out_off + r.len + m.tag_out);
        add(m.aad_in_out ? out : m.aad_in_in ? in : ad, r.aad_off, r.aad_off + r.aad_len);
    }
}

static bool writes_a_mask(const ptls_hip_supp_t &sp, size_t hp_nslots)
{
    return (sp.flags & PTLS_HIP_SUPP_ENABLE) && sp.hp_key < hp_nslots;
}

/* plans every slice of the layout and checks the eight properties of a plan (numbered as in the comments) */
static void check_layout_plans(const Layout &L, PipeMode mode, size_t slice_bytes, size_t hp_nslots)
{
    const ModeInfo m(mode);
    const std::vector<ptls_hip_record_t> &recs = L.recs;
    const ptls_hip_supp_t *supp = L.supp.empty() ? nullptr : L.supp.data();
    const size_t n = recs.size(), max_recs = slice_bytes / 16 + 1;
    CopyOrder ord;
    plan_copy_order(recs.data(), n, m, ord);
    std::vector<SlicePlan> plans;
    std::vector<size_t> first;
    /* owner[b]: 1 + the slice whose record writes output byte b (the layout's records do not overlap), 0: a gap */
    std::vector<uint32_t> owner(L.out_sz, 0);
    for (size_t i = 0; i < n;) {
        SlicePlan pl;
        const int rc = plan_copy_slice(recs.data(), supp, n, i, m, slice_bytes, max_recs, hp_nslots, ord, pl);
        CHECK(rc == 0);
        /* 1. the slices partition [0, n) in order and none is empty */
        CHECK(rc == 0 && pl.j > i && pl.j <= n);
        if (rc != 0 || pl.j <= i || pl.j > n)
            return;
        const size_t j = pl.j, cnt = j - i;
        /* 2. the staged spans are the records', and within the limits */
        Span in, out, ad;
        staged_spans(recs, i, j, m, in, out, ad);
        CHECK(pl.in.lo == in.lo && pl.in.hi == in.hi && pl.out.lo == out.lo && pl.out.hi == out.hi);
        CHECK(ad.hi > ad.lo ? pl.aad.lo == ad.lo && pl.aad.hi == ad.hi : pl.aad.lo == 0 && pl.aad.hi == 0);
        CHECK(pl.in.hi - pl.in.lo <= slice_bytes && pl.out.hi - pl.out.lo <= slice_bytes && pl.aad.hi - pl.aad.lo <= slice_bytes / 4);
        size_t nmask = 0;
        for (size_t t = i; supp != nullptr && t < j; ++t)
            nmask += writes_a_mask(supp[t], hp_nslots);
        CHECK(nmask <= slice_bytes / 64 && pl.mask_dst.size() == nmask && cnt <= max_recs - 1);
        /* 3. the cut is the greedy one: the next record would break a limit */
        if (j < n) {
            staged_spans(recs, i, j + 1, m, in, out, ad);
            CHECK(cnt == max_recs - 1 || (supp != nullptr && writes_a_mask(supp[j], hp_nslots) && nmask == slice_bytes / 64) ||
                  in.hi - in.lo > slice_bytes || out.hi - out.lo > slice_bytes || (ad.hi > ad.lo && ad.hi - ad.lo > slice_bytes / 4));
        }
        /* 6. the slice-local descriptors are the caller's minus the bases, and the bases keep the alignment */
        CHECK(pl.in_base % 16 == 0 && pl.out_base % 16 == 0 && pl.aad_base % 16 == 0);
        CHECK(pl.in_base <= pl.in.lo && pl.in.lo - pl.in_base < 16 && pl.out_base <= pl.out.lo && pl.out.lo - pl.out_base < 16 &&
              pl.aad_base <= pl.aad.lo && pl.aad.lo - pl.aad_base < 16);
        CHECK(pl.recs.size() == cnt && pl.supp.size() == (supp != nullptr ? cnt : 0));
        for (size_t t = 0; t < cnt && t < pl.recs.size(); ++t) {
            const ptls_hip_record_t &a = pl.recs[t], &b = recs[i + t];
            CHECK(a.in_off + pl.in_base == b.in_off && a.out_off + pl.out_base == b.out_off);
            CHECK(a.aad_off + (m.aad_in_out ? pl.out_base : m.aad_in_in ? pl.in_base : pl.aad_base) == b.aad_off);
            CHECK(a.seq == b.seq && a.len == b.len && a.aad_len == b.aad_len && a.key == b.key && a.flags == b.flags);
        }
        /* 7. the mask places: in record order, exactly the masks the kernel writes, packed 16 bytes apart */
        for (size_t t = 0, k = 0; t < pl.supp.size(); ++t) {
            const ptls_hip_supp_t &a = pl.supp[t], &b = supp[i + t];
            CHECK(a.flags == b.flags && a.hp_key == b.hp_key);
            if (!(b.flags & PTLS_HIP_SUPP_ENABLE)) {
                CHECK(a.sample_off == b.sample_off && a.mask_off == b.mask_off);
                continue;
            }
            CHECK(a.sample_off + pl.out_base == b.sample_off);
            if (writes_a_mask(b, hp_nslots)) {
                CHECK(k < pl.mask_dst.size() && pl.mask_dst[k] == b.mask_off && a.mask_off == 16 * k);
                ++k;
            }
        }
        for (size_t t = i; t < j; ++t)
            for (const Span &s : out_parts(recs[t], m))
                std::fill(owner.begin() + s.lo, owner.begin() + s.hi, (uint32_t)plans.size() + 1);
        first.push_back(i);
        plans.push_back(std::move(pl));
        i = j;
    }
    std::vector<uint8_t> gapmark(L.out_sz, 0);
    for (size_t k = 0; k < plans.size(); ++k) {
        const SlicePlan &pl = plans[k];
        /* the slice's runs: its records' output parts, merged where they touch */
        std::vector<Span> parts;
        uint64_t part_bytes = 0, gap_bytes = 0;
        for (size_t t = first[k]; t < pl.j; ++t)
            for (const Span &s : out_parts(recs[t], m)) {
                parts.push_back(s);
                part_bytes += s.hi - s.lo;
            }
        std::sort(parts.begin(), parts.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
        size_t nruns = 0;
        for (size_t t = 0; t < parts.size(); ++t)
            nruns += t == 0 || parts[t].lo > parts[t - 1].hi;
        /* 5. every gap: short, no record's output (this slice's or another's), none at all with few runs, sources packed */
        CHECK(pl.gaps.size() == pl.gap_src.size() && (nruns > COPY_DIRECT_RUNS || pl.gaps.empty()));
        CHECK(pl.pieces.size() + pl.gaps.size() == nruns);
        for (size_t t = 0; t < pl.gaps.size() && t < pl.gap_src.size(); ++t) {
            const GapPiece &g = pl.gaps[t];
            const Span &src = pl.gap_src[t];
            CHECK(g.len != 0 && g.len < GAP_SPLIT && g.src == gap_bytes && g.dst + pl.out_base == src.lo && src.hi - src.lo == g.len);
            CHECK(src.lo >= pl.out.lo && src.hi <= pl.out.hi);
            for (uint64_t b = src.lo; b < src.hi && b < L.out_sz; ++b) {
                CHECK(owner[b] == 0 && gapmark[b] == 0);
                gapmark[b] = 1;
            }
            gap_bytes += g.len;
        }
        /* 4. the pieces: sorted, disjoint, inside the out span; they cover every output part, and beyond those the gaps */
        uint64_t seen_parts = 0, seen_gaps = 0;
        for (size_t t = 0; t < pl.pieces.size(); ++t) {
            const Span &pc = pl.pieces[t];
            CHECK(pc.lo < pc.hi && pc.lo >= pl.out.lo && pc.hi <= pl.out.hi && (t == 0 || pc.lo > pl.pieces[t - 1].hi));
            for (uint64_t b = pc.lo; b < pc.hi && b < L.out_sz; ++b) {
                CHECK(owner[b] == k + 1 || gapmark[b] == 1);
                seen_parts += owner[b] == k + 1;
                seen_gaps += gapmark[b];
            }
            /* the copy splits only where it must: few runs, a long gap, or another slice's record in the gap */
            if (t != 0 && nruns > COPY_DIRECT_RUNS && pc.lo - pl.pieces[t - 1].hi < GAP_SPLIT) {
                bool other = false;
                for (uint64_t b = pl.pieces[t - 1].hi; b < pc.lo; ++b)
                    other = other || owner[b] != 0;
                CHECK(other);
            }
        }
        CHECK(seen_parts == part_bytes && seen_gaps == gap_bytes);
        for (const Span &src : pl.gap_src)
            std::fill(gapmark.begin() + std::min<uint64_t>(src.lo, L.out_sz), gapmark.begin() + std::min<uint64_t>(src.hi, L.out_sz), 0);
    }
}

/* 8. the two refusals, with the offending record in the first slice and in a later one */
static void check_plan_refusals(void)
{
    const size_t slice = 64 << 10, max_recs = slice / 16 + 1;
    CopyOrder ord;
    SlicePlan pl;
    for (size_t bad : {(size_t)0, (size_t)2}) {
        /* three 40 000-byte records, one slice each; record `bad` is larger than a slice */
        std::vector<ptls_hip_record_t> recs(3, ptls_hip_record_t{});
        uint64_t in = 0, out = 0;
        for (size_t t = 0; t < 3; ++t) {
            recs[t].len = t == bad ? (uint32_t)slice : 40000;
            recs[t].in_off = in;
            recs[t].out_off = out;
            in += recs[t].len;
            out += recs[t].len + 16;
        }
        plan_copy_order(recs.data(), 3, PIPE_SEAL, ord);
        for (size_t i = 0; i < 3; ++i) {
            const int rc = plan_copy_slice(recs.data(), nullptr, 3, i, PIPE_SEAL, slice, max_recs, 0, ord, pl);
            if (i == bad) {
                CHECK(rc == PTLS_HIP_EINVAL && std::strstr(ptls_hip_last_error(), "does not fit a 65536-byte slice") != nullptr);
                break;
            }
            CHECK(rc == 0 && pl.j == i + 1);
        }
        /* the same list with every record fitting, and the sample of record `bad` outside its slice's output */
        recs[bad].len = 40000;
        std::vector<ptls_hip_supp_t> supp(3, ptls_hip_supp_t{});
        for (size_t t = 0; t < 3; ++t) {
            recs[t].out_off = t * 40100;
            supp[t].flags = PTLS_HIP_SUPP_ENABLE;
            supp[t].sample_off = recs[t].out_off + (t == bad ? 40016 - 15 : 4);
            supp[t].mask_off = 16 * t;
        }
        plan_copy_order(recs.data(), 3, PIPE_SEAL, ord);
        for (size_t i = 0; i < 3; ++i) {
            const int rc = plan_copy_slice(recs.data(), supp.data(), 3, i, PIPE_SEAL, slice, max_recs, 1, ord, pl);
            if (i == bad) {
                CHECK(rc == PTLS_HIP_EINVAL && std::strstr(ptls_hip_last_error(), "outside the slice's output") != nullptr);
                break;
            }
            CHECK(rc == 0 && pl.j == i + 1);
        }
    }
}

static void check_slice_plans(std::mt19937_64 &rng, int layouts)
{
    static const PipeMode modes[] = {PIPE_SEAL, PIPE_OPEN, PIPE_TLS13_SEAL, PIPE_TLS13_OPEN};
    for (int l = 0; l < layouts; ++l) {
        const PipeMode mode = modes[l % 4];
        const size_t n = l % 5 == 0 ? 5 : 1 + rng() % 400, hp_nslots = 1 + rng() % 3;
        /* header-protection descriptors go with a plain seal only (pipeline_run), in three mask layouts */
        const int mask_layout = mode == PIPE_SEAL && rng() % 4 != 0 ? (int)(rng() % 3) : -1;
        const Layout L = random_layout(rng, n, mode, rng() % 2 != 0, rng() % 4 == 0, mask_layout, hp_nslots);
        check_layout_plans(L, mode, l % 2 ? (size_t)1 << 20 : (size_t)64 << 10, hp_nslots);
    }
    /* many tiny records, each with a mask: the mask staging (slice_bytes / 64 masks) ends the slices, not the bytes */
    Layout tiny = random_layout(rng, 6000, PIPE_SEAL, false, false, 0, 8, 8);
    for (ptls_hip_supp_t &sp : tiny.supp) {
        sp.flags = PTLS_HIP_SUPP_ENABLE;
        sp.hp_key %= 8;
    }
    check_layout_plans(tiny, PIPE_SEAL, 64 << 10, 8);
    check_plan_refusals();
}

/* the C ABI's argument checks and the no-device paths: each must fail with an error code and a message, never crash */
static void check_abi_without_device(void)
{
    CHECK(ptls_hip_is_supported() == 0);
    CHECK(ptls_hip_engine_new(0) == nullptr && std::strlen(ptls_hip_last_error()) != 0);
    CHECK(ptls_hip_engine_new(-1) == nullptr);
    CHECK(ptls_hip_keyset_new(nullptr, 16, 4) == nullptr);
    CHECK(ptls_hip_batch_new(nullptr, nullptr, 0, nullptr) == nullptr);
    CHECK(ptls_hip_pipeline_new(nullptr, 1 << 20) == nullptr);
    const int dev[1] = {0};
    CHECK(ptls_hip_node_new(nullptr, 1, 16, 1, 1 << 20) == nullptr);
    CHECK(ptls_hip_node_new(dev, 1, 16, 1, 1 << 20) == nullptr);
    CHECK(ptls_hip_keyset_set(nullptr, 0, 1, "k", nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_keyset_set_secrets(nullptr, 0, 1, "s", 32, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_keyset_get_iv(nullptr, 0, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_batch_set_lanes(nullptr, 3) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_batch_set_clock(nullptr, nullptr, 0) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_aesgcm_seal_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_aesgcm_open_batch(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_aesecb_batch(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_tls13_seal_batch(nullptr, nullptr, nullptr, nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_pipeline_set_transport(nullptr, 0) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_pipeline_seal(nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_device_copy(nullptr, nullptr, nullptr, 16, nullptr) == PTLS_HIP_EINVAL);
    CHECK(ptls_hip_fill_records(nullptr, nullptr, 0, 0, nullptr, nullptr) == PTLS_HIP_EINVAL);
    /* the plugin without a device: setup_crypto fails (ptls_aead_new returns NULL), no CPU fallback */
    static const uint8_t key[32] = {0}, iv[12] = {0};
    for (ptls_aead_algorithm_t *a : {&ptls_hip_aes128gcm, &ptls_hip_aes256gcm, &ptls_hip_non_temporal_aes128gcm}) {
        std::vector<uint8_t> ctx(a->context_size, 0);
        auto *c = reinterpret_cast<ptls_aead_context_t *>(ctx.data());
        c->algo = a;
        CHECK(a->setup_crypto(c, 1, key, iv) != 0);
        /* the IV-only setup of a fresh context needs no device (fusion: lib/fusion.c:1188-1191) */
        std::vector<uint8_t> ctx2(a->context_size, 0);
        auto *c2 = reinterpret_cast<ptls_aead_context_t *>(ctx2.data());
        c2->algo = a;
        CHECK(a->setup_crypto(c2, 1, nullptr, iv) == 0 && c2->dispose_crypto != nullptr);
        uint8_t got[12];
        c2->do_get_iv(c2, got);
        CHECK(std::memcmp(got, iv, 12) == 0);
        c2->dispose_crypto(c2);
    }
    ptls_hip_aesecb_context_t ecb;
    CHECK(ptls_hip_aesecb_init(&ecb, 1, key, 16, 0) == PTLS_HIP_ENODEV && ecb.state == nullptr);
    CHECK(ptls_hip_aesecb_init(&ecb, 0, key, 16, 0) == PTLS_HIP_EINVAL);
    ptls_hip_aesecb_dispose(&ecb);
    CHECK(ptls_hip_aesgcm_new(key, 16, 1500) == nullptr);
    CHECK(ptls_hip_aesgcm_new(key, 24, 1500) == nullptr);
}

/* one pipeline seal + open over a random layout; returns false (and counts failures) on a mismatch */
static void pipeline_trial(std::mt19937_64 &rng, ptls_hip_pipeline_t *pipe, ptls_hip_keyset_t *ks, size_t key_size,
                           const std::vector<uint8_t> &keys, const std::vector<uint8_t> &ivs, int transport)
{
    const size_t n = 1 + rng() % 160;
    std::vector<uint32_t> len(n), alen(n), key(n);
    std::vector<uint64_t> in_off(n), out_off(n), aad_off(n), pt_off(n);
    size_t in_sz = 0, out_sz = 0, aad_sz = 0, pt_sz = 0;
    for (size_t i = 0; i < n; ++i) {
        len[i] = (uint32_t)(rng() % 8 == 0 ? rng() % 16385 : rng() % 3000);
        alen[i] = (uint32_t)(rng() % 41);
        key[i] = (uint32_t)((i * 3) / n);
        in_off[i] = in_sz + rng() % 4;
        in_sz = in_off[i] + len[i];
        aad_off[i] = aad_sz + rng() % 4;
        aad_sz = aad_off[i] + alen[i];
        out_off[i] = out_sz + 1 + rng() % 64;
        out_sz = out_off[i] + len[i] + 16;
        pt_off[i] = pt_sz + 1 + rng() % 64;
        pt_sz = pt_off[i] + len[i];
    }
    out_sz += 1 + rng() % 64;
    pt_sz += 1 + rng() % 64;
    const bool pinned = transport == PTLS_HIP_TRANSPORT_MAPPED;
    /* exactly-sized buffers: heap (ASan-checked) for COPY, pinned for MAPPED */
    auto alloc = [&](size_t sz) -> uint8_t * {
        void *p = nullptr;
        if (pinned) {
            if (hipHostMalloc(&p, sz ? sz : 1, hipHostMallocDefault) != hipSuccess)
                return nullptr;
        } else {
            p = malloc(sz ? sz : 1);
        }
        return static_cast<uint8_t *>(p);
    };
    auto release = [&](uint8_t *p) {
        if (pinned)
            (void)hipHostFree(p);
        else
            free(p);
    };
    uint8_t *h_in = alloc(in_sz), *h_aad = alloc(aad_sz), *h_out = alloc(out_sz), *h_pt = alloc(pt_sz);
    CHECK(h_in && h_aad && h_out && h_pt);
    if (!(h_in && h_aad && h_out && h_pt))
        return;
    for (size_t i = 0; i < in_sz; ++i)
        h_in[i] = (uint8_t)rng();
    for (size_t i = 0; i < aad_sz; ++i)
        h_aad[i] = (uint8_t)rng();
    memset(h_out, 0xA5, out_sz);
    memset(h_pt, 0x5A, pt_sz);
    /* descriptors, in output order or shuffled */
    std::vector<size_t> perm(n);
    for (size_t i = 0; i < n; ++i)
        perm[i] = i;
    if (rng() % 2)
        std::shuffle(perm.begin(), perm.end(), rng);
    std::vector<ptls_hip_record_t> rs(n), ro(n);
    for (size_t k = 0; k < n; ++k) {
        const size_t i = perm[k];
        rs[k] = ptls_hip_record_t{in_off[i], out_off[i], aad_off[i], 1000 + i, len[i], alen[i], key[i], 0};
        ro[k] = ptls_hip_record_t{out_off[i], pt_off[i], aad_off[i], 1000 + i, len[i], alen[i], key[i], 0};
    }
    CHECK(ptls_hip_pipeline_set_transport(pipe, transport) == 0);
    int rc = ptls_hip_pipeline_seal(pipe, ks, rs.data(), n, h_in, h_aad, h_out);
    CHECK(rc == 0);
    std::vector<uint8_t> exp;
    std::vector<uint8_t> touched(out_sz, 0);
    for (size_t i = 0; rc == 0 && i < n; ++i) {
        exp.resize(len[i] + 16);
        oracle_aesgcm_seal(&keys[key[i] * key_size], key_size, &ivs[key[i] * 12], 1000 + i, h_aad + aad_off[i], alen[i],
                           h_in + in_off[i], len[i], exp.data());
        CHECK(memcmp(h_out + out_off[i], exp.data(), len[i] + 16) == 0);
        memset(&touched[out_off[i]], 1, len[i] + 16);
    }
    for (size_t b = 0; b < out_sz; ++b)
        if (!touched[b] && h_out[b] != 0xA5) {
            CHECK(!"seal wrote a byte between records");
            break;
        }
    CHECK(ptls_hip_pipeline_last_transport(pipe) == transport);
    std::vector<uint64_t> res(n, 0);
    uint64_t *h_res = res.data();
    void *pres = nullptr;
    if (pinned && hipHostMalloc(&pres, n * 8, hipHostMallocDefault) == hipSuccess)
        h_res = static_cast<uint64_t *>(pres);
    rc = ptls_hip_pipeline_open(pipe, ks, ro.data(), n, h_out, h_aad, h_pt, h_res);
    CHECK(rc == 0);
    std::vector<uint8_t> ptouched(pt_sz, 0);
    for (size_t k = 0; rc == 0 && k < n; ++k) {
        const size_t i = perm[k];
        CHECK(h_res[k] == len[i]);
        CHECK(memcmp(h_pt + pt_off[i], h_in + in_off[i], len[i]) == 0);
        memset(&ptouched[pt_off[i]], 1, len[i]);
    }
    for (size_t b = 0; b < pt_sz; ++b)
        if (!ptouched[b] && h_pt[b] != 0x5A) {
            CHECK(!"open wrote a byte between records");
            break;
        }
    if (pres != nullptr)
        (void)hipHostFree(pres);
    release(h_in);
    release(h_aad);
    release(h_out);
    release(h_pt);
}

static void check_pipelines_on_device(std::mt19937_64 &rng, int trials)
{
    ptls_hip_engine_t *eng = ptls_hip_engine_new(0);
    if (eng == nullptr) {
        printf("host_check: no usable gfx950 device (%s): device paths skipped\n", ptls_hip_last_error());
        return;
    }
    for (size_t key_size : {(size_t)16, (size_t)32}) {
        std::vector<uint8_t> keys(3 * key_size), ivs(3 * 12);
        for (auto &b : keys)
            b = (uint8_t)rng();
        for (auto &b : ivs)
            b = (uint8_t)rng();
        ptls_hip_keyset_t *ks = ptls_hip_keyset_new(eng, key_size, 3);
        CHECK(ks != nullptr && ptls_hip_keyset_set(ks, 0, 3, keys.data(), ivs.data(), nullptr) == 0);
        for (size_t slice : {(size_t)64 << 10, (size_t)1 << 20}) {
            ptls_hip_pipeline_t *pipe = ptls_hip_pipeline_new(eng, slice);
            CHECK(pipe != nullptr);
            for (int t = 0; pipe != nullptr && t < trials; ++t)
                pipeline_trial(rng, pipe, ks, key_size, keys, ivs, t % 2 ? PTLS_HIP_TRANSPORT_COPY : PTLS_HIP_TRANSPORT_MAPPED);
            ptls_hip_pipeline_free(pipe);
        }
        ptls_hip_keyset_free(ks);
    }
    ptls_hip_engine_free(eng);
    printf("host_check: device paths run (%d trials x 2 key sizes x 2 slice sizes)\n", trials);
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "device") == 0) { /* the GPU box: the pipelines under the sanitizers */
        std::mt19937_64 rng(0x70697065ull);
        check_pipelines_on_device(rng, argc > 2 ? atoi(argv[2]) : 40);
        printf("host_check: %s (%d failed checks)\n", failures == 0 ? "ok" : "FAILED", failures);
        return failures == 0 ? 0 : 1;
    }
    const int scale = argc > 1 ? atoi(argv[1]) : 1;
    std::mt19937_64 rng(0x68737467ull);
    check_parse(rng, 100000 * scale);
    check_frame(rng, 20000 * scale);
    check_planner(rng, 300 * scale);
    check_partition(rng, 20000 * scale);
    check_slice_plans(rng, 1000 * scale);
    check_abi_without_device();
    printf("host_check: %s (%d failed checks)\n", failures == 0 ? "ok" : "FAILED", failures);
    return failures == 0 ? 0 : 1;
}
