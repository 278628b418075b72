/*
 * slice_plan.cpp -- the copy transport's planning (pipeline.cpp): where a slice of the record list ends, its slice-local
 * descriptors, the copies that bring its output back, the gaps filled under those copies and the places of its masks.
 * Arithmetic on descriptors only, no HIP call: tests/host_check/host_check.cpp checks it on the CPU.
 *
 * The output is exactly the records' bytes.  A slice's records are written into device staging and
 * come back by D2H copies.  Copying back the slice's whole output span would also write, into the caller's buffer,
 * whatever the staging held between the records (another call's plaintext); fusion writes exactly the record's bytes
 * (storen128 and the tag store, lib/fusion.c:388-397, :632).  So the output comes back as the records' merged runs: each
 * run by its own copy when a slice has few runs or a gap is long (COPY_DIRECT_RUNS, GAP_SPLIT), and otherwise several
 * runs by one copy, their gaps first filled in the staging with the caller's own bytes of those gaps (gathered on the
 * host into pinned memory, one upload, gap_scatter_kernel).  A gap is never filled when another slice's record writes
 * into it (records not in output order): the copy splits there.
 *
 * The masks are exactly the records' 16 bytes.  h_mask belongs to every slice of the call at once: mask offsets are the
 * caller's choice, so the masks of different slices may interleave.  A slice therefore neither uploads nor copies back a
 * span of h_mask (bytes of another slice's masks in that span would come back stale, whenever that slice delivered them
 * in between: slices overlap on pinned buffers).  The kernel writes the slice's masks packed into d_mask (slice-local
 * mask_off = 16 x the mask's index among the slice's enabled descriptors with a valid hp_key; the others are skipped by
 * the kernel and have no place there), ONE copy brings them into the slot's pinned h_mask, and the host places each at
 * the caller's mask_off when it has waited for the slice (16 bytes per packet, next to the planning the host does per
 * record anyway).  So the number of copies per slice does not depend on the layout of the masks, no byte of h_mask other
 * than those masks is read or written, and a slice's masks may lie anywhere in h_mask.
 */
#include <algorithm>

#include "host.h"

/* the output byte ranges of record r (its ciphertext + tag or plaintext, and a TLS 1.3 header the device writes) */
static void record_out_parts(const ptls_hip_record_t &r, const ModeInfo &m, std::vector<Span> &v)
{
    if (m.aad_in_out && r.aad_len != 0)
        v.push_back(Span{r.aad_off, r.aad_off + r.aad_len});
    const uint64_t len = (uint64_t)r.len + m.tag_out;
    if (len != 0)
        v.push_back(Span{r.out_off, r.out_off + len});
}

/* sort (unless already in order) and merge touching or overlapping ranges */
static void merge_spans(std::vector<Span> &v)
{
    bool sorted = true;
    for (size_t t = 1; t < v.size() && sorted; ++t)
        sorted = v[t].lo >= v[t - 1].lo;
    if (!sorted)
        std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) { return a.lo < b.lo; });
    size_t k = 0;
    for (size_t t = 0; t < v.size(); ++t) {
        if (k != 0 && v[t].lo <= v[k - 1].hi)
            v[k - 1].hi = std::max(v[k - 1].hi, v[t].hi);
        else
            v[k++] = v[t];
    }
    v.resize(k);
}

/* some range of `uni` (sorted, merged) intersects [lo, hi) */
static bool spans_hit(const std::vector<Span> &uni, uint64_t lo, uint64_t hi)
{
    auto it = std::upper_bound(uni.begin(), uni.end(), lo, [](uint64_t x, const Span &s) { return x < s.hi; });
    return it != uni.end() && it->lo < hi;
}

void plan_copy_order(const ptls_hip_record_t *recs, size_t n, const ModeInfo &m, CopyOrder &o)
{
    o.in_order = true;
    for (size_t t = 0, prev_hi = 0; t < n && o.in_order; ++t) {
        o.uni.clear();
        record_out_parts(recs[t], m, o.uni);
        for (const Span &r : o.uni) {
            o.in_order = o.in_order && r.lo >= prev_hi;
            prev_hi = std::max<uint64_t>(prev_hi, r.hi);
        }
    }
    o.uni.clear();
    if (!o.in_order) {
        for (size_t t = 0; t < n; ++t)
            record_out_parts(recs[t], m, o.uni);
        merge_spans(o.uni);
    }
}

/* a mask the kernel will write (it skips disabled descriptors and hp keys outside the keyset) */
static bool writes_mask(const ptls_hip_supp_t &sp, size_t hp_nslots)
{
    return (sp.flags & PTLS_HIP_SUPP_ENABLE) && sp.hp_key < hp_nslots;
}

int plan_copy_slice(const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n, size_t i, const ModeInfo &m,
                    size_t slice_bytes, size_t max_recs, size_t hp_nslots, const CopyOrder &o, SlicePlan &pl)
{
    /* grow the slice while every span fits the staging buffers */
    Span in{UINT64_MAX, 0}, out{UINT64_MAX, 0}, ad{UINT64_MAX, 0};
    size_t j = i, nmask = 0;
    while (j < n && j - i < max_recs - 1) {
        const ptls_hip_record_t &r = recs[j];
        const bool masked = supp != nullptr && writes_mask(supp[j], hp_nslots);
        if (masked && nmask == slot_max_masks(slice_bytes))
            break; /* the mask staging is full (nmask != 0, so j > i) */
        Span ni{std::min(in.lo, r.in_off), std::max(in.hi, r.in_off + r.len + m.tag_in)};
        Span no{std::min(out.lo, r.out_off), std::max(out.hi, r.out_off + r.len + m.tag_out)};
        Span na{std::min(ad.lo, r.aad_off), std::max(ad.hi, r.aad_off + r.aad_len)};
        if (m.aad_in_out) { /* the header is part of the output span */
            no = Span{std::min(no.lo, r.aad_off), std::max(no.hi, r.aad_off + r.aad_len)};
            na = Span{UINT64_MAX, 0};
        } else if (m.aad_in_in) { /* the header is part of the input span */
            ni = Span{std::min(ni.lo, r.aad_off), std::max(ni.hi, r.aad_off + r.aad_len)};
            na = Span{UINT64_MAX, 0};
        }
        if (j > i && (ni.hi - ni.lo > slice_bytes || no.hi - no.lo > slice_bytes || na.hi - na.lo > slice_bytes / 4))
            break;
        in = ni;
        out = no;
        ad = na;
        nmask += masked;
        ++j;
    }
    if (in.hi - in.lo > slice_bytes || out.hi - out.lo > slice_bytes || (ad.hi > ad.lo && ad.hi - ad.lo > slice_bytes / 4))
        return fail(PTLS_HIP_EINVAL, "pipeline: record %zu does not fit a %zu-byte slice", i, slice_bytes);
    if (ad.hi <= ad.lo)
        ad = Span{0, 0};
    /* header protection: every enabled sample must lie in the slice's output */
    for (size_t t = i; supp != nullptr && t < j; ++t)
        if ((supp[t].flags & PTLS_HIP_SUPP_ENABLE) && (supp[t].sample_off < out.lo || supp[t].sample_off + 16 > out.hi))
            return fail(PTLS_HIP_EINVAL, "pipeline_seal_supp: sample of record %zu is outside the slice's output", t);
    pl.j = j;
    pl.in = in;
    pl.out = out;
    pl.aad = ad;
    /* slice-local descriptors keep the same relative 16-byte alignment as the caller's buffers */
    pl.in_base = in.lo & ~(uint64_t)15;
    pl.out_base = out.lo & ~(uint64_t)15;
    pl.aad_base = ad.lo & ~(uint64_t)15;
    pl.recs.assign(recs + i, recs + j);
    for (ptls_hip_record_t &r : pl.recs) {
        r.in_off -= pl.in_base;
        r.out_off -= pl.out_base;
        r.aad_off -= m.aad_in_out ? pl.out_base : m.aad_in_in ? pl.in_base : pl.aad_base;
    }
    /* the masks the kernel writes get packed places in d_mask; where they go in h_mask stays on the host */
    pl.supp.clear();
    pl.mask_dst.clear();
    if (supp != nullptr) {
        pl.supp.assign(supp + i, supp + j);
        for (ptls_hip_supp_t &sp : pl.supp) {
            if (!(sp.flags & PTLS_HIP_SUPP_ENABLE))
                continue;
            sp.sample_off -= pl.out_base;
            if (writes_mask(sp, hp_nslots)) {
                pl.mask_dst.push_back(sp.mask_off);
                sp.mask_off = 16 * (uint64_t)(pl.mask_dst.size() - 1);
            } else {
                sp.mask_off = 0; /* skipped by the kernel */
            }
        }
    }
    /* the output's copies back: the records' merged runs, joined over short gaps filled with the caller's bytes */
    std::vector<Span> &runs = pl.runs;
    runs.clear();
    for (size_t t = i; t < j; ++t)
        record_out_parts(recs[t], m, runs);
    merge_spans(runs);
    pl.pieces.clear();
    pl.gaps.clear();
    pl.gap_src.clear();
    uint32_t gap_bytes = 0;
    for (size_t t = 0; t < runs.size(); ++t) {
        const uint64_t glo = t != 0 ? pl.pieces.back().hi : 0, ghi = runs[t].lo;
        if (t == 0 || runs.size() <= COPY_DIRECT_RUNS || ghi - glo >= GAP_SPLIT || gap_bytes + (ghi - glo) > UINT32_MAX ||
            (!o.in_order && spans_hit(o.uni, glo, ghi))) {
            pl.pieces.push_back(runs[t]);
            continue;
        }
        pl.gaps.push_back(GapPiece{glo - pl.out_base, gap_bytes, (uint32_t)(ghi - glo)});
        pl.gap_src.push_back(Span{glo, ghi});
        gap_bytes += (uint32_t)(ghi - glo);
        pl.pieces.back().hi = runs[t].hi;
    }
    return 0;
}

/* ---------------------------------------------------------------------------------------------- */
/* QUIC packets (ptls_hip_pipeline_quic_seal / _open)                                               */
/* ---------------------------------------------------------------------------------------------- */

const char *quic_packet_fault(const ptls_hip_quic_packet_t &p, bool open)
{
    if (p.pn_offset == 0)
        return "pn_offset is 0";
    if (p.pkt_len < (uint32_t)p.pn_offset + 4u + 16u)
        return "the header-protection sample at pn_offset + 4 would leave the packet (pkt_len < pn_offset + 20)";
    if (!open && (p.pn_len < 1 || p.pn_len > 4))
        return "pn_len must be 1..4";
    if (!open && p.pn >= ((uint64_t)1 << 62))
        return "the packet number must be below 2^62";
    return nullptr;
}

void quic_records(const ptls_hip_quic_packet_t *pkts, size_t n, bool open, std::vector<ptls_hip_record_t> &recs,
                  std::vector<ptls_hip_supp_t> &supp)
{
    recs.resize(n);
    supp.resize(open ? 0 : n);
    for (size_t i = 0; i < n; ++i) {
        const ptls_hip_quic_packet_t &p = pkts[i];
        const uint32_t pn_len = open ? 1u : p.pn_len;
        ptls_hip_record_t &r = recs[i];
        r.aad_off = p.pkt_off;
        r.aad_len = (uint32_t)p.pn_offset + pn_len;
        r.len = p.pkt_len - r.aad_len - 16u;
        r.seq = p.pn;
        r.key = p.key;
        r.flags = 0;
        if (open) {
            r.in_off = p.pkt_off + r.aad_len;
            r.out_off = p.data_off;
        } else {
            r.in_off = p.data_off;
            r.out_off = p.pkt_off + r.aad_len;
            supp[i] = ptls_hip_supp_t{p.pkt_off + p.pn_offset + 4u, 16 * (uint64_t)i, p.hp_key, PTLS_HIP_SUPP_ENABLE};
        }
    }
}

int plan_quic_slice(const ptls_hip_quic_packet_t *pkts, const ptls_hip_record_t *recs, const ptls_hip_supp_t *supp, size_t n,
                    size_t i, const ModeInfo &m, size_t slice_bytes, size_t max_recs, const CopyOrder &o, QuicSlicePlan &pl)
{
    /* at most slot_max_masks packets: their masks (seal) or packed headers (open) share the slot's small staging.  Every
     * hp_key was checked against its keyset before the first slice, so the kernel writes every mask. */
    const size_t cap = std::min(max_recs, slot_max_masks(slice_bytes) + 1);
    SlicePlan &s = pl.s;
    if (int rc = plan_copy_slice(recs, supp, n, i, m, slice_bytes, cap, SIZE_MAX, o, s))
        return rc;
    s.mask_dst.clear(); /* the masks stay in the slot's d_mask for quic_protect_kernel */
    const size_t cnt = s.j - i;
    const uint64_t pkt_base = m.open ? s.in_base : s.out_base, data_base = m.open ? s.out_base : s.in_base;
    pl.pkts.assign(pkts + i, pkts + s.j);
    pl.hdr_dst.clear();
    uint64_t staged = s.gaps.empty() ? 0 : (uint64_t)s.gaps.back().src + s.gaps.back().len;
    for (size_t t = 0; t < cnt; ++t) {
        ptls_hip_quic_packet_t &p = pl.pkts[t];
        const ptls_hip_record_t &r = recs[i + t];
        /* seal: the header the caller wrote; open: the last 3 bytes of the area (r.len >= 3: pkt_len >= pn_offset + 20) */
        const uint64_t lo = m.open ? p.data_off + r.len - 3 : p.pkt_off;
        const uint32_t len = m.open ? 3u : r.aad_len;
        if (staged + len > slice_bytes)
            return fail(PTLS_HIP_EINVAL, "pipeline_quic_%s: the %s of the slice at packet %zu overlap", m.open ? "open" : "seal",
                        m.open ? "plaintext areas" : "packets", i);
        s.gaps.push_back(GapPiece{lo - s.out_base, (uint32_t)staged, len});
        s.gap_src.push_back(Span{lo, lo + len});
        staged += len;
        if (m.open)
            pl.hdr_dst.push_back(HdrDst{p.pkt_off, p.pn_offset});
        p.pkt_off -= pkt_base;
        p.data_off -= data_base;
    }
    return 0;
}
