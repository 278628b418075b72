/*
 * quic.cpp -- QUIC packet protection batches (include/ptls_hip.h 2e): the device packet array, the inner
 * record batch, the header-protection descriptors and mask buffer of a seal batch, the host-side refusals, and the two
 * calls: seal = seal_batch_supp + quic_protect_kernel, open = quic_unprotect_kernel + open_batch, all on the caller's stream.
 */
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "host.h"

struct st_ptls_hip_quic_batch_t {
    ptls_hip_engine_t *eng = nullptr;
    size_t n = 0;
    bool open = false;
    ptls_hip_quic_packet_t *d_pkts = nullptr;
    ptls_hip_batch_t *inner = nullptr;
    ptls_hip_supp_t *d_supp = nullptr; /* seal: sample of packet i -> mask at 16 i */
    uint8_t *d_mask = nullptr;         /* seal: 16 bytes per packet */
    uint32_t max_key = 0, max_hp_key = 0;
    size_t max_key_at = 0, max_hp_key_at = 0; /* the packets that name them (for the messages) */
    Uses uses; /* the launches that read d_pkts / d_mask: quic_batch_free waits for them */
};

template <class T>
static int upload(ptls_hip_engine_t *eng, T **d, const T *h, size_t n)
{
    HIP_TRY(dev_alloc(eng, reinterpret_cast<void **>(d), n * sizeof(T)), PTLS_HIP_ENOMEM);
    HIP_TRY(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice), PTLS_HIP_ENODEV);
    return 0;
}

extern "C" ptls_hip_quic_batch_t *ptls_hip_quic_batch_new(ptls_hip_engine_t *eng, const ptls_hip_quic_packet_t *pkts, size_t n,
                                                          int open, void *stream)
{
    if (eng == nullptr || (pkts == nullptr && n != 0) || n > 0xffffffffu) {
        fail(PTLS_HIP_EINVAL, "quic_batch_new: bad arguments");
        return nullptr;
    }
    /* every quantity of these checks is host-known; nothing touches the device before they pass */
    for (size_t i = 0; i < n; ++i) {
        const char *why = quic_packet_fault(pkts[i], open != 0);
        if (why != nullptr) {
            fail(PTLS_HIP_EINVAL, "quic_batch_new: packet %zu: %s", i, why);
            return nullptr;
        }
    }
    auto *q = new st_ptls_hip_quic_batch_t();
    q->eng = eng;
    q->n = n;
    q->open = open != 0;
    std::vector<ptls_hip_record_t> recs;
    std::vector<ptls_hip_supp_t> supp; /* seal: sample of packet i -> mask at 16 i */
    quic_records(pkts, n, q->open, recs, supp);
    for (size_t i = 0; i < n; ++i) {
        const ptls_hip_quic_packet_t &p = pkts[i];
        if (i == 0 || p.key > q->max_key)
            q->max_key = p.key, q->max_key_at = i;
        if (i == 0 || p.hp_key > q->max_hp_key)
            q->max_hp_key = p.hp_key, q->max_hp_key_at = i;
        /* open: the packet-number length sits under header protection.  The plan is made from pn_len = 1 (quic_records;
         * lengths are a performance hint to the planner: the kernels take every length from the descriptor they read at
         * launch), and as not 16-byte aligned: quic_unprotect_kernel writes the real in_off */
        if (q->open)
            recs[i].in_off |= 1u;
    }
    q->inner = ptls_hip_batch_new(eng, recs.data(), n, stream);
    if (q->inner == nullptr) { /* (the message is batch_new's) */
        delete q;
        return nullptr;
    }
    if (n != 0) {
        DeviceGuard g(eng->device);
        int e = upload(eng, &q->d_pkts, pkts, n);
        if (e == 0 && !q->open)
            e = upload(eng, &q->d_supp, supp.data(), n);
        if (e == 0 && !q->open && dev_alloc(eng, reinterpret_cast<void **>(&q->d_mask), 16 * n) != hipSuccess)
            e = fail(PTLS_HIP_ENOMEM, "quic_batch_new: cannot allocate %zu masks", n);
        if (e != 0) {
            const std::string why = g_err;
            ptls_hip_quic_batch_free(q);
            g_err = why;
            return nullptr;
        }
    }
    return q;
}

extern "C" void ptls_hip_quic_batch_free(ptls_hip_quic_batch_t *q)
{
    if (q == nullptr)
        return;
    {
        DeviceGuard g(q->eng->device);
        q->uses.wait();
        if (q->inner != nullptr)
            q->inner->uses.wait(); /* the seal launch reads d_supp and writes d_mask */
        dev_free(q->eng, q->d_pkts);
        dev_free(q->eng, q->d_supp);
        dev_free(q->eng, q->d_mask);
    }
    ptls_hip_batch_free(q->inner); /* waits for the record launches and for quic_unprotect_kernel, which writes its descriptors */
    delete q;
}

extern "C" ptls_hip_batch_t *ptls_hip_quic_batch_records(ptls_hip_quic_batch_t *q)
{
    if (q == nullptr) {
        fail(PTLS_HIP_EINVAL, "quic_batch_records: null batch");
        return nullptr;
    }
    return q->inner;
}

void quic_batch_lanes(ptls_hip_quic_batch_t *q, int *lanes, int *chacha_lanes)
{
    *lanes = q->inner->lanes;
    *chacha_lanes = q->inner->chacha_lanes;
}

/* what both calls refuse before anything is launched; `who` is the call's name */
static int check_call(const char *who, ptls_hip_quic_batch_t *q, bool open, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks)
{
    if (q == nullptr || ks == nullptr || hp_ks == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null batch or keyset", who);
    if (q->open != open)
        return fail(PTLS_HIP_EINVAL, "%s: the batch was made for %s", who, q->open ? "open" : "seal");
    if (ks->eng != q->eng || hp_ks->eng != q->eng)
        return fail(PTLS_HIP_EINVAL, "%s: batch and keysets must belong to the same engine", who);
    if (hp_ks->algo != ks->algo || hp_ks->key_size != ks->key_size)
        return fail(PTLS_HIP_EINVAL, "%s: the header-protection keyset must be of the AEAD keyset's algorithm and key size", who);
    if (q->n != 0 && q->max_key >= ks->nslots)
        return fail(PTLS_HIP_EINVAL, "%s: packet %zu names key slot %u, the keyset has %zu", who, q->max_key_at, q->max_key,
                    ks->nslots);
    if (q->n != 0 && q->max_hp_key >= hp_ks->nslots)
        return fail(PTLS_HIP_EINVAL, "%s: packet %zu names header-protection key slot %u, the keyset has %zu", who,
                    q->max_hp_key_at, q->max_hp_key, hp_ks->nslots);
    return 0;
}

int quic_unprotect(ptls_hip_engine_t *eng, const ptls_hip_keyset_t *hp_ks, const ptls_hip_quic_packet_t *d_pkts, size_t n,
                   ptls_hip_record_t *d_recs, ptls_hip_record_t *d_recs_ord, const uint32_t *d_order, void *pkt, uint64_t *pn_out,
                   void *stream, const QuicPhaseArgs *ph)
{
    const bool chacha = hp_ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    QuicArgs a{};
    a.pkts = d_pkts;
    a.n = (uint32_t)n;
    a.order = d_order;
    a.recs = d_recs;
    a.recs_ord = d_recs_ord;
    a.pkt = static_cast<uint8_t *>(pkt);
    a.pn_out = pn_out;
    a.hp_slots = hp_ks->d_slots;
    a.hp_chacha = hp_ks->d_chacha;
    a.t0 = eng->d_t0;
    /* one thread per packet; the AES kernel builds its T-tables per workgroup, so its threads take several packets each
     * (record_grid, the grid of aesecb_batch_kernel) */
    const unsigned grid = chacha ? (unsigned)((n + 255) / 256) : record_grid(n, eng->ncu);
    const int rounds = chacha ? 0 : hp_ks->key_size == 16 ? 10 : 14;
    return ph != nullptr ? launch_quic_unprotect_phase(rounds, a, *ph, grid, stream) : launch_quic_unprotect(rounds, a, grid, stream);
}

int quic_protect(const ptls_hip_quic_packet_t *d_pkts, size_t n, void *pkt, const uint8_t *d_mask, void *stream)
{
    return launch_quic_protect(d_pkts, (uint32_t)n, static_cast<uint8_t *>(pkt), d_mask, (unsigned)((n + 255) / 256), stream);
}

extern "C" int ptls_hip_quic_seal_batch(ptls_hip_quic_batch_t *q, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, const void *in,
                                        void *pkt, void *stream)
{
    if (int e = check_call("quic_seal_batch", q, false, ks, hp_ks))
        return e;
    if (q->n == 0)
        return 0;
    if (in == nullptr || pkt == nullptr)
        return fail(PTLS_HIP_EINVAL, "quic_seal_batch: null buffer");
    /* the record (AAD = the unprotected header in the packet) and the mask of its sample, then the header */
    if (int e = run_batch(q->inner, ks, in, pkt, pkt, nullptr, stream, false, hp_ks, q->d_supp, q->d_mask))
        return e;
    DeviceGuard g(q->eng->device);
    const int e = quic_protect(q->d_pkts, q->n, pkt, q->d_mask, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "quic_seal_batch: kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    q->uses.note(stream);
    return 0;
}

extern "C" int ptls_hip_quic_open_batch(ptls_hip_quic_batch_t *q, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, void *pkt,
                                        void *out, uint64_t *result, uint64_t *pn_out, void *stream)
{
    if (int e = check_call("quic_open_batch", q, true, ks, hp_ks))
        return e;
    if (q->n == 0)
        return 0;
    if (pkt == nullptr || out == nullptr || result == nullptr || pn_out == nullptr)
        return fail(PTLS_HIP_EINVAL, "quic_open_batch: null buffer");
    ptls_hip_batch_t *b = q->inner;
    {
        DeviceGuard g(q->eng->device);
        /* the inner batch's current plan (ptls_hip_batch_set_lanes re-plans it) */
        const int e = quic_unprotect(q->eng, hp_ks, q->d_pkts, q->n, b->d_recs, b->d_recs_ord, b->d_order, pkt, pn_out, stream);
        if (e != 0)
            return fail(PTLS_HIP_ELAUNCH, "quic_open_batch: kernel launch failed: %s", hipGetErrorString((hipError_t)e));
        keyset_note_use(hp_ks, stream);
        b->uses.note(stream); /* re-planning or freeing the inner batch waits for the descriptor writes */
        q->uses.note(stream);
    }
    return run_batch(b, ks, pkt, pkt, out, result, stream, true);
}
