/*
 * batch.cpp -- batches (uploaded record descriptors + their launch plan) and the device-resident calls: seal / open /
 * seal with QUIC header protection / standalone ECB masks / the synthetic-record generator.  One asynchronous launch each
 * on the caller's stream (picotls has no batch API).
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host.h"
/* When the plan keeps the caller's order (equal lengths per key run, or already non-increasing: configs[1], [2], [4]),
 * the kernels read the caller-order descriptors and no order array (record index = plan position): no second copy of
 * the descriptors in HBM and 4 bytes per record less to read per launch. */
static int plan_chunks(ptls_hip_batch_t *b)
{
    std::vector<Chunk> ch;
    std::vector<uint32_t> order;
    build_chunks(b->h_recs.data(), b->n, b->lanes, batch_cus(b), ch, order, b->all_aligned);
    b->wg = b->forced_wg ? b->forced_wg : plan_wg(ch, b->lanes);
    b->uses.wait(); /* an earlier launch may still read the old plan */
    dev_free(b->eng, b->d_chunks);
    dev_free(b->eng, b->d_order);
    dev_free(b->eng, b->d_recs_ord);
    b->d_chunks = nullptr;
    b->d_order = nullptr;
    b->d_recs_ord = nullptr;
    b->nchunks = (uint32_t)ch.size();
    if (ch.empty())
        return 0;
    HIP_TRY(dev_alloc(b->eng, reinterpret_cast<void **>(&b->d_chunks), ch.size() * sizeof(Chunk)), PTLS_HIP_ENOMEM);
    HIP_TRY(hipMemcpy(b->d_chunks, ch.data(), ch.size() * sizeof(Chunk), hipMemcpyHostToDevice), PTLS_HIP_ENODEV);
    if (identity_order(order, order.size()))
        return 0; /* d_order and d_recs_ord stay null: run_batch passes d_recs and no order */
    HIP_TRY(dev_alloc(b->eng, reinterpret_cast<void **>(&b->d_order), order.size() * sizeof(uint32_t)), PTLS_HIP_ENOMEM);
    HIP_TRY(hipMemcpy(b->d_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice), PTLS_HIP_ENODEV);
    std::vector<ptls_hip_record_t> ord(order.size());
    for (size_t k = 0; k < order.size(); ++k)
        ord[k] = b->h_recs[order[k]];
    HIP_TRY(dev_alloc(b->eng, reinterpret_cast<void **>(&b->d_recs_ord), ord.size() * sizeof(ptls_hip_record_t)), PTLS_HIP_ENOMEM);
    HIP_TRY(hipMemcpy(b->d_recs_ord, ord.data(), ord.size() * sizeof(ptls_hip_record_t), hipMemcpyHostToDevice), PTLS_HIP_ENODEV);
    return 0;
}

extern "C" ptls_hip_batch_t *ptls_hip_batch_new(ptls_hip_engine_t *eng, const ptls_hip_record_t *recs, size_t n, void *stream)
{
    (void)stream;
    if (eng == nullptr || (recs == nullptr && n != 0) || n > 0xffffffffu) {
        fail(PTLS_HIP_EINVAL, "batch_new: bad arguments");
        return nullptr;
    }
    DeviceGuard g(eng->device);
    auto *b = new st_ptls_hip_batch_t();
    b->eng = eng;
    b->n = n;
    b->h_recs.assign(recs, recs + n);
    b->max_key = 0;
    for (size_t i = 0; i < n; ++i)
        b->max_key = std::max(b->max_key, recs[i].key);
    b->auto_lanes = b->lanes = choose_lanes(b->h_recs.data(), b->h_recs.size(), (unsigned)eng->ncu);
    b->chacha_auto_lanes = b->chacha_lanes = choose_chacha_lanes(b->h_recs.data(), b->h_recs.size(), (unsigned)eng->ncu);
    if (n != 0) {
        if (dev_alloc(eng, reinterpret_cast<void **>(&b->d_recs), n * sizeof(ptls_hip_record_t)) != hipSuccess ||
            hipMemcpy(b->d_recs, recs, n * sizeof(ptls_hip_record_t), hipMemcpyHostToDevice) != hipSuccess) {
            fail(PTLS_HIP_ENOMEM, "batch_new: cannot upload %zu descriptors", n);
            dev_free(eng, b->d_recs);
            (void)hipStreamSynchronize(eng->util);
            delete b;
            return nullptr;
        }
    }
    if (plan_chunks(b) != 0) {
        ptls_hip_batch_free(b);
        return nullptr;
    }
    return b;
}

extern "C" void ptls_hip_batch_free(ptls_hip_batch_t *b)
{
    if (b == nullptr)
        return;
    DeviceGuard g(b->eng->device);
    b->uses.wait();
    dev_free(b->eng, b->d_recs);
    dev_free(b->eng, b->d_recs_ord);
    dev_free(b->eng, b->d_chunks);
    dev_free(b->eng, b->d_order);
    (void)hipStreamSynchronize(b->eng->util);
    delete b;
}

extern "C" size_t ptls_hip_batch_count(ptls_hip_batch_t *b)
{
    return b->n;
}

extern "C" int ptls_hip_batch_set_lanes(ptls_hip_batch_t *b, int lanes)
{
    if (b == nullptr ||
        !(lanes == 0 || lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == SPARSE_LANES))
        return fail(PTLS_HIP_EINVAL, "batch_set_lanes: lanes must be 0, 1, 2, 4, 8, 16, 32 or 64");
    DeviceGuard g(b->eng->device);
    const int want = lanes == 0 ? b->auto_lanes : lanes;
    if (want == b->lanes)
        return 0;
    b->lanes = want;
    return plan_chunks(b);
}

extern "C" int ptls_hip_batch_lanes(ptls_hip_batch_t *b)
{
    return b->lanes;
}

extern "C" int ptls_hip_batch_set_workgroup(ptls_hip_batch_t *b, int threads)
{
    if (b == nullptr || !(threads == 0 || threads == 512 || threads == WG_ALT))
        return fail(PTLS_HIP_EINVAL, "batch_set_workgroup: threads must be 0, 512 or %d", WG_ALT);
    DeviceGuard g(b->eng->device);
    b->forced_wg = threads;
    return plan_chunks(b);
}

extern "C" int ptls_hip_batch_workgroup(ptls_hip_batch_t *b)
{
    return b->wg;
}

extern "C" int ptls_hip_batch_set_max_workgroups(ptls_hip_batch_t *b, int n)
{
    if (b == nullptr || n < 0)
        return fail(PTLS_HIP_EINVAL, "batch_set_max_workgroups: n must be >= 0");
    DeviceGuard g(b->eng->device);
    b->max_wg = (unsigned)n;
    return plan_chunks(b);
}

extern "C" int ptls_hip_batch_grid(ptls_hip_batch_t *b)
{
    if (b == nullptr)
        return fail(PTLS_HIP_EINVAL, "batch_grid: null batch");
    return (int)plan_grid(b->n, b->nchunks, b->lanes, batch_cus(b));
}

extern "C" int ptls_hip_batch_chunks(ptls_hip_batch_t *b)
{
    return b != nullptr ? (int)b->nchunks : fail(PTLS_HIP_EINVAL, "batch_chunks: null batch");
}

extern "C" int ptls_hip_batch_set_clock(ptls_hip_batch_t *b, void *d_buf, size_t nbytes)
{
    if (b == nullptr || (d_buf != nullptr && nbytes < (size_t)ptls_hip_batch_grid(b) * 32))
        return fail(PTLS_HIP_EINVAL, "batch_set_clock: the buffer needs 32 bytes per workgroup of the launch");
    b->d_clk = static_cast<uint64_t *>(d_buf);
    b->clk_bytes = d_buf != nullptr ? nbytes : 0;
    return 0;
}

int run_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result,
              void *stream, bool open, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, void *mask, int algo)
{
    if (b == nullptr || ks == nullptr || ks->eng != b->eng)
        return fail(PTLS_HIP_EINVAL, "seal/open: batch and keyset must belong to the same engine");
    /* the keyset's kind is host state: a call of the other cipher fails here, before any slot memory is named */
    if (algo != 0 && ks->algo != algo)
        return fail(PTLS_HIP_EINVAL, "seal/open: the keyset holds %s keys",
                    ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305 ? "ChaCha20-Poly1305" : "AES-GCM");
    if (supp != nullptr && hp_ks != nullptr && hp_ks->algo != ks->algo)
        return fail(PTLS_HIP_EINVAL, "seal_batch_supp: the header-protection keyset is of the other algorithm");
    /* (the key sizes of two ChaCha keysets always agree: 32 bytes) */
    if (supp != nullptr && (hp_ks == nullptr || hp_ks->eng != b->eng || hp_ks->key_size != ks->key_size || mask == nullptr))
        return fail(PTLS_HIP_EINVAL, "seal_batch_supp: the header-protection keyset must be on the same engine with the "
                                     "AEAD's key size, and mask must be given");
    if (b->n == 0)
        return 0;
    if (b->max_key >= ks->nslots)
        return fail(PTLS_HIP_EINVAL, "seal/open: a record names key slot %u, the keyset has %zu", b->max_key, ks->nslots);
    if (in == nullptr || out == nullptr || (open && result == nullptr))
        return fail(PTLS_HIP_EINVAL, "seal/open: null buffer");
    LaunchPlan p{};
    p.eng = b->eng;
    p.n = b->n;
    p.d_recs = b->d_recs;
    p.d_recs_ord = b->d_recs_ord;
    p.d_order = b->d_order;
    p.d_chunks = b->d_chunks;
    p.nchunks = b->nchunks;
    p.lanes = b->lanes;
    p.wg = b->wg;
    p.chacha_lanes = b->chacha_lanes;
    p.all_aligned = b->all_aligned;
    p.ncus = batch_cus(b);
    p.d_clk = b->d_clk;
    p.clk_bytes = b->clk_bytes;
    if (int e = run_plan(p, ks, in, aad, out, result, stream, open, hp_ks, supp, mask))
        return e;
    b->uses.note(stream);
    return 0;
}

int run_plan(const LaunchPlan &p, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result, void *stream,
             bool open, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, void *mask)
{
    if (int e = launch_plan(p, ks, in, aad, out, result, stream, open, hp_ks, supp, mask))
        return e;
    keyset_note_use(ks, stream);
    keyset_note_use(hp_ks, stream);
    return 0;
}

int launch_plan(const LaunchPlan &p, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out, uint64_t *result,
                void *stream, bool open, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, void *mask)
{
    DeviceGuard g(p.eng->device);
    const uint8_t *in8 = static_cast<const uint8_t *>(in), *aad8 = static_cast<const uint8_t *>(aad != nullptr ? aad : in);
    const bool aligned = p.all_aligned && ((reinterpret_cast<uintptr_t>(in8) | reinterpret_cast<uintptr_t>(aad8) |
                                            reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    int e;
    if (ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305) {
        ChaChaArgs a{};
        a.recs = p.d_recs; /* descriptor order: no key runs, no chunks */
        a.n = p.n;
        a.in = in8;
        a.aad = aad8;
        a.out = static_cast<uint8_t *>(out);
        a.result = result;
        a.slots = ks->d_chacha;
        a.supp = supp;
        a.hp_slots = hp_ks != nullptr ? hp_ks->d_chacha : nullptr;
        a.hp_nslots = hp_ks != nullptr ? (uint32_t)hp_ks->nslots : 0;
        a.mask = static_cast<uint8_t *>(mask);
        e = p.chacha_runs ? launch_chacha_runs(p.chacha_lanes, open, stream, a, aligned)
                          : launch_chacha_batch(p.chacha_lanes, open, stream, a, aligned);
    } else {
        KernelArgs a{};
        a.recs = p.d_recs;
        a.recs_ord = p.d_recs_ord != nullptr ? p.d_recs_ord : p.d_recs;
        a.order = p.d_order;
        a.chunks = p.d_chunks;
        a.nchunks = p.nchunks;
        a.in = in8;
        a.aad = aad8;
        a.out = static_cast<uint8_t *>(out);
        a.result = result;
        set_key_args(a, p.eng, ks, hp_ks);
        a.supp = supp;
        a.mask = static_cast<uint8_t *>(mask);
        const unsigned grid = plan_grid(p.n, p.nchunks, p.lanes, p.ncus);
        if (p.d_clk != nullptr && p.clk_bytes < (size_t)grid * 32)
            return fail(PTLS_HIP_EINVAL, "seal/open: the clock-stamp buffer is smaller than 32 bytes x %u workgroups", grid);
        a.clk = p.d_clk;
        a.clk_bytes = p.clk_bytes;
        a.queue = queue_slot(p.eng);
        e = launch_batch(p.lanes, ks->key_size == 16 ? 10 : 14, open, p.wg, grid, stream, a, aligned);
    }
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "kernel launch failed: %s", hipGetErrorString((hipError_t)e));
    return 0;
}

extern "C" int ptls_hip_aesgcm_seal_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out,
                                          void *stream)
{
    return run_batch(b, ks, in, aad, out, nullptr, stream, false, nullptr, nullptr, nullptr, PTLS_HIP_ALGO_AESGCM);
}

/* ---- ChaCha20-Poly1305 (chacha_kernel.hip): the same batches, the keyset's other kind ---- */

extern "C" int ptls_hip_batch_set_chacha_lanes(ptls_hip_batch_t *b, int lanes)
{
    if (b == nullptr || !(lanes == 0 || lanes == 1 || lanes == 4 || lanes == 16 || lanes == 64))
        return fail(PTLS_HIP_EINVAL, "batch_set_chacha_lanes: lanes must be 0, 1, 4, 16 or 64");
    b->chacha_lanes = lanes == 0 ? b->chacha_auto_lanes : lanes; /* nothing is planned per width: the next launch uses it */
    return 0;
}

extern "C" int ptls_hip_batch_chacha_lanes(ptls_hip_batch_t *b)
{
    return b != nullptr ? b->chacha_lanes : fail(PTLS_HIP_EINVAL, "batch_chacha_lanes: null batch");
}

extern "C" int ptls_hip_chacha20poly1305_seal_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad,
                                                    void *out, void *stream)
{
    return run_batch(b, ks, in, aad, out, nullptr, stream, false, nullptr, nullptr, nullptr, PTLS_HIP_ALGO_CHACHA20POLY1305);
}

extern "C" int ptls_hip_chacha20poly1305_open_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad,
                                                    void *out, uint64_t *result, void *stream)
{
    return run_batch(b, ks, in, aad, out, result, stream, true, nullptr, nullptr, nullptr, PTLS_HIP_ALGO_CHACHA20POLY1305);
}

extern "C" int ptls_hip_chacha20poly1305_seal_batch_supp(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                                         const ptls_hip_supp_t *supp, const void *in, const void *aad, void *out,
                                                         void *mask, void *stream)
{
    if (supp == nullptr)
        return fail(PTLS_HIP_EINVAL, "seal_batch_supp: supp descriptors missing");
    return run_batch(b, ks, in, aad, out, nullptr, stream, false, hp_ks, supp, mask, PTLS_HIP_ALGO_CHACHA20POLY1305);
}

/* the stand-alone header-protection masks of n samples (the receive side): one AES-ECB block, or the first 16 ChaCha20
 * keystream bytes, per sample, with a keyset of `algo`; `who` is the exported call's name in the messages */
static int mask_batch(const char *who, int algo, ptls_hip_engine_t *eng, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp,
                      size_t n, const void *src, void *mask, void *stream)
{
    const bool chacha = algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    if (eng == nullptr || hp_ks == nullptr || hp_ks->eng != eng || hp_ks->algo != algo || n > 0xffffffffu ||
        (n != 0 && (supp == nullptr || src == nullptr || mask == nullptr)))
        return fail(PTLS_HIP_EINVAL, "%s: bad arguments (%s keyset of this engine is needed)", who, chacha ? "a ChaCha" : "an AES");
    if (n == 0)
        return 0;
    DeviceGuard g(eng->device);
    const unsigned grid = record_grid(n, eng->ncu);
    const uint8_t *src8 = static_cast<const uint8_t *>(src);
    uint8_t *mask8 = static_cast<uint8_t *>(mask);
    const int e = chacha ? launch_chacha_mask(supp, (uint32_t)n, src8, mask8, hp_ks->d_chacha, (uint32_t)hp_ks->nslots, grid, stream)
                         : launch_aesecb(hp_ks->key_size == 16 ? 10 : 14, supp, (uint32_t)n, src8, mask8, hp_ks->d_slots,
                                         (uint32_t)hp_ks->nslots, eng->d_t0, grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "%s: kernel launch failed: %s", who, hipGetErrorString((hipError_t)e));
    keyset_note_use(hp_ks, stream);
    return 0;
}

extern "C" int ptls_hip_chacha20_mask_batch(ptls_hip_engine_t *eng, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, size_t n,
                                            const void *src, void *mask, void *stream)
{
    return mask_batch("chacha20_mask_batch", PTLS_HIP_ALGO_CHACHA20POLY1305, eng, hp_ks, supp, n, src, mask, stream);
}

extern "C" int ptls_hip_aesgcm_seal_batch_supp(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks,
                                               const ptls_hip_supp_t *supp, const void *in, const void *aad, void *out, void *mask,
                                               void *stream)
{
    if (supp == nullptr)
        return fail(PTLS_HIP_EINVAL, "seal_batch_supp: supp descriptors missing");
    return run_batch(b, ks, in, aad, out, nullptr, stream, false, hp_ks, supp, mask, PTLS_HIP_ALGO_AESGCM);
}

extern "C" int ptls_hip_aesecb_batch(ptls_hip_engine_t *eng, ptls_hip_keyset_t *hp_ks, const ptls_hip_supp_t *supp, size_t n,
                                     const void *src, void *mask, void *stream)
{
    return mask_batch("aesecb_batch", PTLS_HIP_ALGO_AESGCM, eng, hp_ks, supp, n, src, mask, stream);
}

extern "C" int ptls_hip_aesgcm_open_batch(ptls_hip_batch_t *b, ptls_hip_keyset_t *ks, const void *in, const void *aad, void *out,
                                          uint64_t *result, void *stream)
{
    return run_batch(b, ks, in, aad, out, result, stream, true, nullptr, nullptr, nullptr, PTLS_HIP_ALGO_AESGCM);
}

extern "C" int ptls_hip_fill_records(ptls_hip_batch_t *b, void *buf, uint64_t seed, uint64_t index_base, const uint64_t *index,
                                     void *stream)
{
    if (b == nullptr || buf == nullptr)
        return fail(PTLS_HIP_EINVAL, "fill_records: bad arguments");
    if (b->n == 0)
        return 0;
    DeviceGuard g(b->eng->device);
    const unsigned grid = (unsigned)std::min<size_t>((b->n + 3) / 4, (size_t)b->eng->ncu * 16);
    int e = launch_fill(b->d_recs, (uint32_t)b->n, static_cast<uint8_t *>(buf), seed, index_base, index, grid, stream);
    if (e != 0)
        return fail(PTLS_HIP_ELAUNCH, "fill launch failed: %s", hipGetErrorString((hipError_t)e));
    b->uses.note(stream);
    return 0;
}
