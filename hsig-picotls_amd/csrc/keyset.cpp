/*
 * keyset.cpp -- keysets: arrays of device-resident AEAD contexts (AES-GCM: KeySlot + GHASH basis; ChaCha20-Poly1305:
 * ChaChaSlot, internal.h), keyed from raw keys
 * (setup_crypto, lib/fusion.c:1184-1206) or from TLS 1.3 traffic secrets (get_traffic_keys, lib/picotls.c:1603-1622),
 * with the static-IV get / set / xor of ptls_aead_xor_iv (lib/picotls.c:6481-6490).
 */
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "host.h"
/* the Initial salt's HMAC pads are hashed on the host with the functions the kernels run (host-only qualifier) */
#define GF128_FN static inline
#include "quic_keys.h"

/* ---------------------------------------------------------------------------------------------- */
/* keysets                                                                                         */
/* ---------------------------------------------------------------------------------------------- */

/* The allocator behind both constructors (`who` names the caller in the messages).  AES-GCM: a KeySlot and a GHASH basis per
 * slot, 16- or 32-byte keys.  ChaCha20-Poly1305: 44 bytes per slot (key + static IV) in its own device array, 32-byte keys.
 * The key size and the slot count are checked before the engine is touched. */
static ptls_hip_keyset_t *keyset_alloc(const char *who, ptls_hip_engine_t *eng, int algo, size_t key_size, size_t nslots)
{
    const bool chacha = algo == PTLS_HIP_ALGO_CHACHA20POLY1305;
    const bool key_ok = chacha ? key_size == 32 : algo == PTLS_HIP_ALGO_AESGCM && (key_size == 16 || key_size == 32);
    if (eng == nullptr || !key_ok || nslots == 0 || nslots > 0xffffffffu) {
        fail(PTLS_HIP_EINVAL, "%s: bad arguments (algo %d, key_size %zu, nslots %zu)", who, algo, key_size, nslots);
        return nullptr;
    }
    DeviceGuard g(eng->device);
    auto *ks = new st_ptls_hip_keyset_t(); /* every slot array starts null */
    ks->eng = eng;
    ks->algo = algo;
    ks->key_size = key_size;
    ks->nslots = nslots;
    ks->ivs.assign(nslots * 12, 0);
    const bool ok = chacha ? dev_alloc(eng, reinterpret_cast<void **>(&ks->d_chacha), nslots * sizeof(ChaChaSlot)) == hipSuccess
                           : dev_alloc(eng, reinterpret_cast<void **>(&ks->d_slots), nslots * sizeof(KeySlot)) == hipSuccess &&
                                 dev_alloc(eng, reinterpret_cast<void **>(&ks->d_basis), nslots * BASIS_WORDS_PER_SLOT * 4) == hipSuccess;
    if (!ok) {
        fail(PTLS_HIP_ENOMEM, "%s: cannot allocate %zu key slots", who, nslots);
        dev_free(eng, ks->d_slots);
        dev_free(eng, ks->d_basis);
        delete ks;
        return nullptr;
    }
    if (chacha)
        (void)hipMemsetAsync(ks->d_chacha, 0, nslots * sizeof(ChaChaSlot), eng->util);
    else
        (void)hipMemsetAsync(ks->d_slots, 0, nslots * sizeof(KeySlot), eng->util);
    (void)hipStreamSynchronize(eng->util);
    return ks;
}

extern "C" ptls_hip_keyset_t *ptls_hip_keyset_new(ptls_hip_engine_t *eng, size_t key_size, size_t nslots)
{
    return keyset_alloc("keyset_new", eng, PTLS_HIP_ALGO_AESGCM, key_size, nslots);
}

extern "C" ptls_hip_keyset_t *ptls_hip_keyset_new_algo(ptls_hip_engine_t *eng, int algo, size_t key_size, size_t nslots)
{
    return keyset_alloc("keyset_new_algo", eng, algo, key_size, nslots);
}

extern "C" int ptls_hip_keyset_algo(ptls_hip_keyset_t *ks)
{
    return ks != nullptr ? ks->algo : fail(PTLS_HIP_EINVAL, "keyset_algo: null keyset");
}

extern "C" void ptls_hip_keyset_free(ptls_hip_keyset_t *ks)
{
    if (ks == nullptr)
        return;
    DeviceGuard g(ks->eng->device);
    if (ks->pool_id >= 0) { /* a plugin context's pooled slot (AES only): zeroed and retired, nothing waits */
        pool_release(ks);
        std::fill(ks->ivs.begin(), ks->ivs.end(), 0);
        delete ks;
        return;
    }
    /* the launches that read this keyset (keyset_note_use), not the whole device: a resident plugin worker or another
     * thread's batches are not waited for */
    ks->uses.wait();
    /* zeroize key material before release (ptls_clear_memory in aesgcm_dispose_crypto, lib/fusion.c:1102-1107, :1042-1048),
     * then release in the same stream order */
    ptls_hip_engine_t *e = ks->eng;
    if (ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305) {
        (void)hipMemsetAsync(ks->d_chacha, 0, ks->nslots * sizeof(ChaChaSlot), e->util);
    } else {
        (void)hipMemsetAsync(ks->d_slots, 0, ks->nslots * sizeof(KeySlot), e->util);
        (void)hipMemsetAsync(ks->d_basis, 0, ks->nslots * BASIS_WORDS_PER_SLOT * 4, e->util);
    }
    dev_free(e, ks->d_chacha); /* the arrays of the other algorithm are null */
    dev_free(e, ks->d_slots);
    dev_free(e, ks->d_basis);
    (void)hipStreamSynchronize(e->util);
    std::fill(ks->ivs.begin(), ks->ivs.end(), 0);
    delete ks;
}

extern "C" size_t ptls_hip_keyset_size(ptls_hip_keyset_t *ks)
{
    return ks->nslots;
}

/* raw keys and IVs in device memory -> the keyset's slots: the AES key expansion and GHASH basis, or ChaCha's plain copy */
static int keyset_setup(ptls_hip_keyset_t *ks, const uint8_t *d_keys, const uint8_t *d_ivs, uint32_t first, uint32_t count,
                        void *stream)
{
    if (ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305)
        return launch_chacha_keysetup(ks->d_chacha, d_keys, d_ivs, first, count, stream);
    return launch_keysetup(ks->d_slots, ks->d_basis, d_keys, d_ivs, first, count, (int)ks->key_size, ks->eng->d_t0, stream);
}

extern "C" int ptls_hip_keyset_set(ptls_hip_keyset_t *ks, size_t first, size_t count, const void *keys, const void *ivs,
                                   void *stream)
{
    if (ks == nullptr || keys == nullptr || first + count > ks->nslots)
        return fail(PTLS_HIP_EINVAL, "keyset_set: bad arguments");
    if (count == 0)
        return 0;
    std::vector<uint8_t> zero_ivs;
    if (ivs == nullptr) { /* header-protection / ECB-only keys carry no IV */
        zero_ivs.assign(count * 12, 0);
        ivs = zero_ivs.data();
    }
    DeviceGuard g(ks->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *d_tmp = nullptr;
    const size_t kbytes = count * ks->key_size, ibytes = count * 12;
    /* stream-ordered (dev_alloc): a hipMalloc / hipFree pair would wait for all device work, a resident plugin worker
     * included */
    HIP_TRY(dev_alloc(ks->eng, reinterpret_cast<void **>(&d_tmp), kbytes + ibytes), PTLS_HIP_ENOMEM);
    int rc = 0;
    if (hipMemcpyAsync(d_tmp, keys, kbytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_tmp + kbytes, ivs, ibytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = fail(PTLS_HIP_ENODEV, "keyset_set: upload failed");
    } else {
        int e = keyset_setup(ks, d_tmp, d_tmp + kbytes, (uint32_t)first, (uint32_t)count, stream);
        if (e != 0)
            rc = fail(PTLS_HIP_ELAUNCH, "keyset_set: key setup launch failed: %s", hipGetErrorString((hipError_t)e));
        else if (hipStreamSynchronize(s) != hipSuccess)
            rc = fail(PTLS_HIP_ENODEV, "keyset_set: key setup failed");
    }
    /* raw keys do not stay in device memory outside the expanded slots: the scrub is ordered after the
     * uploads and the key setup on the same stream, whatever path got here */
    (void)hipMemsetAsync(d_tmp, 0, kbytes + ibytes, s);
    (void)hipStreamSynchronize(s);
    dev_free(ks->eng, d_tmp); /* after the scrub: the stream was synchronized */
    if (rc == 0)
        std::memcpy(&ks->ivs[first * 12], ivs, ibytes);
    return rc;
}

/* TLS 1.3 traffic secrets -> key slots, optionally after the key-update step (keyschedule.hip) */
static int keyset_from_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, void *secrets, size_t hash_size, void *stream,
                               bool update)
{
    if (ks == nullptr || secrets == nullptr || first + count > ks->nslots || !(hash_size == 32 || hash_size == 48) ||
        count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "keyset_%s_secrets: bad arguments", update ? "update" : "set");
    if (count == 0)
        return 0;
    DeviceGuard g(ks->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t sbytes = count * hash_size, kbytes = count * ks->key_size, ibytes = count * 12;
    uint8_t *d = nullptr;
    HIP_TRY(dev_alloc(ks->eng, reinterpret_cast<void **>(&d), 2 * sbytes + kbytes + ibytes), PTLS_HIP_ENOMEM);
    uint8_t *d_sec = d, *d_next = d + sbytes, *d_keys = d + 2 * sbytes, *d_ivs = d + 2 * sbytes + kbytes;
    std::vector<uint8_t> h_ivs(ibytes);
    int rc = 0;
    if (hipMemcpyAsync(d_sec, secrets, sbytes, hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = fail(PTLS_HIP_ENODEV, "keyset secrets: upload failed");
    } else if (int e = launch_derive_traffic_keys(d_sec, update ? d_next : nullptr, (uint32_t)count, (int)hash_size,
                                                  (int)ks->key_size, update ? 1 : 0, d_keys, d_ivs, stream)) {
        rc = fail(PTLS_HIP_ELAUNCH, "keyset secrets: derive launch failed: %s", hipGetErrorString((hipError_t)e));
    } else if (int e2 = keyset_setup(ks, d_keys, d_ivs, (uint32_t)first, (uint32_t)count, stream)) {
        rc = fail(PTLS_HIP_ELAUNCH, "keyset secrets: key setup launch failed: %s", hipGetErrorString((hipError_t)e2));
    } else if (hipMemcpyAsync(h_ivs.data(), d_ivs, ibytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
               (update && hipMemcpyAsync(secrets, d_next, sbytes, hipMemcpyDeviceToHost, s) != hipSuccess) ||
               hipStreamSynchronize(s) != hipSuccess) {
        rc = fail(PTLS_HIP_ENODEV, "keyset secrets: derivation failed");
    }
    /* secrets and raw keys do not stay in device memory outside the expanded slots */
    (void)hipMemsetAsync(d, 0, 2 * sbytes + kbytes + ibytes, s);
    (void)hipStreamSynchronize(s);
    dev_free(ks->eng, d); /* after the scrub: the stream was synchronized */
    if (rc == 0)
        std::memcpy(&ks->ivs[first * 12], h_ivs.data(), ibytes);
    std::fill(h_ivs.begin(), h_ivs.end(), 0);
    return rc;
}

extern "C" int ptls_hip_keyset_set_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, const void *secrets, size_t hash_size,
                                           void *stream)
{
    return keyset_from_secrets(ks, first, count, const_cast<void *>(secrets), hash_size, stream, false);
}

extern "C" int ptls_hip_keyset_update_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, void *secrets, size_t hash_size,
                                              void *stream)
{
    return keyset_from_secrets(ks, first, count, secrets, hash_size, stream, true);
}

/* ---- QUIC: keys from traffic secrets or Destination Connection IDs (quic_keys.hip; include/ptls_hip.h 2f) ---- */

/* what the three QUIC calls refuse about their keysets: `n` slots from `first` in ks and (unless null) hp_ks, which must be
 * ks's twin (engine, algorithm, key size) */
static int quic_keysets_check(const char *who, const ptls_hip_keyset_t *ks, const ptls_hip_keyset_t *hp_ks, size_t first, size_t n)
{
    if (hp_ks != nullptr && (hp_ks->eng != ks->eng || hp_ks->algo != ks->algo || hp_ks->key_size != ks->key_size))
        return fail(PTLS_HIP_EINVAL, "%s: the keysets differ in engine, algorithm or key size", who);
    if (first > ks->nslots || n > ks->nslots - first || (hp_ks != nullptr && (first > hp_ks->nslots || n > hp_ks->nslots - first)))
        return fail(PTLS_HIP_EINVAL, "%s: slots %zu..%zu lie past a keyset", who, first, first + n);
    return 0;
}

/* The device scratch of one QUIC call: the call's input (secrets, or connection IDs), then for n slots the packed raw keys,
 * header-protection keys, IVs, and the zero IVs of the header-protection slots.  Key arrays first: they stay 16-byte aligned. */
struct QuicScratch {
    uint8_t *d = nullptr, *keys, *hps, *ivs, *zero_ivs;
    size_t bytes, kbytes, ibytes;

    hipError_t alloc(ptls_hip_keyset_t *ks, size_t in_bytes, size_t n)
    {
        in_bytes = (in_bytes + 15) & ~(size_t)15;
        kbytes = n * ks->key_size, ibytes = n * 12;
        bytes = in_bytes + 2 * kbytes + 2 * ibytes;
        hipError_t e = dev_alloc(ks->eng, reinterpret_cast<void **>(&d), bytes);
        keys = d + in_bytes, hps = keys + kbytes, ivs = hps + kbytes, zero_ivs = ivs + ibytes;
        return e;
    }
};

/* after the derivation launch: both key expansions, the IVs back to the host, the wait; then, whatever happened, the scrub
 * of the scratch and its release.  Returns rc, or the first failure here. */
static int quic_keys_finish(const char *who, int rc, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, QuicScratch &sc, size_t first,
                            size_t n, void *back, const uint8_t *d_back, size_t back_bytes, void *stream)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint8_t> h_ivs(sc.ibytes);
    if (rc == 0) {
        int e = 0;
        if (hp_ks != nullptr && hipMemsetAsync(sc.zero_ivs, 0, sc.ibytes, s) != hipSuccess)
            rc = fail(PTLS_HIP_ENODEV, "%s: memset failed", who);
        else if ((e = keyset_setup(ks, sc.keys, sc.ivs, (uint32_t)first, (uint32_t)n, stream)) != 0 ||
                 (hp_ks != nullptr && (e = keyset_setup(hp_ks, sc.hps, sc.zero_ivs, (uint32_t)first, (uint32_t)n, stream)) != 0))
            rc = fail(PTLS_HIP_ELAUNCH, "%s: key setup launch failed: %s", who, hipGetErrorString((hipError_t)e));
        else if (hipMemcpyAsync(h_ivs.data(), sc.ivs, sc.ibytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
                 (back != nullptr && hipMemcpyAsync(back, d_back, back_bytes, hipMemcpyDeviceToHost, s) != hipSuccess) ||
                 hipStreamSynchronize(s) != hipSuccess)
            rc = fail(PTLS_HIP_ENODEV, "%s: derivation failed", who);
    }
    /* secrets and raw keys do not stay in device memory outside the expanded slots */
    (void)hipMemsetAsync(sc.d, 0, sc.bytes, s);
    (void)hipStreamSynchronize(s);
    dev_free(ks->eng, sc.d); /* after the scrub: the stream was synchronized */
    if (rc == 0) {
        std::memcpy(&ks->ivs[first * 12], h_ivs.data(), sc.ibytes);
        if (hp_ks != nullptr)
            std::memset(&hp_ks->ivs[first * 12], 0, sc.ibytes);
    }
    std::fill(h_ivs.begin(), h_ivs.end(), 0);
    return rc;
}

static int keyset_from_quic_secrets(const char *who, ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t first, size_t count,
                                    void *secrets, size_t hash_size, int labels, void *stream, bool update)
{
    if (ks == nullptr || (!update && hp_ks == nullptr) || secrets == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null keyset or secrets", who);
    if (labels != PTLS_HIP_QUIC_LABELS_V1 && labels != PTLS_HIP_QUIC_LABELS_V2)
        return fail(PTLS_HIP_EINVAL, "%s: labels must be PTLS_HIP_QUIC_LABELS_V1 or _V2 (got %d)", who, labels);
    if (count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: count %zu is above 2^32 - 1", who, count);
    /* SHA-384 goes with AES-256-GCM only (TLS_AES_256_GCM_SHA384); AES-128-GCM and ChaCha20-Poly1305 are SHA-256 suites */
    const bool hash_ok = hash_size == 32 || (hash_size == 48 && ks->algo == PTLS_HIP_ALGO_AESGCM && ks->key_size == 32);
    if (!hash_ok)
        return fail(PTLS_HIP_EINVAL, "%s: hash_size %zu does not go with the keyset (algo %d, key_size %zu)", who, hash_size,
                    ks->algo, ks->key_size);
    if (int rc = quic_keysets_check(who, ks, hp_ks, first, count))
        return rc;
    if (count == 0)
        return 0;
    DeviceGuard g(ks->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t sbytes = count * hash_size;
    QuicScratch sc;
    HIP_TRY(sc.alloc(ks, 2 * sbytes, count), PTLS_HIP_ENOMEM);
    uint8_t *d_sec = sc.d, *d_next = sc.d + sbytes;
    int rc = 0;
    if (hipMemcpyAsync(d_sec, secrets, sbytes, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = fail(PTLS_HIP_ENODEV, "%s: upload failed", who);
    else if (int e = launch_quic_derive_keys(d_sec, update ? d_next : nullptr, (uint32_t)count, (int)hash_size, (int)ks->key_size,
                                             update ? 1 : 0, labels, sc.keys, sc.ivs, hp_ks != nullptr ? sc.hps : nullptr, stream))
        rc = fail(PTLS_HIP_ELAUNCH, "%s: derive launch failed: %s", who, hipGetErrorString((hipError_t)e));
    return quic_keys_finish(who, rc, ks, hp_ks, sc, first, count, update ? secrets : nullptr, d_next, sbytes, stream);
}

extern "C" int ptls_hip_keyset_set_quic_secrets(ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t first, size_t count,
                                                const void *secrets, size_t hash_size, int labels, void *stream)
{
    return keyset_from_quic_secrets("keyset_set_quic_secrets", ks, hp_ks, first, count, const_cast<void *>(secrets), hash_size, labels,
                                    stream, false);
}

extern "C" int ptls_hip_keyset_update_quic_secrets(ptls_hip_keyset_t *ks, size_t first, size_t count, void *secrets,
                                                   size_t hash_size, int labels, void *stream)
{
    return keyset_from_quic_secrets("keyset_update_quic_secrets", ks, nullptr, first, count, secrets, hash_size, labels, stream, true);
}

extern "C" int ptls_hip_keyset_set_quic_initial(ptls_hip_keyset_t *ks, ptls_hip_keyset_t *hp_ks, size_t first, size_t count,
                                                const void *dcids, const uint8_t *dcid_lens, const void *salt, size_t salt_len,
                                                int labels, void *stream)
{
    const char *who = "keyset_set_quic_initial";
    if (ks == nullptr || hp_ks == nullptr || dcids == nullptr || dcid_lens == nullptr || salt == nullptr)
        return fail(PTLS_HIP_EINVAL, "%s: null keyset, connection IDs or salt", who);
    if (labels != PTLS_HIP_QUIC_LABELS_V1 && labels != PTLS_HIP_QUIC_LABELS_V2)
        return fail(PTLS_HIP_EINVAL, "%s: labels must be PTLS_HIP_QUIC_LABELS_V1 or _V2 (got %d)", who, labels);
    if (count > 0xffffffffu)
        return fail(PTLS_HIP_EINVAL, "%s: count %zu is above 2^32 - 1", who, count);
    if (salt_len < 1 || salt_len > HK_SALT_MAX)
        return fail(PTLS_HIP_EINVAL, "%s: salt_len %zu is outside 1..64", who, salt_len);
    if (ks->algo != PTLS_HIP_ALGO_AESGCM || ks->key_size != 16)
        return fail(PTLS_HIP_EINVAL, "%s: Initial packets use AES-128-GCM: the keyset has algo %d, key_size %zu", who, ks->algo,
                    ks->key_size);
    if (int rc = quic_keysets_check(who, ks, hp_ks, first, 2 * count))
        return rc;
    for (size_t i = 0; i < count; ++i)
        if (dcid_lens[i] > HK_DCID_STRIDE)
            return fail(PTLS_HIP_EINVAL, "%s: dcid_lens[%zu] is %u, above 20", who, i, (unsigned)dcid_lens[i]);
    if (count == 0)
        return 0;
    DeviceGuard g(ks->eng->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    /* the salt is the same HMAC key for every connection: its pads are hashed here, once per call */
    HkPads<HkSha256> pads;
    hk_salt_pads(pads, static_cast<const uint8_t *>(salt), salt_len);
    QuicSaltPads sp;
    std::memcpy(sp.in, pads.in, sizeof(sp.in));
    std::memcpy(sp.out, pads.out, sizeof(sp.out));
    const size_t dbytes = count * HK_DCID_STRIDE;
    QuicScratch sc;
    HIP_TRY(sc.alloc(ks, dbytes + count, 2 * count), PTLS_HIP_ENOMEM);
    uint8_t *d_dcids = sc.d, *d_lens = sc.d + dbytes;
    int rc = 0;
    if (hipMemcpyAsync(d_dcids, dcids, dbytes, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_lens, dcid_lens, count, hipMemcpyHostToDevice, s) != hipSuccess)
        rc = fail(PTLS_HIP_ENODEV, "%s: upload failed", who);
    else if (int e = launch_quic_initial_keys(sp, d_dcids, d_lens, (uint32_t)count, labels, sc.keys, sc.ivs, sc.hps, stream))
        rc = fail(PTLS_HIP_ELAUNCH, "%s: derive launch failed: %s", who, hipGetErrorString((hipError_t)e));
    return quic_keys_finish(who, rc, ks, hp_ks, sc, first, 2 * count, nullptr, nullptr, 0, stream);
}

extern "C" int ptls_hip_keyset_get_iv(ptls_hip_keyset_t *ks, size_t slot, void *iv)
{
    if (ks == nullptr || slot >= ks->nslots)
        return fail(PTLS_HIP_EINVAL, "keyset_get_iv: bad slot");
    std::memcpy(iv, &ks->ivs[slot * 12], 12);
    return 0;
}

extern "C" int ptls_hip_keyset_set_iv(ptls_hip_keyset_t *ks, size_t slot, const void *iv, void *stream)
{
    if (ks == nullptr || slot >= ks->nslots)
        return fail(PTLS_HIP_EINVAL, "keyset_set_iv: bad slot");
    DeviceGuard g(ks->eng->device);
    std::memcpy(&ks->ivs[slot * 12], iv, 12);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *d_iv = ks->algo == PTLS_HIP_ALGO_CHACHA20POLY1305 ? static_cast<void *>(&ks->d_chacha[slot].iv)
                                                            : static_cast<void *>(&ks->d_slots[slot].iv);
    HIP_TRY(hipMemcpyAsync(d_iv, &ks->ivs[slot * 12], 12, hipMemcpyHostToDevice, s), PTLS_HIP_ENODEV);
    HIP_TRY(hipStreamSynchronize(s), PTLS_HIP_ENODEV);
    return 0;
}

extern "C" int ptls_hip_keyset_xor_iv(ptls_hip_keyset_t *ks, size_t slot, const void *bytes, size_t len, void *stream)
{
    if (ks == nullptr || slot >= ks->nslots || len > 12)
        return fail(PTLS_HIP_EINVAL, "keyset_xor_iv: bad arguments");
    uint8_t iv[12];
    std::memcpy(iv, &ks->ivs[slot * 12], 12);
    for (size_t i = 0; i < len; ++i)
        iv[i] ^= static_cast<const uint8_t *>(bytes)[i];
    return ptls_hip_keyset_set_iv(ks, slot, iv, stream);
}
