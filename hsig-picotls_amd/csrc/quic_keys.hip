/*
 * quic_keys.hip -- QUIC packet-protection keys on the device, for many connections at once (RFC 9001 §5.1, §5.2, §6;
 * RFC 9369 §3.3), as picotls derives them on the host for one (ptls_hkdf_expand_label with the "tls13 quic " prefix of
 * ptls_aead_new, lib/picotls.c).  The arithmetic is quic_keys.h, shared with the CPU check; the kernels are loops over it.
 *
 *   quic_derive_keys_kernel    one thread per connection: key / iv / hp of its traffic secret, after the "ku" step if asked
 *   quic_initial_keys_kernel   one thread per (connection, side): HKDF-Extract(salt, DCID), "client in" / "server in", then
 *                              key / iv / hp; the Extract is recomputed by both sides' threads (two compression calls of
 *                              fourteen), the salt's pads arrive hashed as kernel arguments
 *
 * Both write packed raw keys, IVs and header-protection keys; keyset.cpp expands them into the two keysets.  The pad state
 * of a secret is hashed once and serves every label under it (quic_keys.h hk_quic_keys).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"
#include "quic_keys.h"

namespace ptls_hip {

__global__ void __launch_bounds__(64) quic_derive_keys_kernel(const uint8_t *__restrict__ secrets_in, uint8_t *__restrict__ secrets_out,
                                                              uint32_t count, int hash_size, uint32_t key_size, int update, int v2,
                                                              uint8_t *__restrict__ keys, uint8_t *__restrict__ ivs,
                                                              uint8_t *__restrict__ hps)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count)
        return;
    const uint8_t *secret = secrets_in + (size_t)i * hash_size;
    uint8_t *next = secrets_out != nullptr ? secrets_out + (size_t)i * hash_size : nullptr;
    uint8_t *key = keys + (size_t)i * key_size, *iv = ivs + (size_t)i * 12;
    uint8_t *hp = hps != nullptr ? hps + (size_t)i * key_size : nullptr;
    if (hash_size == 32)
        hk_quic_keys_from_secret<HkSha256>(secret, update, v2, key_size, next, key, iv, hp);
    else
        hk_quic_keys_from_secret<HkSha384>(secret, update, v2, key_size, next, key, iv, hp);
}

__global__ void __launch_bounds__(64) quic_initial_keys_kernel(QuicSaltPads salt, const uint8_t *__restrict__ dcids,
                                                               const uint8_t *__restrict__ dcid_lens, uint32_t count, int v2,
                                                               uint8_t *__restrict__ keys, uint8_t *__restrict__ ivs,
                                                               uint8_t *__restrict__ hps)
{
    const uint64_t t = (uint64_t)blockIdx.x * 64 + threadIdx.x; /* 2 * connection + side */
    if (t >= 2 * (uint64_t)count)
        return;
    const uint64_t conn = t >> 1;
    HkPads<HkSha256> p;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        p.in[k] = salt.in[k], p.out[k] = salt.out[k];
    uint32_t len = dcid_lens[conn];
    len = len < HK_DCID_STRIDE ? len : HK_DCID_STRIDE; /* (the host has refused longer ones) */
    hk_quic_initial_keys(p, dcids + conn * HK_DCID_STRIDE, len, (int)(t & 1), v2, keys + t * 16, ivs + t * 12, hps + t * 16);
}

int launch_quic_derive_keys(const uint8_t *secrets_in, uint8_t *secrets_out, uint32_t count, int hash_size, int key_size,
                            int update, int labels, uint8_t *keys, uint8_t *ivs, uint8_t *hps, void *stream)
{
    hipLaunchKernelGGL(quic_derive_keys_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), secrets_in,
                       secrets_out, count, hash_size, (uint32_t)key_size, update, labels == PTLS_HIP_QUIC_LABELS_V2 ? 1 : 0, keys,
                       ivs, hps);
    return (int)hipGetLastError();
}

int launch_quic_initial_keys(const QuicSaltPads &salt, const uint8_t *dcids, const uint8_t *dcid_lens, uint32_t count,
                             int labels, uint8_t *keys, uint8_t *ivs, uint8_t *hps, void *stream)
{
    const unsigned grid = (unsigned)((2 * (uint64_t)count + 63) / 64);
    hipLaunchKernelGGL(quic_initial_keys_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), salt, dcids, dcid_lens,
                       count, labels == PTLS_HIP_QUIC_LABELS_V2 ? 1 : 0, keys, ivs, hps);
    return (int)hipGetLastError();
}

} // namespace ptls_hip
