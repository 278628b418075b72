/*
 * quic_phase.h -- which generation of 1-RTT receive keys a packet is opened under, and how a connection's key-phase state
 * moves on (RFC 9001 §6; include/ptls_hip.h 2j), written for host and device like quic.h and quic_rx.h:
 * quic_phase_kernel.hip runs exactly these functions, and tests/test_quic_phase_native.py compiles them on the host and
 * checks them against the plain-Python model (tests/quic_phase_ref.py).
 *
 * The keys of generation g of connection c live in slot c + stride * (g % 3) of one AEAD keyset: three banks hold the
 * previous, the current and the next generation, and generation g + 2 overwrites g - 1 (RFC 9001 §6.5).  Exactly one
 * generation is tried per packet.
 */
#pragma once

#include <stdint.h>

#include "ptls_hip.h"

/* the function qualifier shared with gf128.h, quic.h and quic_rx.h: a host-only build defines it before the include */
#ifndef GF128_FN
#define GF128_FN __host__ __device__ __forceinline__
#endif
#define QPH_FN GF128_FN

namespace ptls_hip {

/* the first byte as the receiver reads it: with `masked`, the header-protection mask (its first word m0) removed from the
 * protected bits (the low four of a long header, the low five of a short one; the form bit 0x80 is never masked) */
QPH_FN uint32_t quic_phase_first_byte(uint32_t first, bool masked, uint32_t m0)
{
    return masked ? first ^ (m0 & ((first & 0x80u) != 0 ? 0x0fu : 0x1fu)) : first;
}

/* The generation whose keys open a packet with unmasked first byte `first` and decoded packet number pn, for a connection
 * whose current generation is `gen` (its Key Phase bit is gen & 1) and whose lowest packet number opened under it is first_pn
 * (UINT64_MAX: none yet, so every packet with the other bit is from before the update; gen == 0 has no previous generation).
 * A long header carries no Key Phase bit: PTLS_HIP_QUIC_NO_GEN, whatever its low bits are.  gen <= 2^32 - 2. */
QPH_FN uint32_t quic_phase_gen(uint32_t first, uint64_t pn, uint32_t gen, uint64_t first_pn)
{
    if ((first & 0x80u) != 0)
        return PTLS_HIP_QUIC_NO_GEN;
    const uint32_t bit = (first >> 2) & 1u;
    if (bit == (gen & 1u))
        return gen;
    if (gen > 0 && pn < first_pn)
        return gen - 1u; /* a reordered packet from before the update */
    return gen + 1u;     /* the peer has updated */
}

/* the AEAD key slot of a packet of connection `key` under generation gen_out (NO_GEN: the connection's own slot) */
QPH_FN uint32_t quic_phase_slot(uint32_t key, uint32_t stride, uint32_t gen_out)
{
    return gen_out == PTLS_HIP_QUIC_NO_GEN ? key : key + stride * (gen_out % 3u);
}

/* What an opened packet means for its connection's state: only authenticated short-header packets of the current or of the
 * next generation count (RFC 9001 §6.3: a forged packet with a flipped bit must not advance a connection). */
enum { QPH_NONE = 0, QPH_CURRENT = 1, QPH_NEXT = 2 };
QPH_FN int quic_phase_class(uint64_t result, uint32_t gen_out, uint32_t gen)
{
    if (result == UINT64_MAX || gen_out == PTLS_HIP_QUIC_NO_GEN)
        return QPH_NONE;
    if (gen_out == gen)
        return QPH_CURRENT;
    return (uint64_t)gen_out == (uint64_t)gen + 1u ? QPH_NEXT : QPH_NONE;
}

/* a connection has packets of the next generation: min_next = the lowest packet number among them, or UINT64_MAX for none */
QPH_FN bool quic_phase_updates(uint64_t min_next)
{
    return min_next != UINT64_MAX;
}

/* The state after a call: min_next / min_cur = the lowest packet numbers of the call's QPH_NEXT / QPH_CURRENT packets of the
 * connection (UINT64_MAX: none).  Packet numbers are below 2^62, so UINT64_MAX is never one. */
QPH_FN void quic_phase_apply(ptls_hip_quic_keyphase_t *st, uint64_t min_next, uint64_t min_cur)
{
    if (quic_phase_updates(min_next)) {
        st->gen += 1u;
        st->first_pn = min_next;
    } else if (min_cur < st->first_pn) {
        st->first_pn = min_cur;
    }
}

} // namespace ptls_hip
