/*
 * quic_track.h -- which received packet numbers a packet-number space has accepted, and what a further packet is against
 * that (RFC 9000 §12.3, §13.2.3; include/ptls_hip.h 2k), written for host and device like quic_phase.h:
 * quic_track_kernel.hip runs exactly these functions, and tests/test_quic_track_native.py compiles them on the host and
 * checks them against the plain-Python model (tests/quic_track_ref.py).
 *
 * The state of a space is (next, window): next = the largest accepted packet number + 1 (0: none yet), bit k of window =
 * packet number next - 1 - k has been accepted.  A packet is judged against the state BEFORE the call; the state after it is
 * made of a maximum and an OR over the call's new packets, so the outcome does not depend on the order or the grouping in
 * which the packets are looked at.  Duplicates inside one call are found through an open-addressing table of selected
 * positions, in which the lowest position of a key wins (a minimum).
 */
#pragma once

#include <stdint.h>

#include "ptls_hip.h"
#include "quic_parse.h"

#define QTK_FN QUIC_FN

namespace ptls_hip {

constexpr uint32_t QTK_WINDOW = 64;
constexpr uint32_t QTK_EMPTY = 0xffffffffu; /* an empty table slot; selected positions are below 2^32 - 1 */

/* The place 3 c + s of a selected packet in the state table, or UINT64_MAX when it is not tracked: it failed authentication,
 * its connection lies outside the table, or its type has no packet-number space. */
QTK_FN uint64_t quic_track_place(uint64_t result, uint32_t conn, uint64_t count, uint32_t type)
{
    if (result == UINT64_MAX || conn >= count)
        return UINT64_MAX;
    if (type != QP_INITIAL && type != QP_ZERO_RTT && type != QP_HANDSHAKE && type != QP_ONE_RTT)
        return UINT64_MAX;
    return 3 * (uint64_t)conn + quic_pn_space(type);
}

/* a tracked packet against the state before the call: TOO_OLD, DUPLICATE, or NONE for "new unless the call holds it twice" */
QTK_FN uint32_t quic_track_old(uint64_t pn, uint64_t next, uint64_t window)
{
    if (pn >= next)
        return PTLS_HIP_QUIC_PN_NONE;
    const uint64_t back = next - 1 - pn;
    if (back >= QTK_WINDOW)
        return PTLS_HIP_QUIC_PN_TOO_OLD;
    return (window >> back) & 1u ? PTLS_HIP_QUIC_PN_DUPLICATE : PTLS_HIP_QUIC_PN_NONE;
}

/* the window moved on by `by` packet numbers */
QTK_FN uint64_t quic_track_shift(uint64_t window, uint64_t by)
{
    return by >= QTK_WINDOW ? 0 : window << by;
}

/* next after the call: top = 1 + the largest new packet number of the call (0: none) */
QTK_FN uint64_t quic_track_next(uint64_t next, uint64_t top)
{
    return top > next ? top : next;
}

/* the window bit of new packet pn under the next of after the call, or 0 when it lies further back than the window reaches */
QTK_FN uint64_t quic_track_bit(uint64_t next_after, uint64_t pn)
{
    const uint64_t back = next_after - 1 - pn;
    return back < QTK_WINDOW ? (uint64_t)1 << back : 0;
}

/* the state after a call with new packets: top as above (not 0), bits = the OR of quic_track_bit(next after, pn) over them */
QTK_FN void quic_track_apply(ptls_hip_quic_pnspace_t *st, uint64_t top, uint64_t bits)
{
    const uint64_t after = quic_track_next(st->next, top);
    st->window = quic_track_shift(st->window, after - st->next) | bits;
    st->next = after;
}

/* ---- the table of the call's candidates: `size` slots (a power of two, at least twice the selected packets), each EMPTY or a
 * selected position whose key (place, pn) is read back through that position ---- */

/* slots for m selected packets: the power of two that is at least 2 m (and at least 2) */
QTK_FN uint64_t quic_track_slots(uint64_t m)
{
    uint64_t size = 2;
    while (size < 2 * m)
        size <<= 1;
    return size;
}

/* the 64-bit finalizer of MurmurHash3 over place and pn mixed (the table index takes the low bits) */
QTK_FN uint64_t quic_track_hash(uint64_t place, uint64_t pn)
{
    uint64_t h = pn ^ (place * 0x9e3779b97f4a7c15ull);
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

QTK_FN uint64_t quic_track_first(uint64_t place, uint64_t pn, uint64_t size)
{
    return quic_track_hash(place, pn) & (size - 1);
}

QTK_FN uint64_t quic_track_after(uint64_t at, uint64_t size)
{
    return (at + 1) & (size - 1);
}

/* Position j with key (place, pn) enters the table.  Ops gives the two accesses (cas returning what the slot held, min):
 * atomics on the device, plain code in the single-threaded host check.  Keys::same(occupant, place, pn) compares through the
 * read-only inputs.  Every slot is tried with the cas itself (one round trip where it is empty, which at load <= 0.5 most
 * are); a failed cas has re-read the slot: it is judged by the occupant it returned.  An occupant is only ever replaced by a
 * lower position with the same key, so a comparison stays valid whoever else runs.  At most `size` slots are looked at: false
 * (never, at load <= 0.5) when all of them hold other keys. */
template <class Ops, class Keys>
QTK_FN bool quic_track_claim(uint32_t *table, uint64_t size, uint32_t j, uint64_t place, uint64_t pn, const Keys &keys)
{
    uint64_t at = quic_track_first(place, pn, size);
    for (uint64_t step = 0; step < size; ++step) {
        const uint32_t occ = Ops::cas(table + at, QTK_EMPTY, j);
        if (occ == QTK_EMPTY)
            return true;
        if (keys.same(occ, place, pn)) {
            Ops::min(table + at, j);
            return true;
        }
        at = quic_track_after(at, size);
    }
    return false;
}

/* after every claim: the lowest position that holds key (place, pn), or QTK_EMPTY when none entered */
template <class Keys>
QTK_FN uint32_t quic_track_find(const uint32_t *table, uint64_t size, uint64_t place, uint64_t pn, const Keys &keys)
{
    uint64_t at = quic_track_first(place, pn, size);
    for (uint64_t step = 0; step < size; ++step) {
        const uint32_t occ = table[at];
        if (occ == QTK_EMPTY)
            return QTK_EMPTY;
        if (keys.same(occ, place, pn))
            return occ;
        at = quic_track_after(at, size);
    }
    return QTK_EMPTY;
}

} // namespace ptls_hip
