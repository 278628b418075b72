"""Plain-Python / numpy model of the device-side receive step (include/ptls_hip.h 2i; hsig-picotls_amd/csrc/quic_rx.h): which
entries an open call selects, the sums the lane choice is made from, and the wave-per-record kernel's plan order.  Written
from the header's text; nothing here calls the library."""
import numpy as np

QRX_TILE = 1024  # csrc/internal.h
SCAN_SPAN = 2048  # csrc/internal.h QP_SCAN_SPAN
DIGITS = 64
ALL_TYPES = 0xFF


def selectable(p, type_, buf_len, out_len, nslots, hp_nslots, type_mask=ALL_TYPES, has_info=True):
    """one descriptor (a QUIC_PACKET_DTYPE record or a dict of ints)"""
    pn_offset, pkt_len = int(p["pn_offset"]), int(p["pkt_len"])
    if pn_offset == 0:
        return False
    if not pn_offset + 20 <= pkt_len <= 65535:
        return False
    if int(p["pkt_off"]) + pkt_len > buf_len:
        return False
    if int(p["data_off"]) + (pkt_len - pn_offset - 17) > out_len:
        return False
    if int(p["key"]) >= nslots or int(p["hp_key"]) >= hp_nslots:
        return False
    if has_info and (type_ > 31 or not (type_mask >> type_) & 1):
        return False
    return True


def select(pkts, info, buf_len, out_len, nslots, hp_nslots, type_mask=ALL_TYPES):
    """the entry indices an open call takes, in entry order (info: the info records, or None)"""
    return [k for k, p in enumerate(pkts)
            if selectable(p, int(info["type"][k]) if info is not None else 0, buf_len, out_len, nslots, hp_nslots, type_mask,
                          info is not None)]


def lens(pkts):
    """the provisional record lengths (pn_len = 1)"""
    return pkts["pkt_len"].astype(np.int64) - pkts["pn_offset"].astype(np.int64) - 17


def stats(pkts):
    """over selected descriptors: (sum of GHASH elements, sum of len // 64, key runs, max len >> 4, count)"""
    L = lens(pkts)
    aad = pkts["pn_offset"].astype(np.int64) + 1
    ghash = int(((aad + 15) // 16 + (L + 15) // 16 + 1).sum())
    keys = pkts["key"]
    runs = 1 + int((keys[1:] != keys[:-1]).sum()) if len(pkts) else 0
    return ghash, int((L // 64).sum()), runs, int((L >> 4).max()) if len(pkts) else 0, len(pkts)


def plan_order(pkts):
    """the sparse kernel's plan: selected positions in a stable order by decreasing 16-byte block count"""
    return np.argsort(-(lens(pkts) >> 4), kind="stable").astype(np.uint32)


def records(pkts):
    """the records quic_records makes of open descriptors (what the host planner sees): (aad_len, len, key) arrays"""
    return pkts["pn_offset"].astype(np.int64) + 1, lens(pkts), pkts["key"]


SPARSE_LANES, SPARSE_MAX_PER_RUN = 64, 20


def choose_lanes(ghash, runs, n, ncu):
    """planner.cpp choose_lanes_from, from the model's sums"""
    if n == 0:
        return 1
    mean, per_run = ghash / n, n / runs
    g = 4 if mean >= 48 else 2 if mean >= 16 else 1
    if per_run < SPARSE_MAX_PER_RUN:
        return SPARSE_LANES
    if mean >= 256 and per_run <= 64:
        return 32
    if mean >= 256 and per_run <= 128:
        return 16
    if mean >= 256 and per_run <= 320:
        return 8
    waves = 12.0 * (ncu or 256)
    while g < 32 and n * g / 64.0 < 2.0 * waves and mean / (2.0 * g) >= 8.0:
        g *= 2
    return g


def choose_chacha_lanes(blocks64, n, ncu):
    """planner.cpp choose_chacha_lanes_from"""
    if n == 0:
        return 1
    blocks = blocks64 / n
    want = 2048.0 * (ncu or 256)
    g = 4 if blocks >= 4 else 1
    while g < 64 and n * g < want and blocks >= 4.0 * g:
        g *= 4
    return g


def second_level_m():
    """the smallest m whose [digit][tile] count array (64 per tile) needs a second scan level"""
    return (SCAN_SPAN // DIGITS) * QRX_TILE + 1
