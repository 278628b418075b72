"""The plain-Python model of the device-side receive step (tests/quic_rx_ref.py) against independent statements of the same
things: the select rule against the text of include/ptls_hip.h 2i spelled out case by case, the sums against a per-packet
loop over the records ptls_hip_quic_batch_new makes (quic_records: AAD pn_offset + 1, length pkt_len - pn_offset - 17), the
plan order against Python's own stable sort, and the sizes the GPU tests take from it.

The model's lanes are pinned against the library's planner where that can run: without a device by
tests/test_quic_rx_native.py (planner.cpp's choose_lanes over quic_records' records, linked into a stand-alone program), and
through QuicBatch(open=True) and the inner batch's lane getters, which need a device, by tests/test_gpu_quic_rx.py."""
import random

import numpy as np

import ptls_hip
import quic_rx_ref as model


def _pkts(rows):
    p = np.zeros(len(rows), dtype=ptls_hip.QUIC_PACKET_DTYPE)
    for k, r in enumerate(rows):
        for f, v in r.items():
            p[f][k] = v
    return p


GOOD = dict(pkt_off=100, data_off=50, pkt_len=60, key=3, hp_key=2, pn_offset=9)


def test_select_rule_case_by_case():
    lim = dict(buf_len=1000, out_len=500, nslots=8, hp_nslots=4)
    ok = lambda type_=4, mask=0xFF, has_info=True, **kw: model.selectable(dict(GOOD, **kw), type_, type_mask=mask,  # noqa: E731
                                                                          has_info=has_info, **lim)
    assert ok()
    assert not ok(pn_offset=0)
    assert ok(pkt_len=29) and not ok(pkt_len=28)                       # pn_offset + 20
    assert ok(pkt_len=65535, pkt_off=0, data_off=0, pn_offset=65515) is False  # the area does not fit 500 bytes
    assert not ok(pkt_len=65536)
    assert ok(pkt_off=940) and not ok(pkt_off=941)                      # ends at buf_len / one past
    assert ok(data_off=500 - 34) and not ok(data_off=500 - 33)          # the area: 60 - 9 - 17 = 34 bytes
    assert ok(key=7) and not ok(key=8) and not ok(key=0xFFFFFFFF)
    assert ok(hp_key=3) and not ok(hp_key=4) and not ok(hp_key=0xFFFFFFFF)
    for t in range(8):
        assert ok(type_=t, mask=1 << t) and not ok(type_=t, mask=0xFF ^ (1 << t))
        assert ok(type_=t, mask=0, has_info=False)                      # no info records: the mask is ignored
    assert not ok(type_=32, mask=0xFFFFFFFF) and ok(type_=32, mask=0, has_info=False)


def test_select_keeps_entry_order_and_the_mask_applies_per_entry():
    rng = random.Random(5)
    rows = [dict(GOOD, pkt_off=100 * k, data_off=40 * k, key=rng.choice((0, 7, 8, ptls_hip.QUIC_NO_CONN)),
                 pn_offset=rng.choice((0, 9))) for k in range(200)]
    p = _pkts(rows)
    info = np.zeros(200, dtype=ptls_hip.QUIC_PKTINFO_DTYPE)
    info["type"] = [rng.choice((0, 2, 3, 4)) for _ in range(200)]
    every = model.select(p, info, 1 << 20, 1 << 20, 8, 8)
    assert every == sorted(every) and 40 < len(every) < 160
    assert all(rows[k]["pn_offset"] == 9 and rows[k]["key"] < 8 for k in every)
    hs, one = model.select(p, info, 1 << 20, 1 << 20, 8, 8, 1 << 2), model.select(p, info, 1 << 20, 1 << 20, 8, 8, 1 << 4)
    assert set(hs) | set(one) <= set(every) and not set(hs) & set(one)
    assert hs == [k for k in every if info["type"][k] == 2] and one == [k for k in every if info["type"][k] == 4]
    assert model.select(p, None, 1 << 20, 1 << 20, 8, 8, 0) == every


def test_sums_and_order_against_plain_loops():
    rng = random.Random(6)
    for n in (1, 2, 63, 500):
        p = _pkts([dict(pn_offset=rng.choice((1, 9, 47)), key=rng.randrange(4)) for _ in range(n)])
        p["pkt_len"] = [int(po) + 17 + rng.choice((0, 3, 15, 16, 17, 31, 32, 64, 1200, 65535 - 47 - 17)) for po in p["pn_offset"]]
        ghash = blocks = 0
        runs, max16 = 1, 0
        for k in range(n):
            aad, L = int(p["pn_offset"][k]) + 1, int(p["pkt_len"][k]) - int(p["pn_offset"][k]) - 17
            ghash += -(-aad // 16) - (-L // 16) + 1
            blocks += L // 64
            runs += k > 0 and p["key"][k] != p["key"][k - 1]
            max16 = max(max16, L >> 4)
        assert model.stats(p) == (ghash, blocks, runs, max16, n)
        assert max16 <= 4094
        want = sorted(range(n), key=lambda k: -((int(p["pkt_len"][k]) - int(p["pn_offset"][k]) - 17) >> 4))  # (sorted is stable)
        assert model.plan_order(p).tolist() == want
    assert model.stats(_pkts([])) == (0, 0, 0, 0, 0)


def test_sizes_the_gpu_tests_rely_on():
    assert model.QRX_TILE == 1024 and model.second_level_m() == 32 * 1024 + 1
    assert 64 * -(-model.second_level_m() // model.QRX_TILE) > model.SCAN_SPAN >= 64 * -(-(model.second_level_m() - 1) // model.QRX_TILE)
    with open(__file__.replace("tests/test_quic_rx_ref.py", "hsig-picotls_amd/csrc/internal.h")) as f:
        text = f.read()
    assert "constexpr uint32_t QRX_TILE = %d;" % model.QRX_TILE in text and "constexpr uint32_t QP_SCAN_SPAN = %d;" % model.SCAN_SPAN in text
    # the planner's rules on the shapes the issue names: interleaved connections take the wave-per-record kernel, one key does not
    assert model.choose_lanes(1000 * 80, 1000, 1000, 256) == model.SPARSE_LANES
    assert model.choose_lanes(64 * 77, 1, 64, 256) != model.SPARSE_LANES
