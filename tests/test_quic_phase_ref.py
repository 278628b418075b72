"""The plain-Python model of the key chosen by Key Phase bit and of the commit (tests/quic_phase_ref.py) against case-by-case
statements of the rule (include/ptls_hip.h 2j), and the generated case list of the GPU tests (tests/quic_phase_cases.py)
against the reference alone: with the plain-Python packet protection (tests/quic_ref.py), every "must open" packet opens
under the key the model names and every "must fail" packet fails under it.  No GPU, no call into the library."""
import pytest

import quic_phase_cases as gen
import quic_phase_ref as model
import quic_ref

U64, NO_GEN = model.U64, model.NO_GEN
SHORT0, SHORT1 = 0x40, 0x44  # Key Phase bit clear / set


def test_the_rule_case_by_case():
    # the bit of the current generation: that generation, whatever the packet number
    for g, first in ((0, SHORT0), (1, SHORT1), (2, SHORT0), (7, SHORT1), (2 ** 32 - 2, SHORT0)):
        for pn in (0, 5, 1 << 61):
            for first_pn in (0, 5, 6, U64):
                assert model.choose(first, pn, g, first_pn) == g
    # the other bit, a packet number below first_pn: the previous generation
    assert model.choose(SHORT1, 4, 2, 5) == 1
    assert model.choose(SHORT0, 4, 3, 5) == 2
    assert model.choose(SHORT1, 0, 2 ** 32 - 2, 1) == 2 ** 32 - 3
    # ... at or above it: the peer has updated
    assert model.choose(SHORT1, 5, 2, 5) == 3
    assert model.choose(SHORT1, 6, 2, 5) == 3
    assert model.choose(SHORT0, 5, 2 ** 32 - 3, 5) == 2 ** 32 - 2
    # first_pn == UINT64_MAX: every packet with the other bit is a previous-generation packet
    assert model.choose(SHORT1, (1 << 62) - 1, 2, U64) == 1
    assert model.choose(SHORT0, 0, 1, U64) == 0
    # gen == 0 has no previous generation
    assert model.choose(SHORT1, 0, 0, 5) == 1
    assert model.choose(SHORT1, 0, 0, U64) == 1
    # first_pn == 0: nothing lies below it
    assert model.choose(SHORT1, 0, 4, 0) == 5
    # the other protected bits do not matter; the form bit decides alone
    for low in range(32):
        assert model.choose(0x40 | low, 9, 4, 5) == (4 if not low & 4 else 5)
        assert model.choose(0x00 | low, 3, 4, 5) == (4 if not low & 4 else 3)
    for first in range(0x80, 0x100):
        assert model.choose(first, 3, 4, 5) == NO_GEN


def test_the_slot_and_the_select_bound():
    assert [model.slot(7, 100, g) for g in range(7)] == [7, 107, 207, 7, 107, 207, 7]
    assert model.slot(7, 100, 2 ** 32 - 2) == 7 + 100 * ((2 ** 32 - 2) % 3)
    assert model.slot(7, 100, NO_GEN) == 7
    assert model.limit(137, 130) == 130 and model.limit(130, 137) == 130 and model.limit(5, 5) == 5
    # generation g + 2 overwrites g - 1, and three successive generations never share a slot
    for g in range(1, 9):
        assert model.slot(3, 10, g + 2) == model.slot(3, 10, g - 1)
        assert len({model.slot(3, 10, g - 1), model.slot(3, 10, g), model.slot(3, 10, g + 1)}) == 3


def test_the_commit_case_by_case():
    def run(table, rows):
        t = [list(e) for e in table]
        return model.commit(t, *zip(*rows)), t

    base = [[2, 50], [3, U64], [0, 7]]
    # authenticated next-generation packets advance: gen + 1, first_pn = their lowest packet number
    assert run(base, [(0, 10, 60, 3), (0, 10, 55, 3), (0, 10, 70, 3)]) == ([0], [[3, 55], [3, U64], [0, 7]])
    # a failed one does not (a forged packet with a flipped bit), nor does a packet of another connection
    assert run(base, [(0, U64, 60, 3)]) == ([], base)
    assert run(base, [(0, U64, 60, 3), (2, 0, 9, 1)]) == ([2], [[2, 50], [3, U64], [1, 9]])
    # current-generation packets lower first_pn, also from "none yet", and never raise it
    assert run(base, [(0, 5, 40, 2), (0, 5, 45, 2)]) == ([], [[2, 40], [3, U64], [0, 7]])
    assert run(base, [(1, 5, 1 << 40, 3)]) == ([], [[2, 50], [3, 1 << 40], [0, 7]])
    assert run(base, [(0, 5, 51, 2)]) == ([], base)
    assert run(base, [(0, U64, 40, 2)]) == ([], base)
    # next wins over current within one call: first_pn is the next generation's lowest, not the minimum of both
    assert run(base, [(0, 5, 3, 2), (0, 5, 90, 3)]) == ([0], [[3, 90], [3, U64], [0, 7]])
    # previous-generation, long-header and far-off generations change nothing
    assert run(base, [(0, 5, 3, 1), (0, 5, 3, NO_GEN), (0, 5, 3, 4), (0, 5, 3, 0)]) == ([], base)
    # a connection outside the table is ignored; the list is ascending whatever the packet order
    assert run(base, [(9, 5, 3, 1), (2, 1, 8, 1), (0, 1, 99, 3)]) == ([0, 2], [[3, 99], [3, U64], [1, 8]])
    # the order of the packets does not matter
    rows = [(0, 10, 60, 3), (0, 5, 41, 2), (1, 9, 12, 3), (1, 9, 11, 4), (2, 1, 8, 1), (2, 1, 6, 0), (0, 10, 58, 3)]
    assert run(base, rows) == run(base, rows[::-1]) == ([0, 1, 2], [[3, 58], [4, 11], [1, 8]])


@pytest.mark.parametrize("algo", quic_ref.ALGOS)
@pytest.mark.parametrize("make", [gen.three_banks, gen.one_key_only, gen.long_and_short])
def test_case_list_against_the_reference(algo, make):
    """every packet of the GPU tests' cases, opened by the plain-Python reference under the one key the model names"""
    case = make(algo)
    slots = case.slot_keys()
    opened = 0
    for p in case.packets:
        gen_, first_pn = case.states[p.conn]
        assert p.want_gen == model.choose(p.header[0], p.pn, gen_, first_pn)
        slot = case.want_slot(p)
        assert slot == (p.conn if p.long else p.conn + case.stride * (p.want_gen % 3)) and p.conn < model.limit(case.stride, case.count)
        key, iv = slots[slot]
        header, pn, pt, ok = quic_ref.unprotect(algo, key, iv, case.hps[p.conn], case.protected(p), p.pn_offset, p.expected)
        assert pn == p.pn and header == p.header
        assert ok == case.must_open(p), (p.conn, p.sealed, p.want_gen)
        if ok:
            assert pt == p.payload
            opened += 1
        elif not p.damaged:  # and it is the key that is wrong, not the packet: the generation it was sealed under opens it
            key, iv = case.keys[p.conn][case.sealed_generation(p)]
            assert quic_ref.unprotect(algo, key, iv, case.hps[p.conn], case.protected(p), p.pn_offset, p.expected)[3]
    assert opened == sum(case.must_open(p) for p in case.packets) > 0


def test_grouping_case_against_the_reference_and_its_geometry():
    """the bulk case of the commit's GPU test: labels against the reference, and the paths of the mark pass it is laid out for"""
    case = gen.grouping_case("aes128")
    slots = case.slot_keys()
    for p in case.packets[::7] + [q for q in case.packets if q.damaged][:20]:
        key, iv = slots[case.want_slot(p)]
        _, pn, _, ok = quic_ref.unprotect("aes128", key, iv, case.hps[p.conn], case.protected(p), p.pn_offset, p.expected)
        assert pn == p.pn and ok == case.must_open(p)
    paths = gen.mark_paths(case)
    assert paths["fold"] > 500 and paths["flush"] > 100 and paths["reduce"] >= 4 and paths["partial"] >= 2 and paths["split"] >= 2
    assert {13, 37} <= paths["low_lanes"]
    t = [list(s) for s in case.states]
    assert model.commit(t, *gen.commit_inputs(case)) == [1, 3] and t == [[2, 7], [2, 150], [4, 7594], [4, 7593]]


def test_every_branch_occurs_for_every_bank_and_parity():
    case = gen.three_banks("aes128")
    assert case.count == 130 and case.stride > 130 and len(case.packets) > 300
    seen = {"current": set(), "previous": set(), "next": set()}
    for p in case.packets:
        g = case.states[p.conn][0]
        branch = {g: "current", g - 1: "previous", g + 1: "next"}[p.want_gen]
        seen[branch].add((p.want_gen % 3, g & 1))
    for branch, got in seen.items():
        assert {b for b, _ in got} == {0, 1, 2} and {par for _, par in got} == {0, 1}, (branch, got)
    # every shape with every branch, and the first_pn classes: 0, in the middle (packets on both sides and ON it), none yet
    assert {(p.pn_len, len(p.payload)) for p in case.packets} == set(gen.SHAPES)
    assert {fp if fp in (0, U64) else "mid" for _, fp in case.states} == {0, "mid", U64}
    assert any(p.pn == case.states[p.conn][1] and p.want_gen == case.states[p.conn][0] + 1 for p in case.packets)
    # neighbours in the buffer mostly take different banks
    banks = [p.want_gen % 3 for p in case.packets]
    assert sum(a != b for a, b in zip(banks, banks[1:])) > len(banks) // 2
