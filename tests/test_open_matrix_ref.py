"""The open-side authentication matrix (tests/open_matrix.py) against the references alone: the C oracle's `open` for
AES-GCM and tests/chacha_ref.py's `open_` for ChaCha20-Poly1305 must reject 100 % of the damaged cases and accept 100 % of
the intact ones, at every shape the GPU tests run.  This pins the generator (every damaged case really is invalid, the
length cases included) and the references' verdicts, which are the GPU tests' expected results.  No GPU."""
import pytest

import chacha_ref
import open_matrix as om
import open_matrix_case as omc  # (the lists of the GPU tests; imports nothing of the device at module level)

BATCH_GS = (1, 2, 4, 8, 16, 32)
aes_base = omc.base


def check(cases, open_):
    ok = [v[0] for v in om.verdicts(cases, open_)]
    damaged = sum(1 for c in cases if c.kind != "I")
    assert 4 * (len(cases) - damaged) >= len(cases)
    assert om.false_accepts(cases, ok) == ([], [])
    return damaged


@pytest.mark.parametrize("key_len", [16, 32])
def test_generator_counts(oracle, key_len):
    L, A = om.aes_len(4), om.AAD_LEN
    cases = om.matrix(aes_base(oracle, key_len, L, A), oracle.seal)
    n = {k: sum(1 for c in cases if c.kind == k) for k in om.KINDS + "I"}
    blocks = (L + 15) // 16
    assert n == {"T": 128, "C": blocks, "A": A, "S": 64, "K": 12 + key_len, "L": 6, "I": (sum(n.values()) - n["I"] + 2) // 3}
    assert [c.kind for c in cases[-n["K"]:]] == ["K"] * n["K"]  # the foreign key slots come last
    assert len({(c.kind, repr(c.what)) for c in cases}) == len(cases)
    assert len({c.seq for c in cases if c.kind == "I"}) == n["I"]
    base = next(c for c in cases if c.kind == "T")
    assert base.sealed[L - 1] == 0 and base.aad[-1] == 0
    by = {c.what: c for c in cases if c.kind == "L"}
    assert [om.claimed_len(by[w]) - L for w in om.L_CASES] == [1, -1, 0, 0, -16, 16]
    assert [len(by[w].aad) - A for w in om.L_CASES] == [0, 0, 1, -1, 0, 0]
    intact_tag = next(c for c in cases if c.kind == "A").sealed[-16:]
    ct = next(c for c in cases if c.kind == "A").sealed[:L]
    for w in om.L_CASES:  # the base's tag and the base's bytes, only shorter or zero-extended
        c, n = by[w], min(L, om.claimed_len(by[w]))
        assert c.sealed[-16:] == intact_tag and (c.key, c.iv, c.seq) == (base.key, base.iv, base.seq)
        assert c.sealed[:n] == ct[:n] and not any(c.sealed[n:-16])
    # the same list every time
    again = om.matrix(aes_base(oracle, key_len, L, A), oracle.seal)
    assert again == cases


@pytest.mark.parametrize("key_len", [16, 32])
def test_aes_batch_shapes(oracle, key_len):
    damaged = 0
    for G in BATCH_GS:
        damaged += check(omc.batch_cases(oracle, key_len, G), oracle.open)
    assert damaged == 1809 + 6 * (key_len - 16)  # 3 714 over both key sizes


@pytest.mark.parametrize("key_len", [16, 32])
def test_aes_tiny_and_sparse_shapes(oracle, key_len):
    for L, A in om.TINY_SHAPES:
        cases = om.matrix(aes_base(oracle, key_len, L, A), oracle.seal, kinds="TL")
        want_l = 2 + (L >= 1) + (A >= 1) + (L >= 16) + 1
        assert sum(1 for c in cases if c.kind == "L") == want_l
        check(cases, oracle.open)
    tiny = omc.tiny_cases(oracle, key_len)
    assert sum(1 for c in tiny if c.kind == "T") == 4 * 128 and sum(1 for c in tiny if c.kind == "L") == 3 + 4 + 4 + 6
    check(tiny, oracle.open)
    for N in omc.SPARSE_N:  # lanes = 64: every record under its own key
        L = om.aes_len_of_elements(N)
        assert (om.AAD_LEN + 15) // 16 + (L + 15) // 16 + 1 == N
        cases = omc.sparse_cases(oracle, key_len, N)
        assert len({c.key for c in cases}) >= len(cases) - 1
        check(cases, oracle.open)


def chacha_base(L, A, j=0):
    s = chacha_ref.chacha20_block(bytes(range(32)), j, bytes(12))
    pt = b"".join(chacha_ref.chacha20_block(bytes(range(1, 33)), k, bytes(12)) for k in range(L // 64 + 1))[:L]
    return s[:32], bytes(b | 1 for b in s[32:44]), om.BASE_SEQ, s[40:40 + A], pt


def test_chacha_shapes():
    shared = chacha_ref.SharedOpen()
    for L, kinds in ((om.chacha_len(1), "TCAL"), (om.chacha_len(4), "TCAL"), (129, "SK")):
        cases = om.matrix(chacha_base(L, om.AAD_LEN), chacha_ref.seal, kinds=kinds, chacha=True)
        if "C" in kinds:
            assert sum(1 for c in cases if c.kind == "C") == (L + 63) // 64 + 2
        check(cases, om.pt_ok_open(shared.open_))
