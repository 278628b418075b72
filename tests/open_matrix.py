"""The open-side authentication matrix (used by tests/test_open_matrix_ref.py and the test_gpu_*open_matrix.py files).

An open kernel can be wrong in a way no seal-parity or round-trip test sees: it can accept what it must reject.  From a
base record (key, iv, seq, aad, pt) and a `seal(key, iv, seq, aad, pt) -> ct || tag` callable this yields records as an
opener sees them: the CLAIMED fields (key, iv, seq, aad, length = len(sealed) - 16) and the PRESENTED bytes (`sealed`).
Every damaged case differs from a valid record in one field only:

  T  each of the 128 tag bits
  C  one bit in every 16-byte ciphertext block j, at byte (5 j + 3) mod n_j (n_j = the block's size) and bit j mod 8;
     chacha=True: one bit per 64-byte block, plus the first and the last byte of the partial tail
  A  one bit in every AAD byte
  S  each of the 64 sequence-number bits
  K  one bit in each of the 12 static-IV bytes and in each key byte (the record then names another key slot)
  L  the length fields: the base is built so that its last ciphertext byte and its last AAD byte are 0x00, which makes
     `len+1` (ct || 00), `len-1` (the zero byte dropped), `aad+1` (aad || 00) and `aad-1` hash the SAME zero-padded blocks
     as the base: only the length block of GHASH / Poly1305 tells them apart.  `len-16` and `len+16` (16 zero bytes) drop
     or add a whole block.  The tag is the base's in every case; a case whose field cannot shrink does not exist.

Intact copies of the base with sequence numbers of their own (kind I) make up at least a quarter of the list, which is
shuffled with a fixed seed so that damaged and intact records share wave tasks.  The K cases are then moved to the end
in their shuffled order: the AES batch kernel works on runs of one key slot, and K records scattered through the list
would cut the base key's run into pieces shorter than a wave task.

Pure Python, no GPU.  `verdicts` runs a list against a reference `open`; every generated case is meant to be run.
"""
import random
from collections import namedtuple

KINDS = "TCASKL"
L_CASES = ("len+1", "len-1", "aad+1", "aad-1", "len-16", "len+16")

# kind: one of KINDS or "I" (intact); what: the damaged bit / length case; key, iv, seq, aad: the claimed fields;
# sealed: the presented ct || tag (claimed length = len(sealed) - 16)
Case = namedtuple("Case", "kind what key iv seq aad sealed")


AAD_LEN = 21  # two AAD blocks, the second partial: the lanes' first data elements are shifted by two
TINY_SHAPES = ((0, 0), (0, 21), (1, 0), (16, 16))  # (L, A): run with T and whichever L cases exist
BASE_SEQ = 0x0123456789ABCDEF


def aes_len(G):
    """the AES batch kernel's base length at G lanes per record: 5 G + 1 full blocks = two iterations of the full-block
    stretch (PURE_BLOCKS = 2 blocks per lane each) and a generic element per lane, one more block, a 5-byte partial one"""
    return 16 * (5 * G + 1) + 5


def aes_len_of_elements(N, A=AAD_LEN):
    """the length whose GHASH input has N elements (AAD blocks + data blocks + the length block), 5-byte partial block"""
    return 16 * (N - (A + 15) // 16 - 2) + 5


def chacha_len(G):
    return 64 * (2 * G + 1) + 17


def claimed_len(case):
    return len(case.sealed) - 16


def _flip(data, byte, bit):
    b = bytearray(data)
    b[byte] ^= 1 << bit
    return bytes(b)


def damages(L, A, key_len, kinds=KINDS, chacha=False, c_every=1):
    """the (kind, what) descriptors of every damaged case of a record of L payload bytes and A AAD bytes.  c_every: the C
    kind takes every c_every-th block (the plugin's 16 KiB record); 1 everywhere else"""
    out = []
    if "T" in kinds:
        out += [("T", bit) for bit in range(128)]
    if "C" in kinds and L:
        bs = 64 if chacha else 16
        for j in range(0, (L + bs - 1) // bs, c_every):
            n_j = min(bs, L - bs * j)
            out.append(("C", (bs * j + (5 * j + 3) % n_j, j % 8)))
        if chacha and L % 64:
            for byte in sorted({L - L % 64, L - 1}):
                out.append(("C", (byte, 7 - byte % 8)))
    if "A" in kinds:
        out += [("A", (a, a % 8)) for a in range(A)]
    if "S" in kinds:
        out += [("S", bit) for bit in range(64)]
    if "K" in kinds:
        out += [("K", ("iv", b, b % 8)) for b in range(12)]
        out += [("K", ("key", b, (3 * b + 1) % 8)) for b in range(key_len)]
    if "L" in kinds:
        exists = {"len+1": True, "len-1": L >= 1, "aad+1": True, "aad-1": A >= 1, "len-16": L >= 16, "len+16": True}
        out += [("L", name) for name in L_CASES if exists[name]]
    return out


def prepare(base, seal):
    """the base with its last AAD byte and (by its last plaintext byte) its last ciphertext byte made 0x00, and its seal"""
    key, iv, seq, aad, pt = (base[0], base[1], base[2], bytes(base[3]), bytes(base[4]))
    if aad:
        aad = aad[:-1] + b"\x00"
    sealed = seal(key, iv, seq, aad, pt)
    if pt and sealed[len(pt) - 1]:
        pt = pt[:-1] + bytes([pt[-1] ^ sealed[len(pt) - 1]])  # both AEADs XOR a keystream: the ciphertext byte becomes 0
        sealed = seal(key, iv, seq, aad, pt)
    assert not pt or sealed[len(pt) - 1] == 0
    return (key, iv, seq, aad, pt), sealed


def apply(base, sealed, damage):
    """the damaged Case of a prepared base and its seal"""
    key, iv, seq, aad, pt = base
    kind, what = damage
    L = len(pt)
    ct, tag = sealed[:L], sealed[L:]
    if kind == "T":
        sealed = ct + _flip(tag, what // 8, what % 8)
    elif kind == "C":
        sealed = _flip(ct, *what) + tag
    elif kind == "A":
        aad = _flip(aad, *what)
    elif kind == "S":
        seq ^= 1 << what
    elif kind == "K":
        field, byte, bit = what
        if field == "iv":
            iv = _flip(iv, byte, bit)
        else:
            key = _flip(key, byte, bit)
    elif kind == "L":
        if what == "len+1":
            sealed = ct + b"\x00" + tag
        elif what == "len-1":
            assert ct[-1] == 0
            sealed = ct[:-1] + tag
        elif what == "aad+1":
            aad = aad + b"\x00"
        elif what == "aad-1":
            assert aad[-1] == 0
            aad = aad[:-1]
        elif what == "len-16":
            sealed = ct[:-16] + tag
        elif what == "len+16":
            sealed = ct + bytes(16) + tag
        else:
            raise ValueError(what)
    else:
        raise ValueError(kind)
    return Case(kind, what, key, iv, seq, aad, sealed)


def matrix(base, seal, kinds=KINDS, chacha=False, c_every=1, seed=2024, extra_intact=0):
    """the shuffled list of Cases of one base record.  base: (key, iv, seq, aad, pt), or a callable i -> such a record that
    gives every case a base of its own (its own key and therefore its own ciphertext); all bases must have one shape."""
    base_of = base if callable(base) else None
    if base_of is None:
        fixed = prepare(base, seal)
    first = prepare(base_of(0), seal)[0] if base_of else fixed[0]
    L, A, key_len = len(first[4]), len(first[3]), len(first[0])
    cases = []
    for i, dmg in enumerate(damages(L, A, key_len, kinds, chacha, c_every)):
        b, sealed = prepare(base_of(i), seal) if base_of else fixed
        assert (len(b[4]), len(b[3])) == (L, A)
        cases.append(apply(b, sealed, dmg))
    nd = len(cases)
    for k in range((nd + 2) // 3 + extra_intact):  # intact / all >= 1 / 4
        key, iv, seq, aad, pt = prepare(base_of(nd + k), seal)[0] if base_of else fixed[0]
        seq = (seq + 1 + k) & ((1 << 64) - 1)
        cases.append(Case("I", k, key, iv, seq, aad, seal(key, iv, seq, aad, pt)))
    random.Random(seed).shuffle(cases)
    return [c for c in cases if c.kind != "K"] + [c for c in cases if c.kind == "K"]


def verdicts(cases, open_):
    """[(accepted, output bytes)] of a reference open_(key, iv, seq, aad, sealed) -> (length or None, bytes)"""
    out = []
    for c in cases:
        n, pt = open_(c.key, c.iv, c.seq, c.aad, c.sealed)
        assert n is None or n == claimed_len(c)
        out.append((n is not None, pt))
    return out


def pt_ok_open(open_):
    """adapts tests/chacha_ref.py's open_ -> (plaintext, ok) to the (length or None, bytes) of `verdicts`"""
    def f(key, iv, seq, aad, sealed):
        pt, ok = open_(key, iv, seq, aad, sealed)
        return (len(pt) if ok else None), pt
    return f


def false_accepts(cases, accepted):
    """the damaged cases an opener accepted and the intact ones it rejected, as (kind, what) lists"""
    wrong_ok = [(c.kind, c.what) for c, ok in zip(cases, accepted) if ok and c.kind != "I"]
    wrong_fail = [(c.kind, c.what) for c, ok in zip(cases, accepted) if not ok and c.kind == "I"]
    return wrong_ok, wrong_fail
