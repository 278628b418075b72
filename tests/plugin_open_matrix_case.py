"""The open-side authentication matrix (tests/open_matrix.py) through the picotls plugin objects' single-record decrypt
(run in its own process by tests/test_gpu_plugin_open_matrix.py, with and without the resident worker).

The worker takes AAD, IV, sequence number and lengths with each request.  A request that differs from the previous one in
one AAD bit, in its sequence number or in its IV only is the case in which state kept from the previous request becomes a
false accept.  So the calls alternate: the valid record, which must decrypt to its plaintext, then ONE damaged request
(each tag bit, a bit in every ciphertext block and every AAD byte, each sequence-number bit, the length cases: ciphertext
or AAD one byte shorter or longer with the same zero-padded bytes, a block shorter or longer), which therefore follows a
request that differs from it in that field only.  Then, for each of the 12 static-IV bytes: ptls_aead_xor_iv of one bit,
decrypt must fail; the same xor again restores the IV, decrypt must pass.  Expected verdicts: lib/fusion.c (oracle/_ref)
for AES-GCM, tests/chacha_ref.py for ChaCha20-Poly1305.

AES sizes in GHASH elements N (A = 21): 41 (one wave), 100 (mw_record, two waves), 154 (two pairs of waves at stride 128)
and 1 026 (16 KiB, where the C kind takes every 16th block)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "hsig-picotls_amd"), ROOT]

import chacha_ref  # noqa: E402
import open_matrix as om  # noqa: E402
import plugin_driver  # noqa: E402
from oracle_lib import Oracle, Ref  # noqa: E402

AES_N = (41, 100, 154, 1026)
CHACHA_LEN = 64 * 20 + 37
calls = 0


def run(drv, dec, base, seal, ref_open, tag, **kw):
    """valid, damaged, valid, damaged, ...; the valid record is the base every damaged case is made from"""
    global calls
    cases = om.matrix(base, seal, kinds="TCASL", **kw)
    b, sealed = om.prepare(base, seal)
    valid = om.Case("I", "base", b[0], b[1], b[2], b[3], sealed)
    n, pt = ref_open(valid.key, valid.iv, valid.seq, valid.aad, valid.sealed)
    assert n == om.claimed_len(valid), (tag, "the base does not open under the reference")
    for c in cases:
        assert (c.key, c.iv) == (valid.key, valid.iv)
        assert drv.decrypt(dec, valid.sealed, valid.seq, valid.aad) == pt, (tag, "valid before", c.kind, c.what)
        n, want = ref_open(c.key, c.iv, c.seq, c.aad, c.sealed)
        assert (n is None) == (c.kind != "I"), (tag, "reference", c.kind, c.what)
        got = drv.decrypt(dec, c.sealed, c.seq, c.aad)
        assert got == (None if n is None else want), (tag, "ACCEPTED" if got is not None else "rejected", c.kind, c.what)
        calls += 2
    for byte in range(12):
        flip = bytes(byte) + bytes([1 << (byte % 8)])
        drv.xor_iv(dec, flip)
        assert drv.decrypt(dec, valid.sealed, valid.seq, valid.aad) is None, (tag, "ACCEPTED under a damaged IV", byte)
        drv.xor_iv(dec, flip)
        assert drv.decrypt(dec, valid.sealed, valid.seq, valid.aad) == pt, (tag, "IV restored", byte)
        calls += 2
    assert drv.decrypt(dec, valid.sealed, valid.seq, valid.aad) == pt, (tag, "final")
    calls += 1


def main():
    drv, ref, o = plugin_driver.PluginDriver(), Ref(), Oracle()
    for bits in (128, 256):
        key, iv = o.gen_key(950 + bits, bits // 8)
        dec = drv.new(bits, key, iv, 0)
        for N in AES_N:
            L = om.aes_len_of_elements(N)
            base = (key, iv, om.BASE_SEQ + N, o.stream(7300 + N, om.AAD_LEN), o.stream(7400 + N, L))
            run(drv, dec, base, ref.seal, ref.open, (bits, N), c_every=16 if N > 1000 else 1)
        drv.free(dec)
    key, iv = o.stream(7500, 32), bytes(b | 1 for b in o.stream(7501, 12))
    dec = drv.new("chacha20poly1305", key, iv, 0)
    base = (key, iv, om.BASE_SEQ, o.stream(7502, om.AAD_LEN), o.stream(7503, CHACHA_LEN))
    run(drv, dec, base, chacha_ref.seal, om.pt_ok_open(chacha_ref.SharedOpen().open_), ("chacha", CHACHA_LEN), chacha=True)
    drv.free(dec)
    print("ok", calls, flush=True)


if __name__ == "__main__":
    main()
