"""tests/chacha_ref.py (the plain-Python expected bytes of every ChaCha test) against the vectors of RFC 8439 and against
every entry of tests/golden/chacha20poly1305.json, the fixture recorded from picotls's own minicrypto engine.  No GPU."""
import hashlib
import importlib.util
import json
import os

import chacha_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_00_1F = bytes(range(32))
KEY_80_9F = bytes(range(0x80, 0xa0))
SUNSCREEN = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, sunscreen would be "
             b"it.")


def test_rfc8439_2_3_2_block():
    out = chacha_ref.chacha20_block(KEY_00_1F, 1, bytes.fromhex("000000090000004a00000000"))
    assert out.hex() == ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def test_rfc8439_2_4_2_encryption():
    out = chacha_ref.chacha20_xor(KEY_00_1F, 1, bytes.fromhex("000000000000004a00000000"), SUNSCREEN)
    assert out.hex() == ("6e2e359a2568f98041ba0728dd0d6981e97e7aec1d4360c20a27afccfd9fae0bf91b65c5524733ab8f593dabcd62b357"
                         "1639d624e65152ab8f530c359f0861d807ca0dbf500d6a6156a38e088a22b65e52bc514d16ccf806818ce91ab7793736"
                         "5af90bbf74a35be6b40b8eedf2785e42874d")


def test_rfc8439_2_5_2_mac():
    key = bytes.fromhex("85d6be7857556d337f4452fe42d506a80103808afb0db2fd4abff6af4149f51b")
    assert chacha_ref.poly1305_mac(b"Cryptographic Forum Research Group", key).hex() == "a8061dc1305136c6c22b8baf0c0127a9"


def test_rfc8439_2_6_2_key_generation():
    otk = chacha_ref.poly1305_key_gen(KEY_80_9F, bytes.fromhex("000000000001020304050607"))
    assert otk.hex() == "8ad5a08b905f81cc815040274ab29471a833b637e3fd0da508dbb8e2fdd1a646"


def test_rfc8439_2_8_2_aead():
    nonce, aad = bytes.fromhex("070000004041424344454647"), bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    out = chacha_ref.aead_encrypt(KEY_80_9F, nonce, SUNSCREEN, aad)
    assert out.hex() == ("d31a8d34648e60db7b86afbc53ef7ec2a4aded51296e08fea9e2b5a736ee62d63dbea45e8ca9671282fafb69da92728b"
                         "1a71de0a9e060b2905d6a5b67ecd3b3692ddbd7f2d778b8c9803aee328091b58fab324e4fad675945585808b4831d7bc"
                         "3ff4def08e4b7a9de576d26586cec64b6116" "1ae10b594f09e26a7e902ecbd0600691")
    assert chacha_ref.aead_decrypt(KEY_80_9F, nonce, out, aad) == SUNSCREEN


def test_rfc8439_appendix_a5_decryption():
    key = bytes.fromhex("1c9240a5eb55d38af333888604f6b5f0473917c1402b80099dca5cbc207075c0")
    nonce, aad = bytes.fromhex("000000000102030405060708"), bytes.fromhex("f33388860000000000004e91")
    ct = bytes.fromhex(
        "64a0861575861af460f062c79be643bd5e805cfd345cf389f108670ac76c8cb24c6cfc18755d43eea09ee94e382d26b0bdb7b73c321b0100"
        "d4f03b7f355894cf332f830e710b97ce98c8a84abd0b948114ad176e008d33bd60f982b1ff37c8559797a06ef4f0ef61c186324e2b350638"
        "3606907b6a7c02b0f9f6157b53c867e4b9166c767b804d46a59b5216cde7a4e99040c5a40433225ee282a1b0a06c523eaf4534d7f83fa115"
        "5b0047718cbc546a0d072b04b3564eea1b422273f548271a0bb2316053fa76991955ebd63159434ecebb4e466dae5a1073a6727627097a10"
        "49e617d91d361094fa68f0ff77987130305beaba2eda04df997b714d6c6f2c29a6ad5cb4022b02709b")
    tag = bytes.fromhex("eead9d67890cbb22392336fea1851f38")
    want = (b"Internet-Drafts are draft documents valid for a maximum of six months and may be updated, replaced, or obsoleted "
            b"by other documents at any time. It is inappropriate to use Internet-Drafts as reference material or to cite them "
            b"other than as /\xe2\x80\x9cwork in progress./\xe2\x80\x9d")
    assert chacha_ref.aead_decrypt(key, nonce, ct + tag, aad) == want
    bad = bytearray(ct + tag)
    bad[17] ^= 1
    assert chacha_ref.aead_decrypt(key, nonce, bytes(bad), aad) is None


def test_record_nonce_and_mask_rules():
    iv = bytes(range(12))
    assert chacha_ref.record_nonce(iv, 0) == iv
    assert chacha_ref.record_nonce(iv, 0x0102030405060708) == bytes([0, 1, 2, 3, 4 ^ 1, 5 ^ 2, 6 ^ 3, 7 ^ 4, 8 ^ 5, 9 ^ 6, 10 ^ 7,
                                                                     11 ^ 8])
    sample = bytes(range(100, 116))
    assert chacha_ref.hp_mask(KEY_00_1F, sample) == chacha_ref.chacha20_block(KEY_00_1F, 0x67666564, sample[4:])[:16]


def test_every_fixture_entry():
    with open(os.path.join(ROOT, "tests", "golden", "chacha20poly1305.json")) as f:
        gold = json.load(f)
    spec = importlib.util.spec_from_file_location("make_chacha_golden", os.path.join(ROOT, "tests", "golden",
                                                                                     "make_chacha_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert len(gold["records"]) == 200 and len(gold["masks"]) == 32
    assert {e["seq"] for e in gold["records"]} == {0, 1, (1 << 32) - 1, 1 << 32, (1 << 64) - 1}
    for e in gold["records"]:
        key, iv, seq, aad, pt = gen.record_inputs(e["i"])
        assert (len(pt), len(aad), seq) == (e["L"], e["A"], e["seq"]) and all(iv)
        out = chacha_ref.seal(key, iv, seq, aad, pt)
        assert hashlib.sha256(out).hexdigest() == e["sha256"], e["i"]
        assert ("out" in e) == (len(out) <= 256) and e.get("out", out.hex()) == out.hex(), e["i"]
        assert chacha_ref.open_(key, iv, seq, aad, out) == (pt, True)
    for e in gold["masks"]:
        key, iv, seq, aad, pt, hp_key, sample_off = gen.mask_inputs(e["j"])
        out = chacha_ref.seal(key, iv, seq, aad, pt)
        assert hashlib.sha256(out).hexdigest() == e["sha256"] and sample_off == e["sample_off"]
        assert chacha_ref.hp_mask(hp_key, out[sample_off: sample_off + 16]).hex() == e["mask"], e["j"]


def test_shared_open_equals_open():
    """SharedOpen (one keystream per (key, nonce), shared between cases) against open_: growing and shrinking lengths under
    one nonce, a damaged tag, ciphertext, AAD and sequence number"""
    key, iv, aad = KEY_80_9F, bytes(range(1, 13)), bytes(range(21))
    shared = chacha_ref.SharedOpen()
    for L in (0, 1, 63, 64, 65, 200, 129, 17):
        pt = hashlib.sha256(b"%d" % L).digest() * 7
        out = chacha_ref.seal(key, iv, 5, aad, pt[:L])
        cases = [(5, aad, out), (5, aad, out[:-1] + bytes([out[-1] ^ 0x80])), (5, aad[:-1], out), (4, aad, out)]
        if L:
            cases.append((5, aad, bytes([out[0] ^ 1]) + out[1:]))
            cases.append((5, aad, out[:L - 1] + out[L:]))
        for seq, a, sealed in cases:
            assert shared.open_(key, iv, seq, a, sealed) == chacha_ref.open_(key, iv, seq, a, sealed), (L, seq)
    assert shared.open_(key, iv, 5, aad, out) == (pt[:17], True)
