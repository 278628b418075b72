"""The seal-side exact-bytes matrix (tests/seal_exact_case.py) through every AES-GCM device path of the batch API.

The record-by-record seal tests copy into a zero-filled output buffer and read back each record's own bytes: a seal
kernel that stores a block late into a neighbour's line, stores zeros, or writes a byte past the tag into the gap behind it passes all of them.
Here every launch writes into buffers pre-filled with 0xA5 (masks: a position-dependent pattern; in place: random bytes)
and every byte of every buffer is compared with the CPU oracle's image:

  * the batch kernel at G = 1..32 lanes per record and the lanes = 64 kernel, both key sizes, in four layouts: "lines"
    (all offsets multiples of 16, the ALIGNED instantiation with its dword / 16-bit / 8-bit partial store, the deferred
    stores of records that do not start on a 128-byte line, and the unaligned tag store behind another lane's partial
    block; record i at block i mod 8 of a line, 16..112 fill bytes between records), "packed16", "bytes" (the unaligned
    instantiation) and "packed1" (no gaps);
  * lengths 16 k + r around every multiple of the stretch iteration, crossed with r and the line offset; AADs that rotate
    the lanes' first data elements; two key runs sorted by length, so wave tasks mix line-aligned and deferred records;
    every seventh record with a TLS 1.3 content type and a poison byte where the type goes;
  * in place; with QUIC header-protection masks; the TLS 1.3 framing into a wire buffer;
  * the sealed image opened again: the whole plaintext image and every result.

The same matrix run on the TEST-ONLY mutant build (batch_kernel.h SEAL_MUTANT 1: one byte 0x00 stored behind every tag
at G = 8 and 32) must report, in the "lines" layout where that byte is always fill, exactly one stray byte per record,
the one behind its tag, and nothing else.  (The record-by-record tests see that mutant only where the byte behind a tag
is a neighbour's first byte: 16-byte packed records whose length is a multiple of 16.)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import ptls_hip  # noqa: E402
import seal_exact_case as sx  # noqa: E402
from oracle_lib import tls13_wire  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
MUTANT = os.path.join(os.path.dirname(HERE), "hsig-picotls_amd", "mutants", "libptls_hip_seal1.so")
BATCH_GS = list(sx.BATCH_GS)


@pytest.mark.parametrize("layout", sx.LAYOUTS)
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", BATCH_GS)
def test_batch_kernel_seal_writes_exactly_the_records(engine, oracle, lanes, key_len, layout):
    r = sx.check(engine, oracle, sx.case(oracle, key_len, lanes), layout, lanes, wg=768)
    assert r.lanes == lanes


@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [4, 32])
def test_batch_kernel_seal_512_threads(engine, oracle, lanes, key_len):
    sx.check(engine, oracle, sx.case(oracle, key_len, lanes), "lines", lanes, wg=512)


@pytest.mark.parametrize("layout", sx.LAYOUTS)
@pytest.mark.parametrize("key_len", [16, 32])
def test_sparse_kernel_seal_writes_exactly_the_records(engine, oracle, key_len, layout):
    """lanes = 64, every record under a key of its own"""
    sx.check(engine, oracle, sx.case(oracle, key_len, 64), layout, 64)


@pytest.mark.parametrize("layout", ["lines", "bytes"])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", BATCH_GS + [64])
def test_seal_in_place_keeps_every_other_byte(engine, oracle, lanes, key_len, layout):
    """out == in: ct || tag replaces each plaintext and the 16 bytes behind it; the random bytes between the records stay"""
    sx.check(engine, oracle, sx.case(oracle, key_len, lanes), layout, lanes, wg=0 if lanes == 64 else 768, in_place=True)


@pytest.mark.parametrize("layout", ["lines", "bytes"])
@pytest.mark.parametrize("key_len", [16, 32])
@pytest.mark.parametrize("lanes", [4, 32, 64])
def test_seal_supp_masks_exact_on_device(engine, oracle, lanes, key_len, layout):
    """seal + header-protection masks in one launch: the masks of the enabled entries that name a key of the keyset, and
    not one byte more in a mask buffer whose prefill depends on the position (a zero-filled one cannot tell an untouched
    mask from a mask of zeros)"""
    r = sx.check(engine, oracle, sx.case(oracle, key_len, lanes), layout, lanes, wg=0 if lanes == 64 else 768, supp=True)
    n = len(sx.case(oracle, key_len, lanes).shapes)
    assert r.mask is not None and 0 < len(r.mask_offs) < n - n // 5


@pytest.mark.parametrize("bits", [128, 256])
def test_tls13_device_seal_writes_exactly_the_wire(engine, oracle, bits):
    """Batch.tls13_seal: headers and records of 40 messages, 1..64 bytes apart in a 0xA5 wire buffer; the whole wire buffer
    equals the prefill with picotls's framing restated (oracle_lib.tls13_wire) laid in, the message buffer is unchanged"""
    rng = np.random.default_rng(bits)
    nconn = 6
    keys = [oracle.gen_key(4100 + c, bits // 8) for c in range(nconn)]
    ks = ptls_hip.KeySet(engine, bits // 8, nconn)
    ks.set(0, b"".join(k for k, _ in keys), b"".join(iv for _, iv in keys))
    lens = [0, 1, 15, 16, 17, 1350, 16383, 16384, 16385, 40000] * 4
    conns = [i % nconn for i in range(len(lens))]
    types = [(21, 22, 23)[i % 3] for i in range(len(lens))]
    pts = [oracle.stream(4200 + i, L) for i, L in enumerate(lens)]
    seqs, nxt = [], [100 * c for c in range(nconn)]
    for c, L in zip(conns, lens):
        seqs.append(nxt[c])
        nxt[c] += (L + 16383) // 16384
    wires = [tls13_wire(oracle, *keys[c], s, t, p) for c, s, t, p in zip(conns, seqs, types, pts)]
    assert [len(w) for w in wires] == [ptls_hip.lib().ptls_hip_tls13_wire_size(L) for L in lens]
    wire_off, wire_size = sx._place(rng, [len(w) for w in wires], 64)
    in_off, in_size = sx._place(rng, lens, 4)
    h_in = sx.image(rng.integers(0, 256, in_size, dtype=np.uint8), in_off, pts)
    msgs = np.zeros(len(lens), dtype=ptls_hip.TLS13_MESSAGE_DTYPE)
    for m, L in enumerate(lens):
        msgs[m] = (in_off[m], wire_off[m], seqs[m], L, conns[m], types[m], 0)
    recs = ptls_hip.tls13_frame(msgs)
    assert len(recs) == sum((L + 16383) // 16384 for L in lens)
    wbase = np.full(wire_size, sx.FILL, np.uint8)
    d_in, d_wire = torch.from_numpy(h_in).cuda(), torch.from_numpy(wbase.copy()).cuda()
    b = ptls_hip.Batch(engine, recs)
    b.tls13_seal(ks, d_in, d_wire)
    torch.cuda.synchronize()
    b.close()
    ks.close()
    sx.same(d_wire.cpu().numpy(), sx.image(wbase, wire_off, wires), wire_off, [len(w) for w in wires], "TLS 1.3 wire buffer")
    sx.same(d_in.cpu().numpy(), h_in, in_off, lens, "TLS 1.3 message buffer")


def _mutant_run(lanes):
    if not os.path.exists(MUTANT):
        pytest.fail(f"{MUTANT} missing: build it with `make -C hsig-picotls_amd mutants` (part of __graft_entry__.build())")
    env = dict(os.environ, PTLS_HIP_LIB=MUTANT)
    out = subprocess.run([sys.executable, os.path.join(HERE, "seal_exact_case.py"), str(lanes), "16"], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = next(ln for ln in out.stdout.splitlines() if ln.startswith("MISMATCHES"))
    assert MUTANT in line, line
    return {k: v for k, v in (f.split("=", 1) for f in line.split()[1:])}


@pytest.mark.parametrize("lanes", [8, 32])
def test_seal_mutant_is_caught(oracle, lanes):
    """one byte 0x00 behind every tag: no byte inside a record is wrong (and the sealed image opens), and exactly one stray
    byte per record is reported, each right behind that record's tag"""
    got = _mutant_run(lanes)
    n = len(sx.case(oracle, 16, lanes).shapes)
    assert int(got["records"]) == n, got
    assert (int(got["inside"]), int(got["open"])) == (0, 0), got
    assert (int(got["outside"]), int(got["behind_tag"]), int(got["elsewhere"]), int(got["zeros"])) == (n, n, 0, n), got
