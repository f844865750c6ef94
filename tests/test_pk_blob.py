"""CPU: the proving-key file's host-only parser (csrc/pkblob.hpp) through amdzk_pk_blob_info — pure host code, the checks
amdzk_pk_read makes before it touches the device — on files made by the independent Python encoder (tests/pk_blob.py), and
the same refusals once more in a stand-alone program built with ASan + UBSan (tests/native/pk_blob_check.cpp; no
sanitizer goes on anything loaded into Python)."""
import os
import struct
import subprocess
import sys
import tempfile

import pytest
import zkutil as zu

import circuits
import phased_circuits as PC
import phased_oracle as PO
import pk_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
_blobs = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def make(plonk, oracle, name):
    """(circuit, file) — made once per module and never modified."""
    if name not in _blobs:
        c = {"square": lambda: circuits.square_circuit(plonk, 4), "lookup": lambda: circuits.lookup_circuit(plonk, 5, seed=2),
             "rlc": lambda: PC.rlc_circuit(plonk, 5, seed=1)}[name]()
        odesc = PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])) if "challenge_phase" in c.desc else c.desc
        opk = PR.keygen(odesc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        _blobs[name] = (c, pk_blob.encode(plonk, oracle, c.desc, opk, REPR))
    return _blobs[name]


def refused(plonk, pkg, data):
    with pytest.raises(pkg.AmdzkError) as e:
        plonk.blob_info(data)
    return e.value.code == -2


@pytest.mark.parametrize("name", ["square", "lookup", "rlc"])
def test_blob_info_returns_the_shape_and_the_header_decodes_to_the_description(pkg, plonk, oracle, name):
    c, blob = make(plonk, oracle, name)
    assert plonk.blob_info(blob) == pk_blob.shape(c.desc)
    assert plonk.blob_info(bytearray(blob)) == pk_blob.shape(c.desc)
    # the description ProvingKey.read rebuilds flattens to the very header it came from
    desc = plonk.blob_desc(blob)
    assert pk_blob.header(plonk, desc) == pk_blob.header(plonk, c.desc) == blob[:len(pk_blob.header(plonk, c.desc))]
    assert pk_blob.shape(desc) == pk_blob.shape(c.desc) and desc.get("challenge_phase") == c.desc.get("challenge_phase")
    assert (name == "rlc") == (plonk.blob_info(blob)["num_challenges"] > 0)


def test_every_flipped_bit_position_and_every_truncation_is_refused(pkg, plonk, oracle):
    """Exhaustive on the k = 4 file (a few KB): one flipped bit at EVERY byte position (the bit walks with the position),
    and EVERY length 0 .. len - 1, and one byte too many. The library is called directly so that the loop stays quick."""
    import ctypes as C
    c, blob = make(plonk, oracle, "square")
    assert len(blob) < 16384
    L = pkg.lib()
    info = lambda buf, n: L.amdzk_pk_blob_info(buf, n, None, None, None, None, None)
    assert info(blob, len(blob)) == 0
    for i in range(len(blob)):
        m = bytearray(blob)
        m[i] ^= 1 << (i % 8)
        assert info(bytes(m), len(m)) == -2, "flipped bit at byte %d accepted" % i
    for n in range(len(blob)):
        assert info(blob[:n], n) == -2, "truncation to %d bytes accepted" % n
    assert info(blob + b"\0", len(blob) + 1) == -2
    assert info(None, 0) == -2 and info(None, len(blob)) == -2
    assert refused(plonk, pkg, blob[:-1]) and refused(plonk, pkg, b"")


@pytest.mark.parametrize("name", ["square", "lookup", "rlc"])
def test_counts_enlarged_to_2_pow_31_are_refused_without_a_large_allocation(pkg, plonk, oracle, name):
    """Every count field of the header set to 2^31, the digest recomputed (so only the parser's own bounds stand between
    the count and an allocation): refused, and the process's peak memory does not move by anything near 2^31 elements."""
    import resource
    c, blob = make(plonk, oracle, name)
    offsets = pk_blob.count_offsets(plonk, c.desc)
    assert ("num_challenges" in offsets) == (name == "rlc") and len(offsets) >= 12
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for field, off in offsets.items():
        body = bytearray(blob[:-64])
        old, = struct.unpack_from("<I", body, off)
        struct.pack_into("<I", body, off, 1 << 31)
        assert refused(plonk, pkg, pk_blob.seal(body)), field
        struct.pack_into("<I", body, off, old)
        assert pk_blob.seal(body) == blob
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert after - before < 64 * 1024, "peak RSS grew by %d KiB" % (after - before)  # 2^31 of anything is >= 2 GiB


def test_inconsistent_headers_with_a_valid_digest_are_refused(pkg, plonk, oracle):
    """The checks keygen makes on a circuit, on a file whose digest is right: cs_degree < 3, too few rows, an expression
    count that does not add up, a bad format version, a bad has-phases byte, k out of range."""
    c, blob = make(plonk, oracle, "lookup")
    off = pk_blob.count_offsets(plonk, c.desc)

    def patched(at, value, fmt="<I"):
        body = bytearray(blob[:-64])
        struct.pack_into(fmt, body, at, value)
        return pk_blob.seal(body)

    hp = off["num_perm_columns"] + 4 + 8 * len(c.desc["permutation_columns"])  # the has-phases byte
    assert blob[hp] == 0
    for at, value, fmt in ((32, 2, "<I"), (28, (1 << 5) - 2, "<I"), (off["num_gates"], len(c.desc["gates"]) + 1, "<I"), (8, 2, "<I"),
                           (hp, 2, "<B"), (12, 29, "<I"), (12, 0, "<I"), (0, ord("B"), "<B")):
        assert refused(plonk, pkg, patched(at, value, fmt)), (at, value)
    assert plonk.blob_info(patched(8, 1)) == pk_blob.shape(c.desc)


def test_blob_info_says_why_without_a_device(pkg, plonk, oracle):
    """amdzk_pk_blob_check: the refusal's reason, as ProvingKey.read would word it, from pure host code; "" for a good file,
    a short buffer truncates and stays terminated."""
    import ctypes as C
    c, blob = make(plonk, oracle, "square")
    body = bytearray(blob[:-64])
    struct.pack_into("<I", body, 16, (1 << 16) + 1)  # num_fixed
    for data, why in ((b"x" + blob[1:], "pk_read: bad magic"), (blob[:-1], "pk_read: length mismatch"), (blob[:40], "pk_read: .*too few"),
                      (blob[:100] + bytes([blob[100] ^ 4]) + blob[101:], "pk_read: digest mismatch"), (None, "pk_read: null data"),
                      (blob[:8] + struct.pack("<I", 2) + blob[12:], "pk_read: format version 2"),
                      (pk_blob.seal(body), "pk_read: more than 65536 columns of one kind")):
        with pytest.raises(pkg.AmdzkError, match=why) as e:
            plonk.blob_info(data)
        assert e.value.code == -2
    L, msg = pkg.lib(), C.create_string_buffer(b"?" * 63, 64)
    assert L.amdzk_pk_blob_check(blob, len(blob), msg, 64) == 0 and msg.value == b""
    assert L.amdzk_pk_blob_check(blob, len(blob) - 1, msg, 12) == -2 and msg.value == b"pk_read: le" and msg.raw[12:16] == b"????"
    assert L.amdzk_pk_blob_check(blob, len(blob) - 1, None, 0) == -2


def test_refusals_in_a_standalone_program_under_asan_and_ubsan(plonk, oracle, tmp_path):
    """tests/native/pk_blob_check.cpp includes only the host-only header: every flipped bit, every truncation, every
    enlarged count on exact-size heap copies — an out-of-bounds read of the parser is a sanitizer report."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "pk_blob_check")
    subprocess.check_call(["g++", *SAN, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "pk_blob_check.cpp")])
    for name in ("square", "rlc"):
        c, blob = make(plonk, oracle, name)
        path = str(tmp_path / (name + ".pk"))
        with open(path, "wb") as f:
            f.write(blob)
        p = subprocess.run([exe, path], text=True, capture_output=True, env=ENV, timeout=600)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
        assert "pk_blob_check ok" in p.stdout and "FAILED" not in p.stdout
        assert "flips %d refused" % len(blob) in p.stdout and "truncations %d refused" % len(blob) in p.stdout
        s = pk_blob.shape(c.desc)
        assert "parsed k %d fixed %d advice %d perm %d challenges %d" % (s["k"], s["num_fixed"], s["num_advice"], s["num_perm_columns"], s["num_challenges"]) in p.stdout
