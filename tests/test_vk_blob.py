"""CPU: the verifying-key file's host-only parser (csrc/vkblob.hpp) through amdzk_vk_blob_info / amdzk_vk_blob_check — pure
host code, every check amdzk_vk_read makes — on files made by the independent Python encoder (tests/vk_blob.py) from the
oracle's key, and the same refusals once more in a stand-alone program built with ASan + UBSan
(tests/native/vk_blob_check.cpp; no sanitizer goes on anything loaded into Python)."""
import ctypes as C
import os
import re
import resource
import struct
import subprocess
import sys

import pytest

import circuits
import pairing_ref as PRF
import phased_circuits as PC
import phased_oracle as PO
import pk_blob
import vk_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
G = PRF.G1_GEN  # the generator times 1
G2, S_G2 = PRF.G2_GEN, PRF.g2_mul(PRF.G2_GEN, TAU)
NAMES = ["square", "lookup", "rlc"]
COUNT_REASONS = "truncated|more than 65536 columns|expression count mismatch"  # what an enlarged count runs into first
_made = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def make(plonk, oracle, name, with_g2):
    """(circuit, oracle key, VK file, pk file) — made once per module and never modified."""
    if name not in _made:
        c = {"square": lambda: circuits.square_circuit(plonk, 4), "lookup": lambda: circuits.lookup_circuit(plonk, 5, seed=2),
             "rlc": lambda: PC.rlc_circuit(plonk, 5, seed=1)}[name]()
        odesc = PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])) if "challenge_phase" in c.desc else c.desc
        opk = PR.keygen(odesc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        files = [vk_blob.encode(plonk, c.desc, opk.fixed_commitments, opk.permutation_commitments, REPR, G, *pair) for pair in ((), (G2, S_G2))]
        _made[name] = (c, opk, files, pk_blob.encode(plonk, oracle, c.desc, opk, REPR))
    c, opk, files, pkfile = _made[name]
    return c, opk, files[1 if with_g2 else 0], pkfile


def check(pkg, data):
    """(status, message) of amdzk_vk_blob_check; amdzk_vk_blob_info must agree."""
    L, msg = pkg.lib(), C.create_string_buffer(256)
    rc = L.amdzk_vk_blob_check(data, 0 if data is None else len(data), msg, len(msg))
    assert L.amdzk_vk_blob_info(data, 0 if data is None else len(data), None, None, None, None, None, None) == rc
    return rc, msg.value.decode()


def mutants(plonk, c, blob, with_g2):
    """[(name, file, reason)]: the digest recomputed, so that only the parser's own checks stand. The reasons are the
    documented ones (include/amdzk.h): which check a mutation must run into follows from the layout, not from a run."""
    off, out = vk_blob.offsets(plonk, c.desc, with_g2), []

    def patched(at, data):
        body = bytearray(blob[:-64])
        body[at:at + len(data)] = data
        return vk_blob.seal(body)

    q = PRF.P.to_bytes(32, "little")  # the modulus itself: the smallest value that is not a residue
    flip = lambda at: bytes([blob[at] ^ 1])
    for field, at in pk_blob.count_offsets(plonk, c.desc).items():  # the circuit section sits where the pk file has it
        out.append(("count_" + field, patched(at, struct.pack("<I", 1 << 31)), COUNT_REASONS))
    first = off["fixed_commitments"]  # every circuit here has a fixed column
    out += [("commitment_off_curve", patched(first + 32, flip(first + 32)), "commitment 0 is not on the curve"),
            ("commitment_coordinate", patched(first, q), "commitment 0 has a coordinate that is not below the modulus"),
            ("perm_commitment_off_curve", patched(off["perm_commitments"], flip(off["perm_commitments"])),
             "commitment %d is not on the curve" % c.desc["num_fixed"]),
            ("g_identity", patched(off["g"], bytes(64)), "G is the identity"),
            ("g_off_curve", patched(off["g"] + 32, flip(off["g"] + 32)), "G is not on the curve"),
            ("g_coordinate", patched(off["g"] + 32, q), "G has a coordinate that is not below the modulus"),
            ("has_g2_2", patched(off["has_g2"], b"\x02"), "has-g2 byte is 2")]
    if with_g2:
        out += [("g2_off_twist", patched(off["g2"] + 64, flip(off["g2"] + 64)), "g2 is not on the twist"),
                ("s_g2_off_twist", patched(off["s_g2"], flip(off["s_g2"])), "s_g2 is not on the twist"),
                ("g2_coordinate", patched(off["g2"] + 32, q), "g2 has a coordinate that is not below the modulus"),
                ("s_g2_coordinate", patched(off["s_g2"] + 96, q), "s_g2 has a coordinate that is not below the modulus"),
                ("g2_identity", patched(off["g2"], bytes(128)), "g2 is the identity")]
    return out


def identity_commitment_file(plonk, c, blob, with_g2):
    body = bytearray(blob[:-64])
    at = vk_blob.offsets(plonk, c.desc, with_g2)["fixed_commitments"]
    body[at:at + 64] = bytes(64)
    return vk_blob.seal(body)


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_blob_info_returns_the_shape_and_the_circuit_section_is_the_pk_files(pkg, plonk, oracle, name, with_g2):
    c, opk, blob, pkfile = make(plonk, oracle, name, with_g2)
    assert plonk.vk_blob_info(blob) == vk_blob.shape(c.desc, with_g2) and plonk.vk_blob_info(bytearray(blob)) == vk_blob.shape(c.desc, with_g2)
    assert (name == "rlc") == (plonk.vk_blob_info(blob)["num_challenges"] > 0)
    # amdzk_circuit .. permutation commitments: byte for byte the pk file's
    end = vk_blob.offsets(plonk, c.desc, with_g2)["g"]
    assert blob[12:end] == pkfile[12:end] and blob[:8] == b"AMDZKVK\0" and pkfile[:8] == b"AMDZKPK\0"
    assert plonk.blob_desc(blob) == plonk.blob_desc(pkfile)
    assert len(blob) == end + 64 + 1 + (256 if with_g2 else 0) + 64
    assert check(pkg, blob) == (0, "")


@pytest.mark.parametrize("with_g2", [False, True])
def test_every_flipped_bit_position_and_every_truncation_is_refused(pkg, plonk, oracle, with_g2):
    """Exhaustive on the k = 4 file (about 1 KB): one flipped bit at EVERY byte position (the bit walks with the position),
    EVERY length 0 .. len - 1, and one byte too many. The library is called directly so that the loop stays quick."""
    c, opk, blob, _ = make(plonk, oracle, "square", with_g2)
    assert len(blob) < 16384
    L = pkg.lib()
    info = lambda buf, n: L.amdzk_vk_blob_info(buf, n, None, None, None, None, None, None)
    assert info(blob, len(blob)) == 0
    for i in range(len(blob)):
        m = bytearray(blob)
        m[i] ^= 1 << (i % 8)
        assert info(bytes(m), len(m)) == -2, "flipped bit at byte %d accepted" % i
    for n in range(len(blob)):
        assert info(blob[:n], n) == -2, "truncation to %d bytes accepted" % n
    assert info(blob + b"\0", len(blob) + 1) == -2
    assert info(None, 0) == -2 and info(None, len(blob)) == -2
    for data, why in ((b"x" + blob[1:], "vk_read: bad magic"), (blob[:-1], "vk_read: length mismatch"), (blob[:40], "vk_read: .*too few"),
                      (blob[:100] + bytes([blob[100] ^ 4]) + blob[101:], "vk_read: digest mismatch"), (None, "vk_read: null data"),
                      (blob[:8] + struct.pack("<I", 2) + blob[12:], "vk_read: format version 2"), (b"AMDZKPK\0" + blob[8:], "vk_read: bad magic")):
        with pytest.raises(pkg.AmdzkError, match=why) as e:
            plonk.vk_blob_info(data)
        assert e.value.code == -2
    msg = C.create_string_buffer(b"?" * 63, 64)
    assert L.amdzk_vk_blob_check(blob, len(blob) - 1, msg, 12) == -2 and msg.value == b"vk_read: le" and msg.raw[12:16] == b"????"
    assert L.amdzk_vk_blob_check(blob, len(blob) - 1, None, 0) == -2


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_mutations_behind_a_valid_digest_are_refused_and_named(pkg, plonk, oracle, name, with_g2):
    """Every count field at 2^31 (the process's peak memory does not move by anything near 2^31 elements), points off their
    curve, coordinates that are no residues, identities where none may stand, a has-g2 byte of 2: refused with -2, and
    amdzk_vk_blob_check says which."""
    c, opk, blob, _ = make(plonk, oracle, name, with_g2)
    ms = mutants(plonk, c, blob, with_g2)
    counts = [m for m in ms if m[0].startswith("count_")]
    assert len(counts) >= 12 and ("count_num_challenges" in [m[0] for m in ms]) == (name == "rlc") and len(ms) - len(counts) == (12 if with_g2 else 7)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for mname, data, why in counts:
        rc, msg = check(pkg, data)
        assert rc == -2 and msg.startswith("vk_read: ") and re.search(why, msg), (mname, msg)
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    assert after - before < 64 * 1024, "peak RSS grew by %d KiB" % (after - before)  # 2^31 of anything is >= 2 GiB
    for mname, data, why in ms:
        rc, msg = check(pkg, data)
        assert rc == -2 and msg.startswith("vk_read: ") and re.search(why, msg), (mname, msg)
        with pytest.raises(pkg.AmdzkError, match=why):
            plonk.vk_blob_info(data)


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_an_identity_fixed_commitment_is_accepted(pkg, plonk, oracle, name, with_g2):
    """An all-zero fixed column commits to the identity, (0, 0): legal in a key, so legal in its file."""
    c, opk, blob, _ = make(plonk, oracle, name, with_g2)
    data = identity_commitment_file(plonk, c, blob, with_g2)
    assert data != blob and check(pkg, data) == (0, "") and plonk.vk_blob_info(data) == vk_blob.shape(c.desc, with_g2)


def test_header_inconsistencies_pk_read_refuses_are_refused_here(pkg, plonk, oracle):
    """The header checks of test_pk_blob.py on the VK file, whose circuit section goes through the same reader and validate:
    cs_degree < 3, too few rows, an expression count that does not add up, a bad has-phases byte, k out of range."""
    c, opk, blob, _ = make(plonk, oracle, "lookup", True)
    off = pk_blob.count_offsets(plonk, c.desc)
    hp = off["num_perm_columns"] + 4 + 8 * len(c.desc["permutation_columns"])  # the has-phases byte
    assert blob[hp] == 0
    for at, value, fmt, why in ((32, 2, "<I", "cs_degree 2 < 3"), (28, (1 << 5) - 2, "<I", "not enough rows"),
                                (off["num_gates"], len(c.desc["gates"]) + 1, "<I", "expression count mismatch"), (8, 2, "<I", "format version 2"),
                                (hp, 2, "<B", "has-phases byte is 2"), (12, 29, "<I", "k = 29 out of range"), (12, 0, "<I", "k = 0 out of range")):
        body = bytearray(blob[:-64])
        struct.pack_into(fmt, body, at, value)
        rc, msg = check(pkg, vk_blob.seal(body))
        assert rc == -2 and msg.startswith("vk_read: ") and why in msg and "pk_read" not in msg, (at, value, msg)


def test_refusals_in_a_standalone_program_under_asan_and_ubsan(plonk, oracle, tmp_path):
    """tests/native/vk_blob_check.cpp includes only the host-only header: every flipped bit and every truncation on
    exact-size heap copies — an out-of-bounds read of the parser is a sanitizer report — and the named mutations above, from
    files written here."""
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "vk_blob_check")
    subprocess.check_call(["g++", *SAN, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "vk_blob_check.cpp")])

    def write(fname, data):
        path = str(tmp_path / fname)
        with open(path, "wb") as f:
            f.write(data)
        return path

    for name, with_g2 in [(name, with_g2) for name in NAMES for with_g2 in (False, True)]:
        c, opk, blob, _ = make(plonk, oracle, name, with_g2)
        tag = "%s_%d" % (name, with_g2)
        ms = mutants(plonk, c, blob, with_g2)
        args = [write(tag + ".vk", blob)]
        for mname, data, why in ms:
            args += [write("%s_%s.vk" % (tag, mname), data), why]
        runs = [(args, len(blob), len(ms)), ([write(tag + "_identity.vk", identity_commitment_file(plonk, c, blob, with_g2))], len(blob), 0)]
        for argv, size, named in runs:
            p = subprocess.run([exe, *argv], text=True, capture_output=True, env=ENV, timeout=600)
            assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
            assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
            assert "vk_blob_check ok" in p.stdout and "FAILED" not in p.stdout
            assert "flips %d refused" % size in p.stdout and "truncations %d refused" % size in p.stdout and "named %d refused" % named in p.stdout
            s = vk_blob.shape(c.desc, with_g2)
            assert "parsed k %d fixed %d advice %d perm %d challenges %d g2 %d" % (s["k"], s["num_fixed"], s["num_advice"], s["num_perm_columns"],
                                                                                  s["num_challenges"], with_g2) in p.stdout
