"""The verifying key through the C++ mirror (include/amdzk_halo2.hpp) driven from C++ (tests/native/vk_mirror_check.cpp):
keygen_vk without a proving key, a proof from a ProvingKey made separately and freed with its params, write and read of the
key file, decide_proof. The file is the independent encoder's (tests/vk_blob.py) from the oracle's key, the proof is the
oracle prover's, and both verdicts are the oracle's."""
import os
import subprocess
import sys

import pytest

import circuits
import pairing_ref as PRF
import vk_blob
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
TAU, REPR = 0x1234567890ABCDEF1234567, 0xC0FFEE


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vkmc") / "vk_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "vk_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of VerifyingKey, keygen_vk, get_vk and the VerifyingKey overloads of verify_proof /
    decide_proof builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


@pytest.mark.gpu
def test_cpp_keygen_vk_write_read_and_decide(exe, pkg):
    import plonk_ref as PR
    import verify_ref as VR

    plonk = pkg.plonk
    c = circuits.square_circuit(plonk, 4, signal=5)
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    want_proof = PR.create_proof(opk, c.instances, c.advice, seed=17)
    kinds = VR.element_kinds(c.desc, 1)
    at = 32 * kinds.index("s")  # Blake2b: 32 bytes per element, the first evaluation
    lines = dict(ln.split(" ", 1) for ln in subprocess.check_output([exe, "%x" % TAU, "%x" % REPR, str(at)], text=True, timeout=300).splitlines())
    proof = bytes.fromhex(lines["proof"])
    assert proof == want_proof
    g2, s_g2 = PRF.G2_GEN, PRF.g2_mul(PRF.G2_GEN, TAU)
    assert bytes.fromhex(lines["vkfile"]) == vk_blob.encode(plonk, c.desc, opk.fixed_commitments, opk.permutation_commitments, REPR, PRF.G1_GEN, g2, s_g2)
    assert lines["same_file"] == "1" and lines["guard"] == "1"
    # the oracle's verdicts on the proof and on the copy the program mutated
    mutated = bytearray(proof)
    mutated[at] = (mutated[at] + 1) % 256
    mutated = bytes(mutated)
    assert VR.decode(c.desc, 1, [c.instances], proof) == (0, 0) and VR.holds(VR.pair(opk, [c.instances], proof), TAU)
    assert VR.decode(c.desc, 1, [c.instances], mutated) == (0, 0) and not VR.holds(VR.pair(opk, [c.instances], mutated), TAU)
    assert (lines["decide"], lines["mutated"]) == ("1", "0")
