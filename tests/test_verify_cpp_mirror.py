"""verify_proof / verify_proofs of the C++ mirror (include/amdzk_halo2.hpp) driven from C++ (tests/native/
verify_mirror_check.cpp): the key from a key file, proofs made by the device prover; the printed pairs are the reference's
(tests/verify_ref.py), a malformed proof throws naming status and offset, and the batch weights are the seeded draws."""
import os
import subprocess
import sys

import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vmc") / "verify_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "verify_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of verify_proof and verify_proofs builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


def point(words):
    x, y = (zu.fq_to_int([int(w[i:i + 16], 16) for i in (48, 32, 16, 0)]) for w in words)
    return None if x == 0 and y == 0 else (x, y)


@pytest.mark.gpu
def test_cpp_guard_is_the_references(exe, ctx, pkg, oracle, tmp_path):
    from test_gpu_verify import Rig
    plonk = pkg.plonk
    rig = Rig(ctx, pkg, plonk, oracle, "lookup", 1)
    try:
        cases = [rig.case("evm", "gwc", seed=40 + b) for b in range(3)]
        key = str(tmp_path / "key.pk")
        with open(key, "wb") as f:
            f.write(rig.pk.write())
        with open(key + ".inst", "w") as f:
            for col in rig.c.instances:
                f.write(" ".join("%x" % v for v in col) + "\n")
        files = []
        blobs = [cases[0].proof, cases[1].proof[:-1], cases[2].proof]
        for b, blob in enumerate(blobs):
            files.append(str(tmp_path / ("proof%d.bin" % b)))
            with open(files[-1], "wb") as f:
                f.write(blob)
        args = [exe, str(rig.c.k), "%x" % VC.TAU, key, "1", "1"]
        lines = subprocess.check_output(args + files, text=True, timeout=120).splitlines()
        single = lines[0].split()
        assert single[:3] == ["single", "0", "0"]
        assert (point(single[3:5]), point(single[5:7])) == cases[0].pair()
        rng = PR.ChaCha20Rng(7)
        rho = [rng.fr() for _ in range(3)]
        batch = lines[1].split()
        assert batch[0] == "batch" and (point(batch[1:3]), point(batch[3:5])) == VR.combine([cases[0].pair(), cases[2].pair()], [rho[0], rho[2]])
        assert lines[2:] == ["status 0 0", "status 1 0", "status 0 0"]
        # a malformed first proof: verify_proof throws, naming status and offset
        lines = subprocess.check_output(args + [files[1], files[0]], text=True, timeout=120).splitlines()
        assert lines[0] == "single error verify_proof: malformed proof, status 1, offset 0"
    finally:
        rig.free()
