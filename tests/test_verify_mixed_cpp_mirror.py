"""verify_proofs / decide_proofs of the C++ mirror (include/amdzk_halo2.hpp) over a list of VerifyItem — proofs of different
circuits under different keys in one call — driven from C++ (tests/native/verify_mixed_mirror_check.cpp): a proving key over a
downsized setup beside a verifying key at a larger k, the same-key batch word for word the single-key overload's, the mixed
guard the Python binding's, verdicts per proof and combined, and the refusal of a key made over another setup."""
import os
import subprocess
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import verify_cases as VC  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vmmc") / "verify_mixed_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "verify_mixed_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of the VerifyItem overloads builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


def words(guard):
    return ["%064x" % sum(int(w) << (64 * i) for i, w in enumerate(pt[j:j + 4])) for pt in (guard.lhs, guard.rhs) for j in (0, 4)]


@pytest.mark.gpu
def test_cpp_items_give_the_python_bindings_words(exe, ctx, pkg, oracle, tmp_path):
    from test_gpu_verify import Rig
    plonk = pkg.plonk
    a, b = Rig(ctx, pkg, plonk, oracle, "square", 1), Rig(ctx, pkg, plonk, oracle, "lookup", 1)
    try:
        assert a.c.k == 4 and b.c.k == 5
        args = ["%x" % VC.TAU]
        cases = []
        for tag, rig in (("a", a), ("b", b)):
            case = rig.case("blake2b", "shplonk", seed=51)
            cases.append(case)
            key, proof = str(tmp_path / (tag + ".pk")), str(tmp_path / (tag + ".proof"))
            with open(key, "wb") as f:
                f.write(rig.pk.write())
            with open(key + ".inst", "w") as f:
                for col in rig.c.instances:
                    f.write(" ".join("%x" % v for v in col) + "\n")
            with open(proof, "wb") as f:
                f.write(case.proof)
            args += [str(rig.c.k), key, proof]
        # circuit A's verifying key over a setup with another G (H = 7 G): a file, which needs no SRS to be read
        from test_gpu_verify_mixed import OtherSetup
        other = OtherSetup(ctx, pkg, plonk, oracle)
        try:
            vk = other.rig.pk.get_vk()
            with open(str(tmp_path / "foreign.vk"), "wb") as f:
                f.write(vk.write())
            vk.free()
        finally:
            other.free()
        out = subprocess.check_output([exe] + args + [str(tmp_path / "foreign.vk")], text=True, timeout=300).splitlines()
        single, same = out[0].split(), out[1].split()
        assert single[0] == "single" and same[0] == "same" and single[1:5] == ["0"] * 4 and same[1:] == single[1:]
        pa, pb = cases[0].proof, cases[1].proof
        bad = pa[:-1] + bytes([pa[-1] ^ 0x40])
        items = [plonk.VerifyItem(a.pk, a.inst, pa), plonk.VerifyItem(b.pk, b.inst, pb), plonk.VerifyItem(a.pk, a.inst, bad)]
        w = np.stack([zu.fr_from_int(v) for v in (2, 3, 5)])
        g = plonk.verify_proofs_mixed(ctx, items, combine_scalars=w)
        mixed = out[2].split()
        assert mixed[0] == "mixed" and [int(v) for v in mixed[1:7]] == [v for s in g.statuses for v in s]
        assert mixed[7:] == words(g)
        vparams = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(VC.TAU))
        try:
            verdicts, _ = plonk.decide_proofs_mixed(ctx, vparams, items)
            combined, _ = plonk.decide_proofs_mixed(ctx, vparams, items, combined=True, combine_seed=99)
        finally:
            vparams.free()
        assert verdicts[:2] == [True, True]
        assert out[3] == "decide %s %d" % (" ".join(str(int(v)) for v in verdicts), sum(verdicts))
        assert out[4] == "combined %s %d" % (" ".join(str(int(v)) for v in combined), sum(combined))
        assert out[5].startswith("refused: ") and "verify_proofs_mixed: item 1" in out[5]
        assert out[6] == "after 1 1"
    finally:
        a.free()
        b.free()
