"""The challenge-phase part of the C++ mirror (include/amdzk_halo2.hpp), driven by tests/native/halo2_phases_check.cpp.

CPU: a phased circuit configured in C++ flattens to the arrays and the phase table the Python mirror produces (word 9
CHALLENGE, degree 0 of a challenge, the per-column and per-challenge phases), and advice_column_in /
challenge_usable_after refuse what upstream's assertions refuse.
GPU: keygen + create_proof with a synthesize functor, entirely from C++, give the phased-order harness's bytes; a
TranscriptWrite object receives every transcript call; an exception thrown by the functor comes back out of create_proof."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import phased_circuits as PC  # noqa: E402
import phased_oracle as PO  # noqa: E402
from test_cpp_mirror import python_description, write_witness  # noqa: E402

TAU = 0x1234567890ABCDEF1234567


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("hpc")
    out = str(d / "halo2_phases_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "halo2_phases_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


@pytest.fixture(scope="module")
def plonk():
    import __graft_entry__ as g
    return g.load_package().plonk


@pytest.mark.parametrize("name", ["rlc", "rlc3"])
def test_cpp_phased_constraint_system_flattens_like_python(exe, plonk, name):
    c = PC.rlc_circuit(plonk, 6, three_phases=name == "rlc3")
    ph, keep = plonk.flatten_phases(c.desc)
    want = python_description(plonk, c.cs, c.k)
    want += "phased 1 %d\n" % ph.num_challenges
    want += "advice_phase " + " ".join(str(int(v)) for v in keep[0]) + "\n"
    want += "challenge_phase " + " ".join(str(int(v)) for v in keep[1]) + "\n"
    assert " 150994944" in want  # 9 << 24: the CHALLENGE word of challenge 0
    assert subprocess.check_output([exe, "describe", name, str(c.k)], text=True) == want


def test_cpp_mirror_validates_phases_like_upstream(exe):
    out = subprocess.check_output([exe, "errors"], text=True).splitlines()
    assert out == ["advice_column_in(1) first: -2 advice_column_in: no advice column in phase 0, the one before phase 1",
                   "challenge_usable_after(0) first: -2 challenge_usable_after: no advice column in phase 0",
                   "advice_column_in(2) without phase 1: -2 advice_column_in: no advice column in phase 1, the one before phase 2",
                   "advice_column_in(3): -2 advice_column_in: phase 3 (phases are 0, 1, 2)",
                   "challenge_usable_after(1) without phase 1: -2 challenge_usable_after: no advice column in phase 1",
                   "challenge_usable_after(0): accepted", "advice_column_in(1): accepted", "degree of a challenge 0", "phased 1"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rlc", "rlc3"])
def test_cpp_driven_phased_proof_equals_the_harness(exe, plonk, name, tmp_path, monkeypatch):
    import plonk_ref as PR

    c = PC.rlc_circuit(plonk, 6, seed=5, three_phases=name == "rlc3")
    wit = str(tmp_path / "witness.txt")
    write_witness(c, wit)
    out = subprocess.check_output([exe, "prove", name, str(c.k), wit, "17", "%x" % TAU, "%x" % 0xC0FFEE], text=True)
    lines = out.splitlines()
    proof = bytes.fromhex([ln for ln in lines if ln.startswith("proof ")][0].split()[1])
    calls = [[int(v, 16) for v in ln.split()[1:]] for ln in lines if ln.startswith("callback")]
    nch = len(c.desc["challenge_phase"])
    assert len(calls) == nch and all(len(x) == nch for x in calls)  # one callback per later phase, every challenge slot present
    ch = [calls[-1][0]] if nch == 1 else [calls[1][0], calls[1][1]]
    assert calls[0] == [ch[0]] + [0] * (nch - 1)  # the challenges of unfinished phases are zero
    opk = PR.keygen(PO.specialise(c.desc, [0] * nch), c.fixed, c.assembly.mapping, TAU, transcript_repr=0xC0FFEE)
    adv = [list(col) for col in c.advice]
    for phase in range(1, nch + 1):
        c.fill(phase, dict(enumerate(ch)), adv)
    assert proof == PO.create_proof(monkeypatch, opk, c.desc, [c.instances], [adv], 17, ch)
    assert PO.verify_proof(monkeypatch, opk, c.desc, [c.instances], proof, ch)
    # the TranscriptWrite object: no bytes on the library's side, every call forwarded; its counter challenges reach the functor
    obj = [ln for ln in lines if ln.startswith("object ")][0].split()
    assert int(obj[1]) == 0 and int(obj[2]) > 0 and int(obj[3]) > 0 and int(obj[4]) >= nch + 6
    ocalls = [[int(v, 16) for v in ln.split()[1:]] for ln in lines if ln.startswith("object_callback")]
    assert ocalls[0][0] == 1000 and (nch == 1 or ocalls[1][:2] == [1000, 1001])
    assert "throwing: synthesize failed" in lines
    assert bytes.fromhex([ln for ln in lines if ln.startswith("again ")][0].split()[1]) == proof
