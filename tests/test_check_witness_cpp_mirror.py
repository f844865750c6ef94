"""GPU: ProvingKey::check_witness of the C++ mirror (include/amdzk_halo2.hpp) driven from C++
(tests/native/check_witness_mirror.cpp): the lookup circuit configured in C++, a satisfying witness and a corrupted one;
the printed report is the reference's (tests/witness_check_ref.py)."""
import os
import subprocess

import pytest

import circuits
import witness_check_ref as W
from test_cpp_mirror import write_witness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0x1234567890ABCDEF1234567


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cwmc") / "check_witness_mirror")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "check_witness_mirror.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of check_witness builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


@pytest.mark.gpu
def test_cpp_report_is_the_references(exe, pkg, tmp_path):
    c = circuits.lookup_circuit(pkg.plonk, 5, seed=3)
    q_rng = c.desc["lookups"][0]["inputs"][0][1]
    row = next(r for r in range(3, c.usable) if c.fixed[q_rng[1]][r] == 1)
    cells = [(2, 0, (c.advice[2][0] + 1) % circuits.R), (0, row, 1000), (2, 1, (c.advice[2][1] + 1) % circuits.R)]
    bad = [list(a) for a in c.advice]
    for col, r, v in cells:
        bad[col][r] = v
    want = W.report(c, advice=bad)
    assert {e[0] for e in want} == {W.GATE, W.LOOKUP, W.COPY}
    wit = str(tmp_path / "witness.txt")
    write_witness(c, wit)
    with open(wit, "a") as f:
        for cell in cells:
            f.write("B %d %d %x\n" % cell)
    out = subprocess.check_output([exe, str(c.k), wit, "%x" % TAU], text=True, timeout=120)
    lines = out.splitlines()
    assert lines[0] == "good 0 1" and lines[1] == "bad %d 0" % len(want)
    assert [tuple(int(v) for v in ln.split()[1:]) for ln in lines[2:]] == want
