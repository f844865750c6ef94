"""GPU: ProverSHPLONK / ProverGWC of the C++ mirror (include/amdzk_halo2.hpp) driven from C++
(tests/native/multiopen_mirror_check.cpp): three polynomials at two points, each scheme; the printed points are the
oracle's for a transcript with the same counter challenges."""
import os
import subprocess
import sys

import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
TAU = 0x1234567890ABCDEF1234567


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("momc") / "multiopen_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "multiopen_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


class CountingTranscript:
    """The driver's transcript: challenges 1000, 1001, ..; points are only recorded."""

    def __init__(self):
        self.points, self.squeezes = [], 0

    def squeeze_challenge(self):
        self.squeezes += 1
        return 999 + self.squeezes

    def write_point(self, p):
        self.points.append(p)


@pytest.mark.gpu
def test_cpp_provers_write_the_oracles_points(exe):
    import plonk_ref as PR

    k = 5
    n = 1 << k
    polys = [[1 + 7 * i + 13 * j + i * j for j in range(n)] for i in range(3)]
    queries = [(polys[0], 3), (polys[1], 3), (polys[0], 5), (polys[2], 5), (polys[1], 3)]
    out = subprocess.check_output([exe, str(k), "%x" % TAU], text=True, timeout=120)

    def points(tag):
        rows = [ln.split()[1:] for ln in out.splitlines() if ln.split()[0] == tag]
        return [(zu.from_limbs([int(w, 16) for w in r[:4]]) * pow(zu.MONT, -1, zu.Q) % zu.Q,
                 zu.from_limbs([int(w, 16) for w in r[4:]]) * pow(zu.MONT, -1, zu.Q) % zu.Q) for r in rows]
    for scheme, prove, squeezes in (("shplonk", PR.shplonk_prove, 3), ("gwc", PR.gwc_prove, 1)):
        T = CountingTranscript()
        prove(queries, T, TAU, n, lambda *a: None)
        assert len(T.points) == 2 and T.squeezes == squeezes  # h(X) and the quotient; W_3 and W_5
        for tag in (scheme, scheme + "_evals"):
            assert points(tag + "_returned") == T.points, tag
            assert points(tag + "_written") == T.points, tag
            assert "%s_calls %d 0" % (tag, squeezes) in out
        assert "%s_throwing: write_point failed" % scheme in out
