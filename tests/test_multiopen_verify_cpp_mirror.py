"""VerifierSHPLONK / VerifierGWC of the C++ mirror (include/amdzk_halo2.hpp) driven from C++ behind the mirror's provers
(tests/native/multiopen_verify_mirror_check.cpp): three polynomials at two points, counter challenges. The printed guard is
tests/opening_verify_ref.py's pair for the oracle's points and the same challenges; the honest opening is decided valid, a
wrong evaluation and a wrong commitment are not; a throwing transcript is rethrown."""
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
    out = str(tmp_path_factory.mktemp("mvmc") / "multiopen_verify_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "multiopen_verify_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of VerifierSHPLONK and VerifierGWC builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


class CountingTranscript:
    """The driver's transcripts: challenges 1000, 1001, ..; points are only recorded."""

    def __init__(self):
        self.points, self.squeezes = [], 0

    def squeeze_challenge(self):
        self.squeezes += 1
        return 999 + self.squeezes

    def write_point(self, p):
        self.points.append(p)


@pytest.mark.gpu
def test_cpp_verifiers_give_the_reference_pair_and_verdicts(exe):
    import opening_verify_ref as OV
    import plonk_ref as PR
    import pyref as P

    k = 5
    n = 1 << k
    polys = [[1 + 7 * i + 13 * j + i * j for j in range(n)] for i in range(3)]
    which, at = [0, 1, 0, 2, 1], [3, 3, 5, 5, 3]
    out = subprocess.check_output([exe, str(k), "%x" % TAU], text=True, timeout=120)

    def points(tag):
        rows = [[int(w, 16) for w in ln.split()[1:]] for ln in out.splitlines() if ln.split()[0] == tag]
        pts = []
        for r in rows:
            for i in range(0, len(r), 8):
                x, y = zu.fq_to_int(r[i:i + 4]), zu.fq_to_int(r[i + 4:i + 8])
                pts.append(None if x == 0 and y == 0 else (x, y))
        return pts
    coms = [PR.commit_tau(p, TAU) for p in polys]
    assert points("commitment") == coms
    evals = [P.eval_polynomial(polys[p], z) for p, z in zip(which, at)]
    queries = list(zip(which, [0, 0, 1, 1, 0]))
    for scheme, prove, squeezes in (("shplonk", PR.shplonk_prove, 3), ("gwc", PR.gwc_prove, 2)):
        T = CountingTranscript()
        prove([(polys[p], z) for p, z in zip(which, at)], T, TAU, n, lambda *a: None)
        assert points(scheme + "_point") == T.points and len(T.points) == 2
        ch = (1000, 1001, 1002) if scheme == "shplonk" else (1000, 1001)
        ref = OV.pair(scheme, coms, [3, 5], queries, evals, ch, T.points)
        assert OV.holds(ref, TAU)
        assert tuple(points(scheme + "_guard")) == ref
        assert "%s_calls 2 %d 0" % (scheme, squeezes) in out
        assert "%s_verdict 1 0 0" % scheme in out
        assert "%s_throwing: read_point failed" % scheme in out
