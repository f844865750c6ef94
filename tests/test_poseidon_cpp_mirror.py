"""Poseidon of the C++ mirror (include/amdzk_halo2.hpp) driven from C++ (tests/native/poseidon_mirror_check.cpp): the
header-only class gives the ctypes route's digests and states, which are the reference's."""
import os
import struct
import subprocess

import numpy as np
import pytest

import poseidon_cases as PC
import poseidon_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pmc") / "poseidon_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "poseidon_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of Poseidon builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


@pytest.mark.gpu
def test_cpp_poseidon_gives_the_ctypes_routes_words(exe, pkg, ctx, tmp_path):
    spec = PC.spec(5, 4, 8, 57, "cauchy", init=True)
    states = PC.states(5, 9)
    sponges = [PC.inputs(n, "mirror", edge=True) for n in (37, 0, 4, 9)]
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<8I", spec.t, spec.rate, spec.r_f, spec.r_p, 1, len(states), len(sponges), 0))
        for block in ([v for row in spec.rc for v in row], [v for row in spec.mds for v in row], spec.init, [v for s in states for v in s]):
            f.write(PC.to_words(block).tobytes())
        for data in sponges:
            f.write(struct.pack("<2I", len(data), 0) + PC.to_words(data).tobytes())
    p = subprocess.run([exe, path], text=True, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout.splitlines()[0] == "check ok" and p.stdout.splitlines()[-1] == "ok", (p.stdout[-2000:], p.stderr[-2000:])

    def rows(tag):
        return np.array([[int(w, 16) for w in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split()[0] == tag], dtype=np.uint64)

    P = pkg.poseidon.Poseidon(ctx, PC.pkg_spec(pkg, spec))
    try:
        py_digests = P.hash_many([PC.to_words(d) for d in sponges])
        py_states = P.permute_many(np.stack([PC.to_words(s) for s in states]))
    finally:
        P.free()
    assert np.array_equal(rows("digest"), py_digests) and np.array_equal(rows("dev"), py_digests)
    assert np.array_equal(rows("squeeze"), py_digests[:1])
    assert np.array_equal(rows("state").reshape(len(states), 5, 4), py_states)
    assert PC.from_words(py_digests) == [PR.sponge(spec, d) for d in sponges]
    assert [PC.from_words(s) for s in py_states] == [PR.permute(spec, s) for s in states]
