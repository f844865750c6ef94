"""CPU: the header-only builder of witness programs (include/amdzk_halo2.hpp WitnessProgram, CompiledWitness) compiles with
-Wall -Werror and produces, for one program that uses every method, the amdzk_witness_desc bytes of the Python builder
(tests/native/witness_mirror_check.cpp) — and the same plan."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("wmc") / "witness_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "witness_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def python_twin(W):
    w = W(6, 4)
    x, y = w.input(), w.input()
    c7, cm1, c7b = w.const(7), w.const(R - 1), w.const(7)
    s = w.add(x, y)
    d = w.sub(s, c7)
    m = w.mul(d, cm1)
    n = w.neg(m)
    i = w.inv(n)
    z, e, lt = w.is_zero(i), w.eq(c7, c7b), w.lt(x, y)
    sel = w.select(lt, s, d)
    b, a = w.bits(sel, 31, 2), w.and_(x, cm1)
    xo = w.xor(a, b)
    w.assign(s, 0, 0), w.assign(xo, 3, 63), w.assign(z, 1, 17)
    w.expose(e), w.expose(xo)
    return w


def test_cpp_builder_gives_the_python_builder_s_bytes(exe, pkg):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    hexbytes, plan = out.stdout.split("\n")[:2]
    w = python_twin(pkg.witness.WitnessProgram)
    assert bytes.fromhex(hexbytes) == w.desc_bytes()
    pl = w.plan(3)
    assert [int(v) for v in plan.split()] == [pl["levels"], pl["launches"], pl["fused_width"], pl["scratch_bytes"], C.sizeof(pkg.ffi.WitnessDesc)]
