"""CPU: the pairing unit in a stand-alone program (tests/native/pairing_host_check.cpp, plain g++): the host half
(csrc/pairing.hpp) and the ZK_HD device half (csrc/fq12.cuh) exactly as the kernels run it, with the fp29 bounds compiled in
as hard failures (FP29_CHECK_BOUNDS), against tests/pairing_ref.py: s * G2 and GT limb for limb. Once more in a build with
ASan + UBSan (a stand-alone program: nothing here is loaded into Python)."""
import os
import subprocess

import pytest

import pairing_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pairing_host_check.cpp")
_exe = {}

S_RANDOM = 0x2B1C0D9E8F7A6B5C4D3E2F1A0B9C8D7E6F5A4B3C2D1E0F9A8B7C6D5E4F3A2B1
SETUP_SCALARS = [1, 2, X.R - 1, S_RANDOM % X.R]
A1, B1, A2, B2 = 0x9E3779B97F4A7C15F39CC0605CEDC834, 0x1082276BF3A27251F86C6A11D0C18E95, 0x2545F4914F6CDD1D, X.R - 5
# (G1 scalar or None for the identity, G2 scalar) per pair
PRODUCTS = [[(1, 1)], [(A1, B1)], [(A2, B2)], [(A1, 1), (None, B1), (A2, B2)]]


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("pairing_host_check") / ("pairing_check_san" if sanitized else "pairing_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def points(prod):
    return [(None if a is None else X.g1_mul(X.G1_GEN, a), X.g2_mul(X.G2_GEN, b)) for a, b in prod]


def script(setups, products):
    h = lambda v: "%x" % v
    out = ["setup " + h(s) for s in setups]
    for prod in products:
        out.append("prod %d" % len(prod))
        for p, q in points(prod):
            p = p or (0, 0)
            out.append(" ".join(h(v) for v in (p[0], p[1], q[0][0], q[0][1], q[1][0], q[1][1])))
    return "\n".join(out) + "\n"


def run(exe, setups, products, env=None):
    p = subprocess.run([exe], input=script(setups, products), text=True, capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[0] == "selfcheck ok" and lines[-2] == "ok", lines
    body = lines[1:-2]
    g2s = [tuple(int(v, 16) for v in ln.split()[1:]) for ln in body if ln.startswith(("g2 ", "sg2 "))]
    gts = [[int(v, 16) for v in ln.split()[1:]] for ln in body if ln.startswith("gt ")]
    return g2s, gts, p


def flat(q):
    return (q[0][0], q[0][1], q[1][0], q[1][1])


def check(g2s, gts, setups, products):
    assert len(g2s) == 2 * len(setups) and len(gts) == len(products)
    for i, s in enumerate(setups):
        assert g2s[2 * i] == flat(X.G2_GEN)
        assert g2s[2 * i + 1] == flat(X.g2_mul(X.G2_GEN, s)), "s * G2 for s = %x" % s
    for got, prod in zip(gts, products):
        want = X.pairing_product(points(prod))
        assert got[:12] == X.f12_to_tower(want), prod
        assert got[12] == (1 if want == X.F12_ONE else 0)


def test_host_build_with_bounds_matches_the_reference_limb_for_limb(tmp_path_factory):
    g2s, gts, _ = run(build(tmp_path_factory, False), SETUP_SCALARS, PRODUCTS)
    check(g2s, gts, SETUP_SCALARS, PRODUCTS)


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path_factory):
    from test_sanitizers import ENV
    setups, products = [SETUP_SCALARS[2]], [PRODUCTS[0], PRODUCTS[3]]
    g2s, gts, p = run(build(tmp_path_factory, True), setups, products, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    check(g2s, gts, setups, products)
