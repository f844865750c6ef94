"""CPU: the host half of witness programs (csrc/witness.hpp) in a stand-alone program (tests/native/witness_check.cpp, plain
g++): whole programs through wit::build and wit::eval_node — the one function the kernels call per node — with every node of
every proof compared with tests/witness_ref.py. Random programs over all ops on the edge operands, and the op edges. Two
cases once more in a build with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import witness_cases as WC
import witness_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "witness_check.cpp")
_exe = {}


@pytest.fixture(scope="module")
def W(pkg):
    return pkg.witness.WitnessProgram


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("witness_check") / ("witness_check_san" if sanitized else "witness_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def run(exe, prog, inputs, tmp_path, env=None):
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(inputs)) + prog.desc_bytes())
        for row in inputs:
            f.write(WR.to_words(row).tobytes())
    p = subprocess.run([exe, path], text=True, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[-2] == "ok" and lines[0] == "levels %d" % len(WR.level_widths(prog.nodes))
    words = np.array([[int(w, 16) for w in ln.split()] for ln in lines[1:-2]], dtype=np.uint64).reshape(len(inputs), len(prog.nodes), 4)
    return [WR.from_words(words[b]) for b in range(len(inputs))], p


def check(exe, prog, inputs, tmp_path, env=None):
    got, p = run(exe, prog, inputs, tmp_path, env)
    for b, row in enumerate(inputs):
        want = WR.evaluate(prog, row)
        for i, (g, w) in enumerate(zip(got[b], want)):
            assert g == w, "proof %d node %d %s%r: got %x, want %x" % (b, i, WR.OP_NAMES[prog.nodes[i][0]], prog.nodes[i][1:], g, w)
    return p


@pytest.mark.parametrize("seed", range(6))
def test_random_programs_over_all_ops_node_by_node(W, tmp_path, tmp_path_factory, seed):
    rng = random.Random(7000 + seed)
    prog = WC.random_program(W, rng, n_nodes=600, n_inputs=8, near=(0.9, 0.5, 0.2)[seed % 3], recent=0.2)
    assert {n[0] for n in prog.nodes} == set(range(14)), "every op occurs"
    check(build(tmp_path_factory, False), prog, WC.random_inputs(rng, 12, 8), tmp_path)


def test_op_edges(W, tmp_path, tmp_path_factory):
    prog, pairs = WC.edge_program(W)
    check(build(tmp_path_factory, False), prog, pairs, tmp_path)
    # two of the edges by name, read off the reference (which the check above has just compared every node with)
    v = WR.evaluate(prog, (5, 7))
    first_xor = [i for i, n in enumerate(prog.nodes) if n[0] == WR.XOR][0]
    assert v[first_xor] == 0, "(r - 1) ^ 1 = r -> 0"
    assert v[[i for i, n in enumerate(prog.nodes) if n[0] == WR.SUB][0]] == WC.R - 1, "0 - 1"


def test_bits_every_lo_of_a_full_width_value(W, tmp_path, tmp_path_factory):
    """lo = 0..255 with the longest len, and len = 1..256 at lo = 0: every shift and every mask."""
    prog = W(3, 1)
    a = prog.input()
    for lo in range(256):
        prog.bits(a, lo, 256 - lo)
        prog.bits(a, lo, 1)
    for ln in range(1, 257):
        prog.bits(a, 0, ln)
    check(build(tmp_path_factory, False), prog, [[WC.R - 1], [WC.R - 2], [0x2AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA], [1]], tmp_path)


@pytest.mark.parametrize("case", ["random", "edges"])
def test_host_half_is_clean_under_asan_and_ubsan(W, tmp_path, tmp_path_factory, case):
    from test_sanitizers import ENV
    if case == "random":
        rng = random.Random(99)
        prog = WC.random_program(W, rng, n_nodes=300, n_inputs=5)
        inputs = WC.random_inputs(rng, 4, 5)
    else:
        prog, inputs = WC.edge_program(W)
        inputs = inputs[:20]
    prog.assign(len(prog.nodes) - 1, 1, 3)
    prog.expose(0)
    p = check(build(tmp_path_factory, True), prog, inputs, tmp_path, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
