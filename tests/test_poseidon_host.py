"""CPU: the host half of Poseidon (csrc/poseidon.hpp) in a stand-alone program (tests/native/poseidon_check.cpp, plain g++):
pos::permute and pos::sponge — the semantics stated over the 8 x 32-bit field — and the eight-lane host loop over the 29-bit
lane step the kernels run, built with FP29_CHECK_BOUNDS so that a bound that does not hold aborts, all against
tests/poseidon_ref.py on the operand set of the GPU tests. amdzk_poseidon_check_desc (pure host code of the library) on
every refusal. Two cases once more in a build with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import poseidon_cases as PC
import poseidon_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "poseidon_check.cpp")
R = PR.R
TS = (2, 3, 5, 6, 7, 8)
ROUNDS = ((2, 0), (2, 1), (8, 57))
_exe = {}


def rates(t):
    return sorted({1, t // 2, t - 1})


def lengths(rate):
    return sorted({0, 1, rate - 1, rate, rate + 1, 2 * rate, 37})


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("poseidon_check") / ("poseidon_check_san" if sanitized else "poseidon_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def check(exe, spec, states, sponges, tmp_path, env=None):
    """Both routes of the program against the reference, word for word."""
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<8I", spec.t, spec.rate, spec.r_f, spec.r_p, int(spec.init is not None), len(states), len(sponges), 0))
        f.write(PC.to_words([v for row in spec.rc for v in row]).tobytes())
        f.write(PC.to_words([v for row in spec.mds for v in row]).tobytes())
        if spec.init is not None:
            f.write(PC.to_words(spec.init).tobytes())
        for s in states:
            f.write(PC.to_words(s).tobytes())
        for data in sponges:
            f.write(struct.pack("<2I", len(data), 0) + PC.to_words(data).tobytes())
    p = subprocess.run([exe, path], text=True, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[-2] == "ok" and len(lines) == 2 * (len(states) + len(sponges)) + 2
    rows = [PC.from_words(np.array([int(w, 16) for w in ln.split()], dtype=np.uint64)) for ln in lines[:-2]]
    for b, s in enumerate(states):
        want = PR.permute(spec, s)
        assert rows[2 * b] == want, "pos::permute, state %d" % b
        assert rows[2 * b + 1] == want, "the lane loop, state %d" % b
    for b, data in enumerate(sponges):
        want = [PR.sponge(spec, data)]
        assert rows[2 * (len(states) + b)] == want, "pos::sponge, sponge %d (len %d)" % (b, len(data))
        assert rows[2 * (len(states) + b) + 1] == want, "the lane loop, sponge %d (len %d)" % (b, len(data))
    return p


@pytest.mark.parametrize("t", TS)
def test_permutation_on_every_constant_kind(t, tmp_path, tmp_path_factory):
    exe = build(tmp_path_factory, False)
    for r_f, r_p in ROUNDS:
        for kind in PC.KINDS:
            check(exe, PC.spec(t, 1, r_f, r_p, kind), PC.states(t, 8), [], tmp_path)


@pytest.mark.parametrize("t", TS)
def test_sponge_rates_lengths_and_initial_states(t, tmp_path, tmp_path_factory):
    exe = build(tmp_path_factory, False)
    for rate in rates(t):
        for kind, init in (("random", False), ("max", True), ("cauchy", True)):
            check(exe, PC.spec(t, rate, 2, 1, kind, init), [], [PC.inputs(n, "host", edge=True) for n in lengths(rate)], tmp_path)


def test_the_reference_shape(tmp_path, tmp_path_factory):
    """t = 5, rate = 4, (8, 57), 950 inputs below 256: what the reference's nullifier hashes."""
    spec = PC.spec(5, 4, 8, 57, "cauchy")
    data = [[v % 256 for v in PC.inputs(950, "bytes%d" % b)] for b in range(2)]
    check(build(tmp_path_factory, False), spec, [], data, tmp_path)


@pytest.mark.parametrize("case", ["permute", "sponge"])
def test_host_half_is_clean_under_asan_and_ubsan(tmp_path, tmp_path_factory, case):
    from test_sanitizers import ENV
    exe = build(tmp_path_factory, True)
    if case == "permute":
        p = check(exe, PC.spec(8, 7, 8, 5, "max"), PC.states(8, 6), [], tmp_path, env=ENV)
    else:
        p = check(exe, PC.spec(7, 3, 2, 1, "random", init=True), [], [PC.inputs(n, "san", edge=True) for n in (0, 2, 3, 37)], tmp_path, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]


# ---- amdzk_poseidon_check_desc: every refusal of the description, without a device
@pytest.mark.parametrize("name,kw,code,needle", PC.DESC_REFUSALS, ids=[r[0] for r in PC.DESC_REFUSALS])
def test_check_desc_refuses(pkg, name, kw, code, needle):
    d, keep = PC.raw_desc(pkg, **kw)
    with pytest.raises(pkg.AmdzkError) as e:
        pkg.poseidon.check_desc(d)
    assert e.value.code == code and "poseidon: " in str(e.value) and needle in str(e.value), str(e.value)
    del keep


def test_check_desc_null_and_accepts(pkg):
    with pytest.raises(pkg.AmdzkError) as e:
        pkg.poseidon.check_desc(None)
    assert e.value.code == -2 and "poseidon: null description" in str(e.value)
    for kw in (dict(), dict(init=True), dict(t=8, rate=7, r_f=8, r_p=57), dict(t=2, rate=1, r_f=2, r_p=0), dict(t=3, r_p=510)):
        d, keep = PC.raw_desc(pkg, **kw)
        pkg.poseidon.check_desc(d)
        del keep
    # a NULL msg and a short one are both fine
    d, keep = PC.raw_desc(pkg, t=9)
    assert pkg.lib().amdzk_poseidon_check_desc(C.byref(d), None, 0) == -2
    msg = C.create_string_buffer(12)
    assert pkg.lib().amdzk_poseidon_check_desc(C.byref(d), msg, len(msg)) == -2 and msg.value == b"poseidon: t"
    PC.pkg_spec(pkg, PC.spec(5, 4, 8, 57)).check()
