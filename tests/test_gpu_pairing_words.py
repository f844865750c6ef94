"""GPU: the pairing's Fq2 layer, executor and programs (csrc/fq12.cuh, csrc/pairing.hpp) word by word on the device.

tests/test_gpu_pairing.py reaches this code only through whole pairings on generic points; on the CPU the products are C,
not the asm blocks of fp29_asm.inc. Here the device build of tests/native/fq12_check.hip — the library's compile flags, a
kernel of pairing_miller_kernel's shape (a lane's slab at slab + t * regs in global memory, K and the lines in global
memory, one call of pairing_exec, no arithmetic of its own) — runs every case of tests/fq12_model.py: all 13 ops as single
words with coefficients at 0, p, p + 1, 2p - 1, one hot limb, the boundaries of f29_reduce_weak's quotient estimate, the
c3(8) edge of fqx_9a_pm_b, every aliasing of d, a and b and register 255; every emitter of pairing.hpp out of place and
with the destination aliasing each operand; the three whole programs. Every case runs in two lanes of different
wavefronts with lanes of other cases (other ops of the switch) beside it. The words that come back must equal

  * reference B, the limb-exact model, wherever B ran (every single word, every short emitter, a handful of the long
    programs),
  * the host build of the same source (plain g++, the fp29 bounds as hard failures) for every case,

and reference A (integers mod p, pairing_ref's f12_* for emitters and programs) must accept them; registers nobody asked
the program to write (operands, a guard register on each side) come back as the harness prefilled them. Bit-exact, no
tolerance, no case left out. One child process on the device for the whole file (and one of the host build, which opens no
GPU); if it fails, times out or is not on a gfx950 device, every test here fails and nothing is started again.

5882 cases x 2 replicas in 36 launches; on an MI355X the launches take 0.23 s, the child process 0.5 s and the whole file
about 6 s, most of it building the cases (reference B, 4 s) and reference A's Fq12 powers."""
import os
import shutil
import subprocess
import time

import pytest

import fq12_model as M

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EXE = os.path.join(M.NATIVE, "fq12_check")
TAGS = M.OP_NAMES + sorted(M.EMITTER_NAMES.values())
N_CASES, N_LAUNCHES = 5882, 36


def fresh_binary():
    """The device build, rebuilt when it is missing or older than what it is made from. No binary and no compiler is a
    failure: a skip here would put back the gap this file closes."""
    deps = M.DEPS + [os.path.join(M.CSRC, "Makefile")]
    if not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in deps):
        assert os.path.exists(HIPCC), "tests/native/fq12_check is missing or stale and there is no hipcc to build it"
        subprocess.run(["make", "-C", M.NATIVE, "fq12_check"], check=True, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return EXE


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(cases, device results[replica][case], host results, the device harness' report line)."""
    cases = M.build_cases()
    t0 = time.time()
    dev, report, _ = M.run_harness(fresh_binary(), cases, str(tmp_path_factory.mktemp("fq12dev")), timeout=300)
    report += " (child process %.2f s)" % (time.time() - t0)
    host, _, _ = M.run_harness(M.host_binary(), cases, str(tmp_path_factory.mktemp("fq12host")))
    return cases, dev, host, report


@pytest.mark.gpu
def test_harness_ran_every_case_on_gfx950(runs):
    cases, dev, host, report = runs
    print(report)
    assert "gfx950" in report and ("%d cases x %d replicas in %d launches" % (N_CASES, M.REPLICAS, N_LAUNCHES)) in report
    assert len(cases) == N_CASES and {c.tag for c in cases} == set(TAGS) and {c.kind for c in cases} == set(range(18))
    assert {w >> 24 for c in cases if c.kind == M.E_RAW for w in c.prog} == set(range(13))


def _hex(ws):
    return " ".join("%x" % x for x in ws)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_device_equals_the_model_and_the_host_build(runs, tag):
    cases, dev, host, _ = runs
    mine = [(i, c) for i, c in enumerate(cases) if c.tag == tag]
    assert mine
    for i, c in mine:
        for rep in range(M.REPLICAS):
            got = dev[rep][i]
            where = "%s, replica %d" % (c.describe(), rep)
            if c.expect is not None:
                assert got == c.expect, "device differs from reference B: %s\n  device %s\n  model  %s" % (where, _hex(got), _hex(c.expect))
            assert got == host[rep][i], "device differs from the host build: %s\n  device %s\n  host   %s" % (where, _hex(got), _hex(host[rep][i]))
            try:
                c.judge(got)
            except AssertionError as e:
                raise AssertionError("reference A rejects the device's result: %s: %s\n  device %s" % (where, e, _hex(got)))
