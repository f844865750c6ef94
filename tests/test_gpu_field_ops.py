"""GPU: csrc/fp29.cuh and the device-only branches of csrc/bn254.cuh, function by function, on the device.

The asm products (fp29_asm.inc), the 8 x 32-bit CIOS `mul` and the Fermat `inv` are compiled only for the device, and the
rest of the suite reaches them only through whole MSMs, NTTs and proofs on random or witness-like data. Here
tests/native/fp29_device_check.hip — the two headers, the library's compile flags, nothing else — runs every case of
tests/fp29_model.py (operands at the documented bounds, one hot limb, chosen Montgomery factors, lazy limbs, chains, the
point formulas with all their branches) in two lanes (quads) of different wavefronts, and the words that come back must equal the
model's limb-exact restatement of the C code (reference B); then integer arithmetic (reference A) judges them as residues
with the documented bound. Bit-exact, no tolerance. One child process for the whole file; if it fails, times out or is not
on a gfx950 device, every test here fails and nothing is started again.

Also here, without a GPU: the disassembly of the harness shows that its one-product kernels contain exactly the
multiply-adds of one asm block between the inline-asm markers (the harness tests the asm path, not the C fallback) and
that no harness kernel uses scratch memory.

The quad-lane formulas of csrc/fp29_quad.cuh (x29_dbl_quad, x29_add_quad, and the two chained as msm_window_combine_kernel
chains them) take one quad of lanes per case: the four lanes' results must be word-equal and equal to reference B, with quads
of other branches, and quads that sit out, beside them in the wavefront. Every point formula, lane-serial or quad, also gets
its operands at the top of the documented accumulator bounds (x below 9p, y below 5p, zz and zzz below 2p).

3598 cases x 2 replicas in 47 launches; the whole file takes under 2 s on an MI355X, most of it the child process' start-up."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import fp29_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anon-aadhaar-halo2_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
SRC, EXE = os.path.join(NATIVE, "fp29_device_check.hip"), os.path.join(NATIVE, "fp29_device_check")
DEPS = [SRC, os.path.join(CSRC, "fp29.cuh"), os.path.join(CSRC, "fp29_quad.cuh"), os.path.join(CSRC, "fp29_asm.inc"), os.path.join(CSRC, "bn254.cuh")]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MAGIC = 0x43393246
REPLICAS = 2
# which compile context of the asm block a function exercises (the module docstring of the harness)
CONTEXT = {M.F_MUL: "(i) one product per thread", M.F_SQR: "(i) one product per thread", M.F_MUL_CHAIN: "(ii) dependent chain",
           M.F_SQR_CHAIN: "(ii) dependent chain", M.F_MUL2_CHAIN: "(ii) dependent chain", M.F_DBL_AFFINE: "(iii) point formula",
           M.F_ADD_AFFINE: "(iii) point formula", M.F_DBL: "(iii) point formula", M.F_ADD: "(iii) point formula", M.F_ADD_CHAIN: "(iii) point formula",
           M.F_DBL_QUAD: "(iv) quad formula", M.F_ADD_QUAD: "(iv) quad formula", M.F_QUAD_CHAIN: "(iv) quad formula"}


def library_flags():
    """CXXFLAGS of csrc/Makefile with ARCH substituted: what libamdzk.so's kernels are compiled with."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", mk, re.M).group(1)
    return re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", arch).split()


def fresh_binary():
    """The harness, rebuilt when it is missing or older than what it is made from. No binary and no compiler is a failure:
    a skip here would put back the gap this file closes."""
    stale = not os.path.exists(EXE) or any(os.path.getmtime(d) > os.path.getmtime(EXE) for d in DEPS)
    if stale:
        assert os.path.exists(HIPCC), "tests/native/fp29_device_check is missing or stale and there is no hipcc to build it"
        subprocess.run(["make", "-C", NATIVE, "fp29_device_check"], check=True, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return EXE


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<4I", MAGIC, len(cases), M.IN_WORDS, M.OUT_WORDS))
        for c in cases:
            f.write(struct.pack("<4I", c.func, 0 if c.F is M.FQ else 1, c.aux, len(c.data)))
            f.write(struct.pack("<%dI" % M.IN_WORDS, *(c.data + [0] * (M.IN_WORDS - len(c.data)))))


def read_results(path, n):
    raw = open(path, "rb").read()
    assert struct.unpack_from("<4I", raw) == (MAGIC, n, REPLICAS, M.OUT_WORDS) and len(raw) == 16 + 4 * REPLICAS * n * M.OUT_WORDS
    w = struct.unpack_from("<%dI" % (REPLICAS * n * M.OUT_WORDS), raw, 16)
    return [[w[(r * n + i) * M.OUT_WORDS:(r * n + i + 1) * M.OUT_WORDS] for i in range(n)] for r in range(REPLICAS)]


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    """(cases, results[replica][case], the harness' report line). Cases are grouped by (function, field): one launch each."""
    cases = sorted(M.build_cases(), key=lambda c: (c.func, c.F.tag))
    d = tmp_path_factory.mktemp("fp29dev")
    inp, outp = str(d / "cases.bin"), str(d / "results.bin")
    write_cases(inp, cases)
    p = subprocess.run([fresh_binary(), inp, outp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, "fp29_device_check exit %d (2 HIP error, 3 not gfx950, 4 case file): %s" % (p.returncode, p.stdout[-2000:])
    return cases, read_results(outp, len(cases)), p.stdout.strip()


@pytest.mark.gpu
def test_harness_ran_every_case_on_gfx950(device_run):
    cases, res, report = device_run
    print(report)
    assert "gfx950" in report and ("%d cases x %d replicas" % (len(cases), REPLICAS)) in report
    assert len(cases) > 2000 and {c.func for c in cases} == set(M.FUNC_NAMES)


def _hex(ws):
    return " ".join("%08x" % x for x in ws)


@pytest.mark.gpu
@pytest.mark.parametrize("func", sorted(M.FUNC_NAMES), ids=lambda f: M.FUNC_NAMES[f])
def test_device_equals_the_model(device_run, func):
    cases, res, _ = device_run
    mine = [(i, c) for i, c in enumerate(cases) if c.func == func]
    assert mine
    for i, c in mine:
        for rep in range(REPLICAS):
            got = list(res[rep][i][:len(c.expect)])
            where = "%s, context %s, replica %d" % (c.describe(), CONTEXT.get(func, "surrounding C code"), rep)
            assert got == c.expect, "device differs from reference B: %s\n  device %s\n  model  %s" % (where, _hex(got), _hex(c.expect))
            try:
                c.check(got)
            except AssertionError as e:
                raise AssertionError("reference A rejects the device's result: %s: %s\n  device %s" % (where, e, _hex(got)))
            assert all(x == 0xFFFFFFFF for x in res[rep][i][len(c.expect):]), "the harness wrote past the result of " + where


# ------------------------------------------------------------------------------------------ CPU: what the harness is made of
def _kernel_bodies(asm):
    return {m.group(1): m.group(2) for m in re.finditer(r"^(_Z10run_kernel\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_harness_runs_the_asm_blocks_and_uses_no_scratch(tmp_path):
    from test_miscompile_guard import kernel_meta

    flags = library_flags()
    assert "-O3" in flags and "-DAMDZK_ASM_PRODUCT" in flags and "--offload-arch=gfx950" in flags
    out = str(tmp_path / "fp29_device_check.s")
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", SRC, "-o", out], check=True, timeout=900, cwd=str(tmp_path),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = {k: v for k, v in kernel_meta(asm).items() if "run_kernel" in k}
    assert len(meta) == 47, "one kernel per (function, field) of the harness table"
    for name, (priv, spills) in meta.items():
        assert (priv, spills) == (0, 0), "harness kernel %s uses scratch memory (%d bytes, %d spills)" % (name, priv, spills)
    bodies = _kernel_bodies(asm)
    for op, mads in (("5OpMulI", 171), ("5OpSqrI", 135)):
        mine = [b for k, b in bodies.items() if op in k]
        assert len(mine) == 2, op  # Fq and Fr
        for b in mine:
            blocks = re.findall(r";;#ASMSTART\n(.*?);;#ASMEND", b, re.S)
            assert len(blocks) == 1, "context (i) holds exactly one asm block"
            assert len(re.findall(r"\bv_mad_u64_u32\b", blocks[0])) == mads
            # outside the block only the address arithmetic of the record (a few 64-bit index products); the C fallback would add 162
            assert len(re.findall(r"\bv_mad_u64_u32\b", b)) - mads < 8, "multiply-adds outside the block: the C fallback was compiled in"
    # the generated text counts the same (its own comment lines), so the harness, the text test and the generator agree
    inc = open(os.path.join(CSRC, "fp29_asm.inc")).read()
    assert re.findall(r"// \w+ (mul|sqr): (\d+) v_mad_u64_u32", inc) == [("mul", "171"), ("sqr", "135")] * 2
