"""CPU: the pairing's Fq2 layer, executor and programs word by word (csrc/fq12.cuh, csrc/pairing.hpp) in the host build of
tests/native/fq12_check.hip — plain g++, the fp29 bounds compiled in as hard failures — against tests/fq12_model.py.

Reference B (the limb-exact restatement of fq12.cuh) runs every single-word case, every short emitter and a handful of
whole programs; the host build has to return B's words wherever B ran, and reference A (integers mod p; pairing_ref's
f12_* for emitters and programs) has to accept every register the host build returns — the ones B did not run included.
Once more in a build with ASan + UBSan: a stand-alone program, nothing is loaded into Python. tests/test_gpu_pairing_words.py
runs the same cases through the device build of the same source.

Also here, with hipcc present: the device build's kernel — pairing_miller_kernel's shape around the same pairing_exec — has
no private segment and no spills, as the kernels the library ships."""
import os
import shutil
import subprocess

import pytest

import fq12_model as M
import pairing_ref as X

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TAGS = M.OP_NAMES + sorted(M.EMITTER_NAMES.values())


@pytest.fixture(scope="module")
def cases():
    return M.build_cases()


@pytest.fixture(scope="module")
def host_run(cases, tmp_path_factory):
    res, report, _ = M.run_harness(M.host_binary(), cases, str(tmp_path_factory.mktemp("fq12host")))
    return res, report


def test_tower_conversion_round_trips():
    import random
    rnd = random.Random(5)
    for _ in range(4):
        f = tuple(rnd.randrange(X.P) for _ in range(12))
        assert X.f12_from_tower(X.f12_to_tower(f)) == f
    assert X.f12_from_tower([1] + [0] * 11) == X.F12_ONE
    # c1.c2 = u is u v^2 w = (w^6 - 9) w^5
    assert X.f12_from_tower([0] * 11 + [1]) == X.f12_add(X.f12_from_fq2((0, 1), 5), (0,) * 12)


def test_constant_table_of_the_model_is_the_harness_table():
    """K as pairing::device_consts builds it (host Montgomery arithmetic, then one f29_mul by k_in) against the model's
    (integers, then the limb model's f29_mul): limb for limb, and the right field elements."""
    K = M.harness_consts()
    assert K == M.device_consts()
    assert [M.res2(k) for k in K] == M.K_RES() and len(K) == M.K_COUNT


def test_class_coverage(cases):
    """What section 3 of the issue asks the builder for (the boundary sets of the weak reduction are asserted inside it)."""
    by = {}
    for c in cases:
        by.setdefault(c.tag, []).append(c)
    assert set(by) == set(TAGS) and len(cases) > 5000
    assert {c.kind for c in cases} == set(range(18)), "an emitter id is missing"
    n = len(M.coeff_classes())
    for op in ("sqr", "neg", "conj", "mulxi", "mov"):
        assert len({(tuple(c.inputs[1][0]), tuple(c.inputs[1][1])) for c in by[op] if c.regs == 6}) >= n * n
    top = M.digits(2 * M.Q - 1)
    assert any(c.inputs.get(1) == [top, top] and c.inputs.get(2) == [top, top] for c in by["mul"])
    assert {c.prog[0] & 255 for c in by["mulk"] if c.regs == 6} == set(range(M.K_COUNT)) == {c.prog[0] & 255 for c in by["movk"] if c.regs == 6}
    assert any(len(c.prog) == 3 and len({w >> 16 & 255 for w in c.prog}) == 3 for c in by["line"])
    assert any((c.prog[0] >> 16 & 255) + 2 == c.regs for c in by["line"])
    for op in M.OP_NAMES:
        fields = {(w >> 16 & 255, w >> 8 & 255, w & 255) for c in by[op] if c.regs == 256 for w in c.prog}
        assert any(d == 255 or d == 254 and op == "line" for d, _, _ in fields), op
        if op not in ("movk", "line"):
            assert any(a == 255 for _, a, _ in fields), op
        if op in ("mul", "add", "sub", "mulfq"):
            assert any(b == 255 for _, _, b in fields), op
            whats = {c.what for c in by[op]}
            assert {"aliasing, d == a", "aliasing, d == b", "aliasing, a == b", "aliasing, d == a == b"} <= whats
    # B ran every single word and every short emitter; the long programs on a handful of inputs
    long_tags = {"e12_pow_u", "miller_program", "final_exp_program"}
    assert all(c.expect is not None for c in cases if c.tag not in long_tags)
    for t in long_tags:
        assert 1 <= sum(c.expect is not None for c in by[t]) < len(by[t])
    assert {k for c in by["e12_frobenius"] for k in [c.args[3]]} == {1, 2, 3}


@pytest.mark.parametrize("tag", TAGS)
def test_reference_a_accepts_reference_b(cases, tag):
    for c in cases:
        if c.tag == tag and c.expect is not None:
            try:
                c.judge(c.expect)
            except AssertionError as e:
                raise AssertionError("reference A rejects reference B: %s: %s" % (c.describe(), e))


def _compare(cases, res, tag, who):
    mine = [(i, c) for i, c in enumerate(cases) if c.tag == tag]
    assert mine
    for i, c in mine:
        assert res[0][i] == res[1][i], "the two replicas differ: " + c.describe()
        if c.expect is not None:
            assert res[0][i] == c.expect, "%s differs from reference B: %s\n  got   %s\n  model %s" % (
                who, c.describe(), " ".join("%x" % x for x in res[0][i]), " ".join("%x" % x for x in c.expect))
        try:
            c.judge(res[0][i])
        except AssertionError as e:
            raise AssertionError("reference A rejects what %s returns: %s: %s" % (who, c.describe(), e))


@pytest.mark.parametrize("tag", TAGS)
def test_host_build_with_bounds_equals_b_and_a_accepts_it(cases, host_run, tag):
    res, report = host_run
    assert ("%d cases x %d replicas" % (len(cases), M.REPLICAS)) in report
    _compare(cases, res, tag, "the host build")


def test_host_build_is_clean_under_asan_and_ubsan(cases, host_run, tmp_path):
    from test_sanitizers import ENV, SAN
    exe = str(tmp_path / "fq12_check_san")
    subprocess.check_call(["g++", "-x", "c++", *SAN, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, M.SRC])
    res, _, p = M.run_harness(exe, cases, str(tmp_path), env=ENV, timeout=900)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    assert res == host_run[0]


def _raw(word, inputs):
    return M.Case("raw", "precondition", M.E_RAW, (), [word], 6, inputs, (), [3], lambda got, pre: None, run_b=False)


@pytest.mark.parametrize("what,word,inputs", [
    ("sqr: operand not normalised", M.pair_word(M.P_SQR, 3, 1), {1: [[1 << 29] + [0] * 8, [0] * 9]}),
    ("9a_pm_b: subtrahend too large", M.pair_word(M.P_MULXI, 3, 1), {1: [[0] * 9, [0] * 8 + [M.F.c(3)[8] + 1]]}),
    ("sub: subtrahend too large", M.pair_word(M.P_SUB, 3, 1, 2), {1: [[0] * 9, [0] * 9], 2: [[0] * 8 + [M.F.c(3)[8] + 1], [0] * 9]}),
    ("reduce_weak: value >= 2^261", M.pair_word(M.P_ADD, 3, 1, 2), {1: [[0] * 8 + [1 << 28], [0] * 9], 2: [[0] * 8 + [1 << 28], [0] * 9]}),
    ("an operand nobody set (the prefill): not normalised", M.pair_word(M.P_MUL, 3, 1, 2), {2: [[0] * 9, [0] * 9]}),
], ids=lambda v: v if isinstance(v, str) else None)
def test_a_broken_precondition_fails_on_the_cpu(tmp_path, what, word, inputs):
    """In the model while the case is built (ContractError) and in the host build (abort), before any GPU run."""
    with pytest.raises(M.ContractError):
        R = [inputs.get(r) or M.pattern_reg(r) for r in range(6)]
        M.pairing_exec([word], R, M.device_consts(), [])
    with pytest.raises(AssertionError, match="fp29 bound violated"):
        M.run_harness(M.host_binary(), [_raw(word, inputs)], str(tmp_path))


def test_a_word_that_leaves_the_slab_is_refused_before_it_runs(tmp_path):
    for word, regs in ((M.pair_word(M.P_MOV, 6, 1), 6), (M.pair_word(M.P_ADD, 1, 2, 6), 6), (M.pair_word(M.P_MULK, 1, 2, M.K_COUNT), 6),
                       (M.pair_word(M.P_LINE, 5), 6), (M.pair_word(13, 1, 1, 1), 6)):
        c = _raw(word, {})
        c.lines = [M.line_words(0)] * 4
        with pytest.raises(AssertionError, match="exit 4"):
            M.run_harness(M.host_binary(), [c], str(tmp_path))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_device_build_has_the_shipped_code_shape(tmp_path):
    """The library's flags, one kernel, no private segment and no spills: the executor the library ships, not a variant that
    keeps an Fq2 on the stack."""
    from test_gpu_field_ops import library_flags
    from test_miscompile_guard import kernel_meta

    flags = library_flags()
    assert "-O3" in flags and "-DAMDZK_ASM_PRODUCT" in flags and "--offload-arch=gfx950" in flags
    out = str(tmp_path / "fq12_check.s")
    subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", M.SRC, "-o", out], check=True, timeout=900, cwd=str(tmp_path),
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = open(out).read()
    meta = kernel_meta(asm)
    assert len(meta) == 1 and "fq12_check_kernel" in list(meta)[0]
    assert list(meta.values())[0] == (0, 0), "the harness kernel uses scratch memory: %r" % (meta,)
    assert ";;#ASMSTART" in asm, "the asm products are not in the device build: the C fallback was compiled"
