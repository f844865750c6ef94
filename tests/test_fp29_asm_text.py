"""CPU: the four generated asm products of csrc/fp29_asm.inc (F29_MUL_ASM_FQ/FR, F29_SQR_ASM_FQ/FR) exist only in the
device compile, so no host build ever executes them. This file runs their TEXT: a small emulator of the instruction forms
the blocks use executes the committed lines on every operand class of tests/fp29_model.py that the products' contract
admits and compares limb for limb with the model's restatement of the C code (reference B) and, as residues with the
documented bound, with integer arithmetic (reference A). A carry out of any v_mad_u64_u32 — the hardware would put it into
vcc and drop it — is a failure for every in-contract operand. The register contract between the text and the asm
statements of fp29.cuh (clobbers, early-clobber outputs, operand numbering) is checked statically, and single-line
mutants of every block show that the operand set can fail.

The same model drives tests/test_gpu_field_ops.py, which runs the compiled functions on the device."""
import os
import re
import subprocess
import sys

import pytest

import fp29_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anon-aadhaar-halo2_amd", "csrc")
INC = open(os.path.join(CSRC, "fp29_asm.inc")).read()
HDR = open(os.path.join(CSRC, "fp29.cuh")).read()
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def blocks(text=INC):
    out = {}
    for m in re.finditer(r"#define (F29_\w+) \\\n((?:  \".*\n)+)", text):
        out[m.group(1)] = re.findall(r'"([^"\\]+)\\n\\t"', m.group(2))
    return out


BLOCKS = blocks()
BLOCK_NAMES = ["F29_MUL_ASM_FQ", "F29_SQR_ASM_FQ", "F29_MUL_ASM_FR", "F29_SQR_ASM_FR"]


def field_of(name):
    return M.FIELDS[name[-2:]]


def kind_of(name):
    return name.split("_")[1]  # MUL / SQR


# ------------------------------------------------------------------------------------------ the emulator
class EmuError(Exception):
    """The text does something the emulator does not accept: an instruction it does not know, a register that was never
    written, an operand form that does not exist."""


_PARSED = {}


def _operand(x):
    x = x.strip()
    if re.fullmatch(r"0x[0-9a-f]+", x):
        return ("imm", int(x, 16))
    if re.fullmatch(r"\d+", x):
        return ("imm", int(x))
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", x)
    if m:
        if int(m.group(2)) != int(m.group(1)) + 1 or int(m.group(1)) % 2:
            raise EmuError("not an even-aligned register pair: " + x)
        return ("pair", "v" + m.group(1), "v" + m.group(2))
    if re.fullmatch(r"%\d+|v\d+|s\d+|vcc", x):
        return ("reg", x)
    raise EmuError("unknown operand: " + x)


def parse_line(ln):
    if ln not in _PARSED:
        op, _, rest = ln.partition(" ")
        _PARSED[ln] = (op, [_operand(t) for t in re.split(r",\s*(?![^\[]*\])", rest)])
    return _PARSED[ln]


def run(lines, inputs):
    """Executes the block. `inputs`: {'%9': value, ...}. Returns (registers, number of carries out of v_mad_u64_u32,
    largest 64-bit multiply-add result)."""
    reg = dict(inputs)
    carries = peak = 0

    def rd(o, bits=32):
        if o[0] == "imm":
            return o[1]
        try:
            if o[0] == "pair":
                if bits != 64:
                    raise EmuError("64-bit pair where a 32-bit operand is expected")
                return reg[o[1]] | (reg[o[2]] << 32)
            if bits == 64:
                raise EmuError("32-bit register where a 64-bit operand is expected")
            return reg[o[1]]
        except KeyError as e:
            raise EmuError("read of a register nobody wrote: %s" % e)

    def wr(o, v, bits=32):
        if o[0] == "pair" and bits == 64:
            reg[o[1]], reg[o[2]] = v & M32, (v >> 32) & M32
        elif o[0] == "reg" and bits == 32 and o[1] != "vcc":
            reg[o[1]] = v & M32
        else:
            raise EmuError("bad destination")

    for ln in lines:
        op, a = parse_line(ln)
        if op == "s_mov_b32" and len(a) == 2 and a[0][0] == "reg" and a[0][1][0] == "s":
            wr(a[0], rd(a[1]))
        elif op == "v_mov_b32" and len(a) == 2:
            wr(a[0], rd(a[1]))
        elif op == "v_and_b32" and len(a) == 3:
            wr(a[0], rd(a[1]) & rd(a[2]))
        elif op == "v_lshlrev_b32" and len(a) == 3:
            wr(a[0], rd(a[2]) << (rd(a[1]) & 31))
        elif op == "v_lshrrev_b64" and len(a) == 3:
            wr(a[0], rd(a[2], 64) >> (rd(a[1]) & 63), 64)
        elif op == "v_mad_u64_u32" and len(a) == 5 and a[1] == ("reg", "vcc"):
            addend = rd(a[4], 64) if a[4][0] == "pair" else rd(a[4])
            v = rd(a[2]) * rd(a[3]) + addend  # the full 65-bit result
            if v > M64:
                carries += 1
            peak = max(peak, v)
            wr(a[0], v & M64, 64)
        else:
            raise EmuError("instruction the emulator does not know: " + ln)
    return reg, carries, peak


def run_product(name, lines, a, b=None):
    """The block on limb vectors as f29_mul_asm / f29_sqr_asm bind them: mul %9.. = a, %18.. = b; sqr %18.. = a."""
    if kind_of(name) == "MUL":
        ins = {"%%%d" % (9 + i): a[i] for i in range(9)}
        ins.update({"%%%d" % (18 + i): b[i] for i in range(9)})
    else:
        ins = {"%%%d" % (18 + i): a[i] for i in range(9)}
    reg, carries, peak = run(lines, ins)
    try:
        return [reg["%%%d" % i] for i in range(9)], carries, peak
    except KeyError as e:
        raise EmuError("output never written: %s" % e)


# ------------------------------------------------------------------------------------------ operands
def operands(name):
    """Every (what, a, b) of the shared case list that belongs to this block (context (i) cases of f29_mul / f29_sqr)."""
    F, func = field_of(name), (M.F_MUL if kind_of(name) == "MUL" else M.F_SQR)
    out = []
    for c in CASES:
        if c.func == func and c.F is F:
            out.append((c.what, c.data[:9], c.data[9:18] if func == M.F_MUL else None, c))
    assert len(out) > 50
    return out


CASES = M.build_cases()


def first_failure(name, lines, ops):
    """None if the block computes what it should on every operand, else a short reason."""
    for what, a, b, case in ops:
        try:
            r, carries, _ = run_product(name, lines, a, b)
        except EmuError as e:
            return "emulator: %s" % e
        if carries:
            return "carry out of a multiply-add at [%s]" % what
        if r != case.expect:
            return "limbs differ from reference B at [%s]" % what
        try:
            case.check(r)
        except AssertionError as e:
            return "reference A at [%s]: %s" % (what, e)
    return None


# ------------------------------------------------------------------------------------------ tests
def test_asm_inc_is_what_the_generator_prints():
    gen = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "gen_fp29_asm.py")], text=True)
    assert gen == INC, "csrc/fp29_asm.inc is not the output of tools/gen_fp29_asm.py: regenerate it, do not edit it"


def _header_const(struct, name):
    blk = HDR[HDR.index("struct %s {" % struct):]
    blk = blk[:blk.index("};")]
    m = re.search(r"uint32_t %s\(int i\) \{ return (.*?); \}" % name, blk)
    v = [int(x, 16) for x in re.findall(r"\? (0x[0-9a-f]+)u", m.group(1))] + [int(re.search(r": (0x[0-9a-f]+)u$", m.group(1)).group(1), 16)]
    assert len(v) == 9
    return v


@pytest.mark.parametrize("F", [M.FQ, M.FR], ids=repr)
def test_header_constants_equal_the_model(F):
    """The model derives its constants from the two integers; the header's copies (and the 8 x 32-bit moduli of bn254.cuh)
    must be the same numbers."""
    for name, want in (("p", F.P), ("one", F.one), ("k_in", F.k_in), ("k_out", F.k_out)):
        assert _header_const(F.struct, name) == want, name
    for K in (3, 5, 6, 7, 8, 10):
        assert _header_const(F.struct, "c%d" % K) == F.c(K)
    blk = HDR[HDR.index("struct %s {" % F.struct):]
    assert int(re.search(r"pinv = (0x[0-9a-f]+)u", blk).group(1), 16) == F.pinv
    assert int(re.search(r"recip42 = (\d+)u", blk).group(1)) == F.recip42
    bn = open(os.path.join(CSRC, "bn254.cuh")).read()
    blk = bn[bn.index("struct %s {" % F.packed_struct):]
    assert [int(x, 16) for x in re.findall(r"0x[0-9a-f]{8}", blk[:blk.index("r1(int")])] == M.words(F.p)
    assert int(re.search(r"inv = (0x[0-9a-f]+)u", blk).group(1), 16) == (-pow(F.p, -1, 1 << 32)) % (1 << 32)
    # the s_mov lines of the blocks carry the same digits
    for kind in ("MUL", "SQR"):
        lines = BLOCKS["F29_%s_ASM_%s" % (kind, F.tag)]
        assert lines[:10] == ["s_mov_b32 s%d, 0x%08x" % (90 + i, v) for i, v in enumerate(F.P + [F.pinv])]


def test_reference_b_agrees_with_reference_a_on_every_case():
    """B-vs-A for every function and class the device suite uses: B's output has the right residue, the documented bound and
    is normalised where the header says so (each case's `check`); building the cases already ran every precondition
    assertion of B and every accumulator-width check."""
    assert len(CASES) > 2000
    for c in CASES:
        try:
            c.check(c.expect)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c.describe(), e))
    funcs = {c.func for c in CASES}
    assert funcs == set(M.FUNC_NAMES), "a harness function without cases: %s" % (set(M.FUNC_NAMES) - funcs)


def test_point_formula_cases_reach_the_top_of_the_accumulator_bounds_and_every_quad_branch():
    """What the case list promises about the point formulas, counted: every formula that takes an accumulator sees one with
    x, y, zz, zzz in the last p below 9p, 5p, 2p, 2p; x29_add_quad sees each branch with canonical, lifted and mixed
    operands; the quad chain feeds its own outputs (y not canonical: the unreduced sum of two products) back in. (That B stays inside its own preconditions on all of them is what
    building the list asserts; that A accepts B's output is the test above.)"""
    def top(words):
        c = [M.val(words[9 * i:9 * i + 9]) for i in range(4)]
        return all((b - 1) * M.Q <= v < b * M.Q for v, b in zip(c, M.ACC_BOUNDS))
    for func in (M.F_ADD_AFFINE, M.F_DBL, M.F_ADD, M.F_DBL_QUAD, M.F_ADD_QUAD):
        assert sum(top(c.data[:36]) for c in CASES if c.func == func) >= 6, M.FUNC_NAMES[func]
    for func in (M.F_ADD, M.F_ADD_QUAD):
        mine = [c for c in CASES if c.func == func and c.aux == 0]
        both = [c for c in mine if top(c.data[:36]) and top(c.data[36:72])]
        mixed = [c for c in mine if top(c.data[:36]) != top(c.data[36:72]) and any(c.data[18:27]) and any(c.data[54:63])]
        for group in (both, mixed):
            results = {"identity" if not any(c.expect[18:27]) else "point" for c in group}
            assert results == {"identity", "point"} and len(group) >= 18, M.FUNC_NAMES[func]
    quads = [c for c in CASES if c.func == M.F_ADD_QUAD]
    assert {c.kind for c in quads} == {"generic", "doubling", "cancellation", "identity", "sits out"}
    fed_back = [c for c in CASES if c.func == M.F_QUAD_CHAIN and c.expect]
    assert len(fed_back) == 4 and any(M.val(c.expect[36 * i + 9:36 * i + 18]) >= M.Q for c in fed_back for i in range(3))
    with pytest.raises(M.ContractError):  # one p more in x is outside x29_add_quad's contract, and B says so: 10p * 2p... s2 - s1
        S = M.x29_lift(M.x29_add_affine(M.x29_from_affine(M.G1), *M.affine_to_r261(M.affine_mul(5, M.G1)), False))
        far = (M.digits(M.val(S[0]) + 160 * M.Q),) + S[1:]
        M.x29_add_quad(far, M.x29_lift(M.x29_dbl(S)))


@pytest.mark.parametrize("F", [M.FQ, M.FR], ids=repr)
def test_reference_b_refuses_operands_one_step_outside_the_contract(F):
    """Classes 3-5 once more with the top limb one higher: a*b (a*b + c*d) reaches 169 p^2 and B's own precondition says so."""
    outs = M.class_bound_pairs(F, M.MASK)[1] + M.class_bound_pairs(F, (1 << 30) - 1)[1] + M.class_lazy_mul(F)[1]
    assert len(outs) >= 8
    for a, b in outs:
        with pytest.raises(M.ContractError):
            M.f29_mul(F, a, b)
    with pytest.raises(M.ContractError):
        M.f29_sqr(F, M.class_sqr_bound(F)[1])
    with pytest.raises(M.ContractError):
        M.f29_mul2(F, *M.class_lazy_mul2(F)[1])
    with pytest.raises(M.ContractError):  # limbs: both operands above 2^30
        M.f29_mul(F, [1 << 30] * 8 + [0], [1 << 30] * 8 + [0])
    with pytest.raises(M.ContractError):  # a seventh term without a carry is what f29_wide_madd's comment forbids
        M.f29_wide_madd(F, M.f29_wide_zero(), [1 << 29] + [0] * 8, [0] * 9)
    w = M.f29_wide_zero()
    with pytest.raises(M.OverflowError_):  # the model's width check can fire: 8 * 9 * 2^58 does not fit a column
        for _ in range(8):
            M.f29_wide_madd(F, w, [M.MASK] * 9, [M.MASK] * 9)


@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_block_equals_both_references_without_a_carry_out(name):
    assert first_failure(name, BLOCKS[name], operands(name)) is None


def _stated(pattern):
    m = re.search(pattern, HDR, re.S)
    assert m, "fp29.cuh no longer states this headroom figure: " + pattern
    return m.group(1)


def _below_pow2(v, exp_tenths):
    """v < 2^(exp_tenths / 10), in integers."""
    return v ** 10 < 1 << exp_tenths


@pytest.mark.parametrize("F", [M.FQ, M.FR], ids=repr)
def test_accumulator_peaks_stay_below_the_figures_the_header_states(F):
    """The worst column of each documented operand regime against the figure in fp29.cuh's comments (read from the header,
    so that a changed comment has to be re-justified here). Operands: limbs 0..7 at the top of the regime's range on one
    side, 2^29 - 1 on the other, values at the a*b < 169 p^2 bound."""
    lazy = _stated(r"f29_mul /\s*// the asm product then holds <= 9 \* 2\^60 \+ 9 \* 2\^58 < 2\^(\d+\.\d)")
    mul2 = _stated(r"f29_mul2 with its other three operands\s*// normalised <= 9 \* 2\^60 \+ 18 \* 2\^58 < 2\^(\d+\.\d)")
    lazy2 = _stated(r"<= 9 \* 2\.5 \* 2\^59 \+ 9 \* 2\^58 \+ a carry < 2\^(\d+\.\d)")
    assert (lazy, mul2, lazy2) == ("63.5", "63.8", "63.8")
    name = "F29_MUL_ASM_" + F.tag
    peaks = {}
    for lim, key in ((0x7FFFFFFF, "lazy"), (0x9FFFFFFF, "lazy2")):
        peaks[key] = 0
        for va in (2 * F.p, 12 * F.p, 16 * F.p - 1):
            a = M._top_for([lim] * 8, va)
            b = M._fill_b(F, a, [M.MASK] * 8)[0]
            for x, y in ((a, b), (b, a)):
                F.max_acc = 0
                want = M.f29_mul(F, x, y)
                r, carries, peak = run_product(name, BLOCKS[name], x, y)
                assert r == want and carries == 0
                assert peak == F.max_acc, "the asm text and the C code do not reach the same column sums"
                peaks[key] = max(peaks[key], peak)
    assert _below_pow2(peaks["lazy"], 635), "f29_sub10_lazy operand: 2^%.3f" % M._log2(peaks["lazy"])
    assert _below_pow2(peaks["lazy2"], 638), "f29_sub10_lazy2 operand: 2^%.3f" % M._log2(peaks["lazy2"])
    assert peaks["lazy2"] > peaks["lazy"] > 1 << 63, "the operands above do not come near the limit they are meant to test"
    F.max_acc = 0
    M.f29_mul2(F, *M.class_lazy_mul2(F)[0])
    assert 1 << 63 < F.max_acc and _below_pow2(F.max_acc, 638), "f29_mul2: 2^%.3f" % M._log2(F.max_acc)
    F.max_acc = 0
    M.wide_sum(F, [([M.MASK] * 9, [M.MASK] * 9)] * 6, 6)  # six terms between carries: 54 * 2^58 in a column
    assert 1 << 63 < F.max_acc < 1 << 64


@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_overflow_detection_can_fire(name):
    """Limbs 2^31 - 1 on both sides are outside every contract: nine products of 2^62 do not fit, and the emulator says so.
    (CPU only: out-of-contract operands never go to the device.)"""
    a = [(1 << 31) - 1] * 8 + [1]
    _, carries, peak = run_product(name, BLOCKS[name], a, a)
    assert carries > 0 and peak > M64


def test_an_unknown_instruction_is_a_failure():
    lines = list(BLOCKS["F29_MUL_ASM_FQ"])
    lines[40] = lines[40].replace("v_mad_u64_u32", "v_mad_co_u64_u32")
    with pytest.raises(EmuError):
        run_product("F29_MUL_ASM_FQ", lines, M.FQ.one, M.FQ.one)
    assert {parse_line(ln)[0] for name in BLOCK_NAMES for ln in BLOCKS[name]} == \
        {"s_mov_b32", "v_mov_b32", "v_and_b32", "v_lshlrev_b32", "v_lshrrev_b64", "v_mad_u64_u32"}


# ---- the register contract between the text and fp29.cuh's asm statements
def _macro(name):
    m = re.search(r"#define %s(?:\(\w+\))? (.*)" % name, HDR)
    assert m, name
    return m.group(1)


def _asm_statements():
    """{block macro: (outputs, inputs) as lists of (constraint, struct variable, limb)} from f29_mul_asm / f29_sqr_asm."""
    out = {}
    for m in re.finditer(r"asm\((F29_\w+) : ([^:]*) : ([^:]*) : F29_ASM_CLOBBERS\);", HDR):
        def expand(part):
            ops = []
            for mac, var in re.findall(r"(F29_ASM_OUT9|F29_ASM_IN9)\((\w+)\)", part):
                par = re.search(r"#define %s\((\w+)\)" % mac, HDR).group(1)
                for cons, v, limb in re.findall(r'"([^"]+)"\((\w+)\.l\[(\d)\]\)', _macro(mac)):
                    assert v == par
                    ops.append((cons, var, int(limb)))
            return ops
        out[m.group(1)] = (expand(m.group(2)), expand(m.group(3)))
    return out


def test_every_literal_register_is_in_the_clobber_list():
    clobbers = set(re.findall(r'"(\w+)"', _macro("F29_ASM_CLOBBERS")))
    for name in BLOCK_NAMES:
        used = set()
        for ln in BLOCKS[name]:
            for lo, hi in re.findall(r"\bv\[(\d+):(\d+)\]", ln):
                used |= {"v%d" % i for i in range(int(lo), int(hi) + 1)}
            used |= set(re.findall(r"\b(?:v\d+|s\d+|vcc)\b", ln))
        assert used, name
        assert used <= clobbers, "%s names %s without clobbering it" % (name, sorted(used - clobbers))
        assert used == clobbers, "F29_ASM_CLOBBERS lists registers no block touches: %s" % sorted(clobbers - used)


def test_operand_numbering_and_early_clobbers():
    """mul: %0-8 r, %9-17 a, %18-26 b; sqr: %0-8 r, %9-17 d (doubled limbs, scratch outputs), %18-26 a — what
    tools/gen_fp29_asm.py documents is what f29_mul_asm / f29_sqr_asm pass; and every %N the text writes while an input is
    still to be read is an early-clobber output (otherwise hipcc may give it an input's register)."""
    stm = _asm_statements()
    assert set(stm) == set(BLOCK_NAMES)
    gen_doc = open(os.path.join(ROOT, "tools", "gen_fp29_asm.py")).read()
    assert "mul: %9..%17 = a, %18..%26 = b" in gen_doc and "%9..%17 = d (2a), a = %18..%26" in gen_doc
    for name, (outs, ins) in stm.items():
        nine = lambda var: [(var, i) for i in range(9)]
        got = [(v, i) for _, v, i in outs + ins]
        if kind_of(name) == "MUL":
            assert got == nine("r") + nine("a") + nine("b"), name
        else:
            assert got == nine("r") + nine("d") + nine("a"), name
        n_out = len(outs)
        assert all(c == "v" for c, _, _ in ins) and all(c in ("=&v", "=v") for c, _, _ in outs)
        lines = BLOCKS[name]
        inputs = {"%%%d" % i for i in range(n_out, n_out + len(ins))}
        reads = [set(o[1] for o in parse_line(ln)[1][1:] if o[0] == "reg") for ln in lines]
        writes = [parse_line(ln)[1][0] for ln in lines]
        last_input_read = max(i for i, r in enumerate(reads) if r & inputs)
        for i, w in enumerate(writes):
            if w[0] == "reg" and w[1].startswith("%"):
                n = int(w[1][1:])
                assert n < n_out, "%s writes the input operand %s" % (name, w[1])
                if i < last_input_read:
                    assert outs[n][0] == "=&v", "%s writes %s at line %d, before the last read of an input (line %d), but it is not early-clobber" % (name, w[1], i, last_input_read)
        assert {int(x[1:]) for ln in lines for x in re.findall(r"%\d+", ln)} <= set(range(n_out + len(ins)))


# ---- the operand set can fail: single-line mutants
def mutants(lines):
    for i, ln in enumerate(lines):
        rest = lines[:i], lines[i + 1:]
        yield ("delete", i, rest[0] + rest[1])
        for m in re.finditer(r"%(\d+)", ln):
            for d in (-1, 1):
                if int(m.group(1)) + d >= 0:
                    yield ("index %+d" % d, i, rest[0] + [ln[:m.start()] + "%%%d" % (int(m.group(1)) + d) + ln[m.end():]] + rest[1])
        for m in re.finditer(r"\bs(9\d)\b", ln):
            for d in (-1, 1):
                yield ("sreg %+d" % d, i, rest[0] + [ln[:m.start()] + "s%d" % (int(m.group(1)) + d) + ln[m.end():]] + rest[1])
        if "0x1fffffff" in ln:
            for alt in ("0x3fffffff", "0x0fffffff"):
                yield ("mask " + alt, i, rest[0] + [ln.replace("0x1fffffff", alt)] + rest[1])
        if ", 29," in ln:
            for alt in ("28", "30"):
                yield ("shift " + alt, i, rest[0] + [ln.replace(", 29,", ", %s," % alt)] + rest[1])


def allowed_survivor(name, kind, line):
    """The two kinds of single-line change that leave every in-contract result unchanged:
    (a) a 30-bit mask on the Montgomery factor m_0 .. m_7: m_k + 2^29 is another multiplier that clears column k (p is odd
        and only the low 29 bits of the column must vanish); the extra 2^29 * p is absorbed by the next columns' own
        factors and the result limbs are identical. For m_8 there is no later factor: that mutant changes the result.
    (b) in the square, the doubling of limb 0, `v_lshlrev_b32 %9, 1, %18`: d_0 is never read (a_0 pairs with d_k, k > 0,
        and with itself), so deleting the line or re-indexing its destination or source changes nothing that is used."""
    m = re.fullmatch(r"v_and_b32 %([0-7]), 0x1fffffff, v4", line)
    if m and kind == "mask 0x3fffffff":
        return "a"
    if kind_of(name) == "SQR" and line == "v_lshlrev_b32 %9, 1, %18" and (kind == "delete" or kind.startswith("index")):
        return "b"
    return None


@pytest.mark.parametrize("name", BLOCK_NAMES)
def test_single_line_mutants_are_rejected(name):
    lines, ops = BLOCKS[name], operands(name)
    # a handful of operands kills almost everything; only what survives them meets the whole set
    quick = [o for o in ops if o[0] in ("random", "limbs 2^30-1 at the 169 p^2 bound", "largest normalised operand")][:6]
    assert first_failure(name, lines, ops) is None
    total, survivors = 0, []
    for kind, i, mut in mutants(lines):
        total += 1
        if first_failure(name, mut, quick) is None and first_failure(name, mut, ops) is None:
            survivors.append((kind, i, lines[i]))
    assert total > 800
    unexplained = [s for s in survivors if allowed_survivor(name, s[0], s[2]) is None]
    assert not unexplained, "mutants the operand set does not notice: %s" % unexplained
    kinds = {allowed_survivor(name, s[0], s[2]) for s in survivors}
    assert kinds <= ({"a"} if kind_of(name) == "MUL" else {"a", "b"})
    # the m_8 variant of (a) is not equivalent and must be among the killed
    assert not any(s[2].startswith("v_and_b32 %8, 0x1fffffff, v4") for s in survivors)
