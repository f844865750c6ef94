"""Model of the pairing's Fq2 layer and executor (csrc/fq12.cuh) on top of tests/fp29_model.py, and the cases that
tests/native/fq12_check.hip runs word by word: tests/test_fq12_model.py (CPU: the host build of the harness, with the fp29
bounds compiled in) and tests/test_gpu_pairing_words.py (GPU: the device build). Plain Python integers only.

Reference B — fq12.cuh restated statement for statement on limb lists from fp29_model's f29_mul, f29_sqr, f29_mul2,
f29_add, f29_add_lazy, f29_sub / f29_neg (K = 3), f29_reduce_weak and f29_unpack: fqx_*, fq2x_* and pairing_exec itself
(all 13 ops, the word decoding, the advancing line pointer). Every F29_REQUIRE of the C code is a `require` here and
mul_admits / sqr_admits / mul2_admits stay on, so a case that breaks a stated precondition fails while the cases are built,
on the CPU. What the device has to return limb for limb.

Reference A — integers mod p. A single word is judged by Fq2 arithmetic written out below (`a_word`); emitters and programs
by tests/pairing_ref.py's f12_* (one polynomial ring, no tower), reached through f12_from_tower. A accepts a register if
every coefficient is normalised, below the bound the function's comment states (2p, or 1.0003p) and has the right
residue; the Montgomery factor 2^261 is taken out as fp29_model does (`res`).

The emitters of csrc/pairing.hpp are NOT restated: the harness prints the words they emit (`emit`), and B runs those."""
import functools
import os
import random
import subprocess
import tempfile

import fp29_model as M
import pairing_ref as X
from fp29_model import FQ, MASK, M32, Q, RADIX, ContractError, OverflowError_, digits, require, val, words  # noqa: F401

F = FQ
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
SRC = os.path.join(NATIVE, "fq12_check.hip")
CSRC = os.path.join(ROOT, "anon-aadhaar-halo2_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, n) for n in ("fq12.cuh", "pairing.hpp", "fp29.cuh", "fp29_asm.inc", "bn254.cuh")]
MAGIC = 0x43323146
REPLICAS = 2
R256 = 1 << 256
P8 = Q >> 232

(P_MUL, P_SQR, P_ADD, P_SUB, P_NEG, P_CONJ, P_MULXI, P_MOV, P_MOVK, P_MULK, P_MULFQ, P_FQINV, P_LINE) = range(13)
OP_NAMES = ["mul", "sqr", "add", "sub", "neg", "conj", "mulxi", "mov", "movk", "mulk", "mulfq", "fqinv", "line"]
K_ZERO, K_ONE, K_GAMMA, K_COUNT = 0, 1, 2, 17
(E_RAW, E6_MUL_V, E6_MUL, E6_SQR, E6_MUL_01, E6_INV, E12_CONJ, E12_MUL, E12_SQR, E12_MUL_034, E12_FROBENIUS, E4_SQR,
 E12_CYCLOTOMIC_SQR, E12_INV, E12_POW_U, MILLER_PROGRAM, MUL_PROGRAM, FINAL_EXP_PROGRAM) = range(18)
EMITTER_NAMES = {v: k.lower() for k, v in list(globals().items()) if k.startswith(("E6_", "E12_", "E4_")) or k.endswith("_PROGRAM")}
MILLER_XP, MILLER_YP, MILLER_F, FINAL_A, FINAL_B = 0, 1, 2, 0, 6


def pair_word(op, d, a=0, b=0):
    return op << 24 | d << 16 | a << 8 | b


def pattern_reg(r):
    """What a register nobody wrote holds: the harness prefills every slab with it."""
    return [[0xA5000000 | r << 8 | j for j in range(9)], [0xA5000000 | r << 8 | (9 + j) for j in range(9)]]


# ------------------------------------------------------------------------------------------ reference B
_seen_tops = {}  # op of a single-word case -> the top limbs that entered f29_reduce_weak
_op = [None]


def _reduce_weak(v):
    if _op[0] is not None:
        _seen_tops.setdefault(_op[0], set()).add(v[8])
    return M.f29_reduce_weak(F, v)


def fqx_zero():
    return [0] * 9


def fqx_add(a, b):
    return _reduce_weak(M.f29_add_lazy(a, b))


def fqx_sub(a, b):
    return _reduce_weak(M.f29_sub(F, 3, a, b))


def fqx_neg(a):
    return _reduce_weak(M.f29_neg(F, 3, a))


def fqx_9a_pm_b(a, b, minus):
    require(all(x < 1 << 29 for x in a[:8] + b[:8]), "9a_pm_b: operand not normalised")
    c3 = F.c(3)
    require(b[8] <= c3[8], "9a_pm_b: subtrahend too large")
    r, acc = [], 0
    for i in range(9):
        t = M._u32(c3[i] - b[i], "9a_pm_b") if minus else b[i]
        acc = M._acc(F, acc + 9 * a[i] + t)
        if i == 8 and acc > M32:
            raise OverflowError_("9a_pm_b: top limb does not fit 32 bits")
        r.append(acc & MASK if i < 8 else acc)
        acc >>= 29
    return _reduce_weak(r)


def fqx_inv(a):
    r, started = list(F.one), False
    pw = words(Q)
    for limb in range(7, -1, -1):
        w = pw[limb] - 2 if limb == 0 else pw[limb]
        for b in range(31, -1, -1):
            if started:
                r = M.f29_sqr(F, r)
            if (w >> b) & 1:
                r = M.f29_mul(F, r, a)
                started = True
    return r


def fq2x_add(a, b):
    return [fqx_add(a[0], b[0]), fqx_add(a[1], b[1])]


def fq2x_sub(a, b):
    return [fqx_sub(a[0], b[0]), fqx_sub(a[1], b[1])]


def fq2x_dbl(a):
    return fq2x_add(a, a)


def fq2x_neg(a):
    return [fqx_neg(a[0]), fqx_neg(a[1])]


def fq2x_conj(a):
    return [list(a[0]), fqx_neg(a[1])]


def fq2x_mul_xi(a):
    return [fqx_9a_pm_b(a[0], a[1], True), fqx_9a_pm_b(a[1], a[0], False)]


def fq2x_mul(a, b):
    return [M.f29_mul2(F, a[0], b[0], M.f29_neg(F, 3, a[1]), b[1]), M.f29_mul2(F, a[0], b[1], a[1], b[0])]


def fq2x_sqr(a):
    return [M.f29_mul(F, M.f29_add(a[0], a[1]), M.f29_sub(F, 3, a[0], a[1])), M.f29_mul(F, M.f29_add(a[0], a[0]), a[1])]


def fq2x_mul_fq(a, s):
    return [M.f29_mul(F, a[0], s), M.f29_mul(F, a[1], s)]


def pairing_exec(prog, R, K, lines, record=False):
    """R: the lane's registers, a list of [c0, c1] limb lists, changed in place; lines: packed canonical Fq (eight words
    each), four per P_LINE in order. `record`: note the top limbs that enter the weak reduction, per op."""
    lp = 0
    for w in prog:
        op, d, a, b = w >> 24, (w >> 16) & 255, (w >> 8) & 255, w & 255
        _op[0] = op if record else None
        if op in (P_MUL, P_MULK):
            R[d] = fq2x_mul(R[a], K[b] if op == P_MULK else R[b])
        elif op == P_SQR:
            R[d] = fq2x_sqr(R[a])
        elif op == P_ADD:
            R[d] = fq2x_add(R[a], R[b])
        elif op == P_SUB:
            R[d] = fq2x_sub(R[a], R[b])
        elif op == P_NEG:
            R[d] = fq2x_neg(R[a])
        elif op == P_CONJ:
            R[d] = fq2x_conj(R[a])
        elif op == P_MULXI:
            R[d] = fq2x_mul_xi(R[a])
        elif op == P_MOV:
            R[d] = [list(R[a][0]), list(R[a][1])]
        elif op == P_MOVK:
            R[d] = [list(K[b][0]), list(K[b][1])]
        elif op == P_MULFQ:
            R[d] = fq2x_mul_fq(R[a], R[b][0])
        elif op == P_FQINV:
            R[d] = [fqx_inv(R[a][0]), fqx_zero()]
        else:  # P_LINE (the C code's default)
            R[d] = [M.f29_unpack(lines[lp]), M.f29_unpack(lines[lp + 1])]
            R[d + 1] = [M.f29_unpack(lines[lp + 2]), M.f29_unpack(lines[lp + 3])]
            lp += 4
    _op[0] = None


# ------------------------------------------------------------------------------------------ values
def res(c):
    """The field element a limb vector in radix 2^261 stands for."""
    return val(c) * F.rinv % Q


def res2(x):
    return (res(x[0]), res(x[1]))


def stored(x, lift=0):
    """Limbs of the field element x in radix 2^261: the canonical representative plus lift * p."""
    return digits(x * RADIX % Q + lift * Q)


def stored2(c, lifts=(0, 0)):
    return [stored(c[0], lifts[0]), stored(c[1], lifts[1])]


def line_words(x):
    """A prepared line coefficient as the library keeps it: packed canonical, radix 2^261."""
    return words(x * RADIX % Q)


def to_fq2x(c):
    """pairing.hpp's to_fq2x on a canonical Montgomery (R = 2^256) constant: one f29_mul by k_in, below 2p."""
    return [M.fq29_from_r256(words(c[0] * R256 % Q)), M.fq29_from_r256(words(c[1] * R256 % Q))]


@functools.lru_cache(maxsize=None)
def gammas():
    """xi^(i (p^k - 1)/6) for k = 1..3, i = 1..5, as integers."""
    return tuple(X.f2_pow(X.XI, i * (Q**k - 1) // 6) for k in (1, 2, 3) for i in range(1, 6))


@functools.lru_cache(maxsize=None)
def _consts():
    return [[fqx_zero(), fqx_zero()], [list(F.one), fqx_zero()]] + [to_fq2x(g) for g in gammas()]


def device_consts():
    return [[list(c[0]), list(c[1])] for c in _consts()]


def K_RES():
    """The field elements the constant table stands for."""
    return [(0, 0), (1, 0)] + list(gammas())


# ------------------------------------------------------------------------------------------ reference A
def _coeff(c, want, num, den, what):
    assert all(x < 1 << 29 for x in c[:8]), what + ": not normalised"
    assert val(c) * den < num * Q, "%s: not below %s p" % (what, num / den)
    assert res(c) == want % Q, what + ": wrong residue"


WEAK, PROD = (10003, 10000), (2, 1)  # the two documented bounds of a stored coefficient


def a_word(op, A, B):
    """What one word means, on field elements A = (a0, a1), B = (b0, b1) of Fq2 = Fq[u]/(u^2 + 1)."""
    a0, a1 = A
    b0, b1 = B
    if op in (P_MUL, P_MULK):
        return ((a0 * b0 - a1 * b1) % Q, (a0 * b1 + a1 * b0) % Q)
    if op == P_SQR:
        return ((a0 * a0 - a1 * a1) % Q, 2 * a0 * a1 % Q)
    if op == P_ADD:
        return ((a0 + b0) % Q, (a1 + b1) % Q)
    if op == P_SUB:
        return ((a0 - b0) % Q, (a1 - b1) % Q)
    if op == P_NEG:
        return (-a0 % Q, -a1 % Q)
    if op == P_CONJ:
        return (a0, -a1 % Q)
    if op == P_MULXI:
        return ((9 * a0 - a1) % Q, (9 * a1 + a0) % Q)
    if op == P_MULFQ:
        return (a0 * b0 % Q, a1 * b0 % Q)
    if op == P_FQINV:
        return (pow(a0, -1, Q) if a0 % Q else 0, 0)
    raise AssertionError(op)


def judge_word(word, pre, out):
    """Reference A on one executed word (P_LINE apart). pre: register -> value before; out: register -> value after."""
    op, d, a, b = word >> 24, (word >> 16) & 255, (word >> 8) & 255, word & 255
    what = OP_NAMES[op]
    got = out[d]
    if op == P_MOV:
        assert got == pre[a], "mov: not a copy"
    elif op == P_MOVK:
        assert got == device_consts()[b], "movk: not the constant"
    else:
        B = K_RES()[b] if op == P_MULK else res2(pre[b]) if op in (P_MUL, P_ADD, P_SUB, P_MULFQ) else (0, 0)
        want = a_word(op, res2(pre[a]), B)
        bound = WEAK if op in (P_ADD, P_SUB, P_NEG, P_MULXI) else PROD
        if op == P_CONJ:
            assert got[0] == pre[a][0], "conj: c0 not a copy"
            _coeff(got[1], want[1], *WEAK, "conj c1")
        elif op == P_FQINV:
            _coeff(got[0], want[0], *PROD, "fqinv c0")
            assert got[1] == [0] * 9, "fqinv: c1 not zero"
        else:
            _coeff(got[0], want[0], *bound, what + " c0")
            _coeff(got[1], want[1], *bound, what + " c1")


def regs_f12(regs6):
    """Six registers in tower order -> pairing_ref's Fq12; every coefficient must be in stored form (normalised, below 2p)."""
    t = []
    for r in regs6:
        for c in r:
            assert all(x < 1 << 29 for x in c[:8]) and val(c) < 2 * Q, "result not in stored form"
            t.append(res(c))
    return X.f12_from_tower(t)


def regs_f6(regs3):
    return regs_f12(list(regs3) + [[fqx_zero(), fqx_zero()]] * 3)


def f12_regs(f, lifts=None):
    t = X.f12_to_tower(f)
    lifts = lifts or [0] * 12
    return [[stored(t[2 * i], lifts[2 * i]), stored(t[2 * i + 1], lifts[2 * i + 1])] for i in range(6)]


@functools.lru_cache(maxsize=None)
def f12_inv(a):
    return X.f12_inv(a) if any(a) else a


@functools.lru_cache(maxsize=None)
def f12_pow(a, e):
    return X.f12_pow(a, e)


# ------------------------------------------------------------------------------------------ the harness, host build
def host_binary():
    """tests/native/fq12_check_host, rebuilt when missing or older than what it is made from."""
    exe = os.path.join(NATIVE, "fq12_check_host")
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in DEPS):
        subprocess.run(["make", "-C", NATIVE, "fq12_check_host"], check=True, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return exe


_emitted = {}


def _emit_many(requests):
    """(K limbs, [(regs, words)]) from the harness' --emit mode."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "requests.txt")
        with open(path, "w") as f:
            f.write("".join(" ".join(str(x) for x in r) + "\n" for r in requests))
        p = subprocess.run([host_binary(), "--emit", path], check=True, timeout=300, stdout=subprocess.PIPE, text=True)
    K, progs = [], []
    for ln in p.stdout.splitlines():
        t = ln.split()
        if t[0] == "K":
            v = [int(x, 16) for x in t[2:]]
            K.append([v[:9], v[9:]])
        else:
            w = [int(x, 16) for x in t[3:]]
            assert t[0] == "prog" and len(w) == int(t[2])
            progs.append((int(t[1]), w))
    assert len(K) == K_COUNT and len(progs) == len(requests)
    return K, progs


def emit(kind, args=()):
    """(regs, words) of emitter `kind` with `args` = (base, register arguments...), as csrc/pairing.hpp emits them."""
    key = (kind,) + tuple(args)
    if key not in _emitted:
        _emitted[key] = _emit_many([key])[1][0]
    return _emitted[key]


def harness_consts():
    return _emit_many([])[0]


# ------------------------------------------------------------------------------------------ cases
class Case:
    """One lane of the harness: a program (raw words, or an emitter id with its arguments), the slab size, input
    registers, lines, the registers to return. `expect`: reference B's registers (None where B did not run); `check`:
    reference A on the returned registers; `same`: registers that must come back as they went in."""

    def __init__(self, tag, what, kind, args, prog, regs, inputs, lines, outs, check, run_b=True, record=False):
        self.tag, self.what, self.kind, self.args, self.prog, self.regs = tag, what, kind, list(args), list(prog), regs
        self.inputs, self.lines, self.outs, self.check = dict(inputs), [list(l) for l in lines], list(outs), check
        assert 0 < regs <= 256 and all(0 <= r < regs for r in list(self.inputs) + self.outs) and len(self.lines) % 4 == 0
        self.pre = {r: self.inputs.get(r, pattern_reg(r)) for r in self.outs}
        self.expect = None
        if run_b:
            R = [self.inputs.get(r) or pattern_reg(r) for r in range(regs)]
            pairing_exec(self.prog, R, device_consts(), self.lines, record)
            self.expect = sum((R[r][0] + R[r][1] for r in self.outs), [])

    def describe(self):
        body = " ".join("%08x" % w for w in self.prog[:8]) + (" ..." if len(self.prog) > 8 else "")
        ins = "; ".join("R%d = %s | %s" % (r, " ".join("%x" % x for x in v[0]), " ".join("%x" % x for x in v[1])) for r, v in sorted(self.inputs.items()))
        return "%s [%s] regs=%d words=%d (%s) %s" % (self.tag, self.what, self.regs, len(self.prog), body, ins)

    def record(self):
        """The words of this case in the harness' case file."""
        given = self.prog if self.kind == E_RAW else self.args
        out = [self.kind, self.regs, len(given), len(self.inputs), len(self.lines) // 4, len(self.outs)] + list(given)
        for r, v in sorted(self.inputs.items()):
            out += [r] + v[0] + v[1]
        for l in self.lines:
            out += l
        return out + self.outs

    def judge(self, got_words):
        got = {r: [got_words[18 * i:18 * i + 9], got_words[18 * i + 9:18 * i + 18]] for i, r in enumerate(self.outs)}
        self.check(got, self.pre)


def case_file(cases):
    import struct
    body = [MAGIC, len(cases)]
    for c in cases:
        body += c.record()
    return struct.pack("<%dI" % len(body), *body)


def read_results(raw, cases):
    import struct
    n_words = sum(18 * len(c.outs) for c in cases)
    assert struct.unpack_from("<3I", raw) == (MAGIC, len(cases), REPLICAS) and len(raw) == 12 + 4 * REPLICAS * n_words
    w = struct.unpack_from("<%dI" % (REPLICAS * n_words), raw, 12)
    out, pos = [], 0
    for _ in range(REPLICAS):
        rep = []
        for c in cases:
            rep.append(list(w[pos:pos + 18 * len(c.outs)]))
            pos += 18 * len(c.outs)
        out.append(rep)
    return out


def run_harness(exe, cases, workdir, env=None, timeout=300):
    """One child process: (results[replica][case], report line, the finished process)."""
    inp, outp = os.path.join(workdir, "fq12_cases.bin"), os.path.join(workdir, "fq12_results.bin")
    with open(inp, "wb") as f:
        f.write(case_file(cases))
    p = subprocess.run([exe, inp, outp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, env=env)
    assert p.returncode == 0, "%s exit %d (2 HIP error, 3 not gfx950, 4 case file, -6 a bound violated): %s %s" % (
        os.path.basename(exe), p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return read_results(open(outp, "rb").read(), cases), p.stdout.strip(), p


# ---- coefficient classes
def coeff_classes(seed=61):
    """(name, limbs): stored coefficients at the edges of the invariant `normalised and below 2p`."""
    rnd = random.Random(seed)
    named = [("0", 0), ("1", 1), ("M(1)", RADIX % Q), ("p-1", Q - 1), ("p", Q), ("p+1", Q + 1), ("2p-1", 2 * Q - 1),
             ("random canonical", rnd.randrange(Q)), ("random in [p, 2p)", Q + rnd.randrange(Q))]
    out = [(n, digits(v)) for n, v in named]
    for i in range(9):
        hot = [0] * 9
        hot[i] = MASK if i < 8 else (2 * Q - 1) >> 232
        out.append(("limb %d hot" % i, hot))
    out.append(("limbs 0..7 = 2^29-1, largest top limb below 2p", M._top_for([MASK] * 8, 2 * Q - 1)))
    assert all(val(c) < 2 * Q and max(c[:8]) <= MASK for _, c in out)
    return out


def rw_boundaries(vmin, vmax):
    """(top limb, value) for every boundary k (p8 + 1) + d, d in -2..2, of f29_reduce_weak's quotient estimate whose value
    (lower limbs all 0 or all 2^29 - 1) lies in [vmin, vmax)."""
    out = []
    for k in range(1, 22):
        for d in (-2, -1, 0, 1, 2):
            t = k * (P8 + 1) + d
            for low in (0, (1 << 232) - 1):
                if vmin <= (t << 232) + low < vmax:
                    out.append((t, (t << 232) + low))
    return out


def rw_estimate_sets(tops):
    """fp29_model.class_reduce_weak's split: where the quotient estimate is exact, and where it is one short."""
    exact = {t for t in tops if (t * F.recip42) >> 42 == t // (P8 + 1)}
    short = {t for t in tops if (t * F.recip42) >> 42 == t // (P8 + 1) - 1}
    assert exact | short == set(tops)
    return exact, short


def _word_case(op, what, d, a, b, inputs, regs=6, lines=(), outs=None, record=True, prog=None):
    prog = prog or [pair_word(op, d, a, b)]
    outs = list(range(regs)) if outs is None else outs
    ln = [list(l) for l in lines]

    assert len(prog) == 1 or all(w >> 24 == P_LINE for w in prog), "more than one word only for P_LINE in a row"

    def check(got, pre):
        if op == P_LINE:  # the last line written to a register is what it holds
            last = {}
            for i, w in enumerate(prog):
                wd = (w >> 16) & 255
                last[wd], last[wd + 1] = ln[4 * i:4 * i + 2], ln[4 * i + 2:4 * i + 4]
            for r, pair in last.items():
                for c, packed in zip(got[r], pair):
                    assert all(x < 1 << 29 for x in c) and val(c) == M.from_words(packed) < Q, "line: register %d is not the packed value" % r
            touched = set(last)
        else:
            judge_word(prog[0], pre, got)
            touched = {d}
        for r in got:
            if r not in touched:
                assert got[r] == pre[r], "register %d changed" % r
    return Case(OP_NAMES[op], what, E_RAW, (), prog, regs, inputs, ln, outs, check, record=record)


def single_word_cases(seed=67):
    rnd = random.Random(seed)
    C = coeff_classes()
    n = len(C)
    cs = []
    G0, RA, RB, RD = 0, 1, 2, 3  # registers of the six-register slab: guard, a, b, d, d + 1, guard
    fq2 = lambda i, j: [list(C[i][1]), list(C[j][1])]
    nm = lambda i, j: "(%s, %s)" % (C[i][0], C[j][0])
    junk = [[M32] * 9, [0xDEADBEEF] * 9]
    # every pair of classes in a; for the binary ops a second operand that walks the classes, and the same with the roles swapped
    for i in range(n):
        for j in range(n):
            k, l = (7 * i + 3 * j + 1) % n, (5 * i + 11 * j + 2) % n
            for op in (P_SQR, P_NEG, P_CONJ, P_MULXI, P_MOV):
                cs.append(_word_case(op, nm(i, j), RD, RA, 0, {RA: fq2(i, j)}))
            for op in (P_MUL, P_ADD, P_SUB):
                cs.append(_word_case(op, nm(i, j) + " . " + nm(k, l), RD, RA, RB, {RA: fq2(i, j), RB: fq2(k, l)}))
                cs.append(_word_case(op, nm(k, l) + " . " + nm(i, j), RD, RA, RB, {RA: fq2(k, l), RB: fq2(i, j)}))
            cs.append(_word_case(P_MULFQ, nm(i, j) + " * %s, junk in R[b].c1" % C[k][0], RD, RA, RB, {RA: fq2(i, j), RB: [list(C[k][1]), junk[l % 2]]}))
    top, zero = n_index(C, "2p-1"), n_index(C, "0")
    cs.append(_word_case(P_MUL, "all four coefficients 2p-1: the 10 p^2 and 8 p^2 sums", RD, RA, RB, {RA: fq2(top, top), RB: fq2(top, top)}))
    for i in range(n):
        cs.append(_word_case(P_MUL, "zero . " + nm(i, top), RD, RA, RB, {RA: fq2(zero, zero), RB: fq2(i, top)}))
        cs.append(_word_case(P_MUL, nm(top, i) + " . zero", RD, RA, RB, {RA: fq2(top, i), RB: fq2(zero, zero)}))
    for kb in range(K_COUNT):
        cs.append(_word_case(P_MOVK, "K[%d]" % kb, RD, 0, kb, {}))
        for i in range(n):
            cs.append(_word_case(P_MULK, nm(i, (i + kb) % n) + " . K[%d]" % kb, RD, RA, kb, {RA: fq2(i, (i + kb) % n)}))
        cs.append(_word_case(P_MULK, "all 2p-1 . K[%d]" % kb, RD, RA, kb, {RA: fq2(top, top)}))
    # P_SQR: a0 + a1 = 0 mod p in every pair of representations (a0 == a1, a1 == 0 and both 2p - 1 are in the cross above)
    for _ in range(8):
        x = rnd.randrange(1, Q)
        for la in (0, 1):
            for lb in (0, 1):
                cs.append(_word_case(P_SQR, "a0 + a1 = 0 mod p, lifts %d %d" % (la, lb), RD, RA, 0, {RA: [stored(x, la), stored(Q - x, lb)]}))
    # P_MULXI: b with its top limb at the c3(8) bound of fqx_9a_pm_b — the REQUIRE's edge, beyond the stored invariant
    c3_8 = F.c(3)[8]
    for t8 in (c3_8, c3_8 - 1):
        for a0 in (C[zero][1], C[top][1], stored(rnd.randrange(Q))):
            cs.append(_word_case(P_MULXI, "subtrahend's top limb at c3(8)%+d" % (t8 - c3_8), RD, RA, 0, {RA: [list(a0), [0] * 8 + [t8]]}))
    # the value entering f29_reduce_weak with its top limb at every reachable boundary of the quotient estimate
    hit = {op: set() for op in (P_ADD, P_SUB, P_NEG, P_CONJ, P_MULXI)}
    other = lambda: stored(rnd.randrange(Q), rnd.randrange(2))
    amax = {0: 2 * P8, (1 << 232) - 1: 2 * P8 - 1}
    for t, v in rw_boundaries(0, 4 * Q):  # P_ADD: the sum is lazy, its top limb is a8 + b8
        low = v - (t << 232)
        if t <= 2 * amax[low]:
            a8 = min(t, amax[low])
            a, b = digits((a8 << 232) + low), digits(((t - a8) << 232) + low)
            assert val(a) < 2 * Q and val(b) < 2 * Q
            cs.append(_word_case(P_ADD, "reduce_weak top limb %#x" % t, RD, RA, RB, {RA: [a, other()], RB: [b, other()]}))
            cs.append(_word_case(P_ADD, "reduce_weak top limb %#x, c1" % t, RD, RA, RB, {RA: [other(), b], RB: [other(), a]}))
            hit[P_ADD].add(t)
    for t, v in rw_boundaries(Q + 1, 5 * Q):  # P_SUB: a - b + 3p = v
        a, b = (v - 3 * Q, 0) if v >= 3 * Q else (0, 3 * Q - v)
        s = rnd.randrange(2 * Q - max(a, b))
        cs.append(_word_case(P_SUB, "reduce_weak top limb %#x" % t, RD, RA, RB, {RA: [digits(a + s), other()], RB: [digits(b + s), other()]}))
        cs.append(_word_case(P_SUB, "reduce_weak top limb %#x, c1" % t, RD, RA, RB, {RA: [other(), digits(a)], RB: [other(), digits(b)]}))
        hit[P_SUB].add(t)
    for t, v in rw_boundaries(Q + 1, 3 * Q + 1):  # P_NEG, P_CONJ: 3p - a = v
        cs.append(_word_case(P_NEG, "reduce_weak top limb %#x" % t, RD, RA, 0, {RA: [digits(3 * Q - v), other()]}))
        cs.append(_word_case(P_NEG, "reduce_weak top limb %#x, c1" % t, RD, RA, 0, {RA: [other(), digits(3 * Q - v)]}))
        cs.append(_word_case(P_CONJ, "reduce_weak top limb %#x" % t, RD, RA, 0, {RA: [other(), digits(3 * Q - v)]}))
        hit[P_NEG].add(t), hit[P_CONJ].add(t)
    for t, v in rw_boundaries(Q + 1, 21 * Q):  # P_MULXI: 9 a0 - a1 + 3p = v and 9 a1 + a0 = v
        D = v - 3 * Q
        lo, hi = max(0, -D), min(2 * Q, 18 * Q - D) - 9
        if lo < hi:
            r = rnd.randrange(lo, hi)
            a1 = r + (-(D + r)) % 9
            cs.append(_word_case(P_MULXI, "reduce_weak top limb %#x in 9 a0 - a1 + 3p" % t, RD, RA, 0, {RA: [digits((D + a1) // 9), digits(a1)]}))
            hit[P_MULXI].add(t)
        lo, hi = max(0, v - 18 * Q + 9), min(v, 2 * Q) - 9
        if lo < hi and v < 20 * Q:
            r = rnd.randrange(lo, hi)
            a0 = r + (v - r) % 9
            cs.append(_word_case(P_MULXI, "reduce_weak top limb %#x in 9 a1 + a0" % t, RD, RA, 0, {RA: [digits(a0), digits((v - a0) // 9)]}))
            hit[P_MULXI].add(-t)
    # P_FQINV: every class, junk in the input's c1 and in the destination (the prefill)
    for i in range(n):
        cs.append(_word_case(P_FQINV, C[i][0] + ", junk in c1", RD, RA, 0, {RA: [list(C[i][1]), junk[i % 2]]}))
    # P_LINE: three in a row (the pointer advances), lines 0 and p - 1, d + 1 the last register
    lv = [0, Q - 1, 1, rnd.randrange(Q)] + [rnd.randrange(Q) for _ in range(8)]
    L = [line_words(x) for x in lv]
    cs.append(_word_case(P_LINE, "three in a row", 0, 0, 0, {}, regs=8, lines=L, prog=[pair_word(P_LINE, 1), pair_word(P_LINE, 3), pair_word(P_LINE, 5)]))
    cs.append(_word_case(P_LINE, "three in a row into the same registers", 0, 0, 0, {}, regs=8, lines=L[4:] + L[:4], prog=[pair_word(P_LINE, 6)] * 3))
    cs.append(_word_case(P_LINE, "0 and p - 1; d + 1 the last register", 6, 0, 0, {}, regs=8, lines=L[:4]))
    cs.append(_word_case(P_LINE, "d + 1 the last register", 4, 0, 0, {}, lines=L[4:8]))
    # aliasing: d == a, d == b, a == b, all three equal
    ops3, ops2 = (P_MUL, P_ADD, P_SUB, P_MULFQ), (P_SQR, P_NEG, P_CONJ, P_MULXI, P_MOV, P_MULK, P_FQINV)
    vals = [fq2(top, top), [stored(rnd.randrange(Q)), stored(rnd.randrange(Q), 1)], [stored(rnd.randrange(Q), 1), stored(rnd.randrange(Q))]]
    for vi, x in enumerate(vals):
        y = vals[(vi + 1) % len(vals)]
        for op in ops3:
            for what, (d, a, b) in (("d == a", (RA, RA, RB)), ("d == b", (RB, RA, RB)), ("a == b", (RD, RA, RA)), ("d == a == b", (RA, RA, RA))):
                cs.append(_word_case(op, "aliasing, " + what, d, a, b, {RA: x, RB: y}))
        for op in ops2:
            cs.append(_word_case(op, "aliasing, d == a", RA, RA, K_GAMMA + vi if op == P_MULK else 0, {RA: x}))
    # register 255 as d, a and b
    ends = [253, 254, 255]
    for vi, x in enumerate(vals):
        y = vals[(vi + 1) % len(vals)]
        for op in ops3:
            for d, a, b in ((255, 1, 2), (1, 255, 2), (1, 2, 255), (255, 255, 255), (255, 254, 253)):
                cs.append(_word_case(op, "register 255", d, a, b, {a: x, b: y} if a != b else {a: x}, regs=256, outs=sorted({0, 1, 2, 3, d, a, b} | set(ends))))
        for op in ops2:
            for d, a in ((255, 1), (1, 255), (255, 255)):
                cs.append(_word_case(op, "register 255", d, a, K_COUNT - 1 if op == P_MULK else 0, {a: x}, regs=256, outs=sorted({0, 1, 2, d, a} | set(ends))))
    cs.append(_word_case(P_MOVK, "register 255", 255, 0, K_COUNT - 1, {}, regs=256, outs=[0, 1] + ends))
    cs.append(_word_case(P_LINE, "registers 254 and 255", 254, 0, 0, {}, regs=256, lines=L[8:12], outs=[0, 1] + ends))
    # coverage: every boundary that can be reached was reached, with the estimate exact and one short, in every op
    for op, (vmin, vmax) in ((P_ADD, (0, 4 * Q)), (P_SUB, (Q + 1, 5 * Q)), (P_NEG, (Q + 1, 3 * Q + 1)), (P_CONJ, (Q + 1, 3 * Q + 1)), (P_MULXI, (Q + 1, 21 * Q))):
        tops = {abs(t) for t in hit[op]}
        want = {t for t, _ in rw_boundaries(vmin, vmax)}
        if op == P_ADD:
            want = {t for t in want if t <= 4 * P8 - 2}
        assert tops == want, (OP_NAMES[op], sorted(want - tops))
        exact, short = rw_estimate_sets(tops)
        assert exact and short and tops <= _seen_tops[op], "%s: reference B did not see the top limbs the builder aimed at" % OP_NAMES[op]
        assert (exact & _seen_tops[op]) and (short & _seen_tops[op])
        if op == P_MULXI:
            assert {-t for t in tops if t <= 19 * P8} <= hit[op], "mulxi: the sum 9 a1 + a0 misses boundaries"
    return cs


def n_index(C, name):
    return [i for i, (n, _) in enumerate(C) if n == name][0]


# ---- emitters and programs
def _lifted(rnd, f):
    return f12_regs(f, [rnd.randrange(2) for _ in range(12)])


def _rand12(rnd):
    return tuple(rnd.randrange(Q) for _ in range(12))


def _tower(vals12):
    return X.f12_from_tower(list(vals12))


def TOP_REG():
    return [digits(2 * Q - 1), digits(2 * Q - 1)]


def ZERO_REG():
    return [fqx_zero(), fqx_zero()]


def f12_inputs(seed=71):
    """(name, six registers): the inputs of section 3 of the issue for an Fq12 emitter."""
    rnd = random.Random(seed)
    z = [0] * 12
    sub6 = [rnd.randrange(Q) for _ in range(6)] + [0] * 6
    c0zero = [0] * 6 + [rnd.randrange(Q) for _ in range(6)]
    sparse = [rnd.randrange(Q), 0, 0, 0, 0, 0] + [rnd.randrange(Q) for _ in range(4)] + [0, 0]  # y_P + l3 w + l4 v w
    return [("0", f12_regs(_tower(z))), ("1", f12_regs(X.F12_ONE)), ("in the Fq6 subfield", _lifted(rnd, _tower(sub6))),
            ("c0 = 0", _lifted(rnd, _tower(c0zero))), ("line-shaped", _lifted(rnd, _tower(sparse))), ("all twelve at 2p-1", [TOP_REG() for _ in range(6)]),
            ("random, lifted", _lifted(rnd, _rand12(rnd))), ("random, lifted (2)", _lifted(rnd, _rand12(rnd)))]


def f6_inputs(seed=73):
    rnd = random.Random(seed)
    full = f12_inputs(seed)
    return [(n, r[:3]) for n, r in full if n != "c0 = 0"] + [("c2 = 0", _lifted(rnd, _tower([rnd.randrange(Q) for _ in range(4)] + [0] * 8))[:3])]


@functools.lru_cache(maxsize=None)
def gt_values():
    """A GT value of the reference, its inverse, and 1."""
    g = X.pairing(X.G1_GEN, X.G2_GEN)
    ginv = X.f12_pow(g, X.R - 1)
    assert X.f12_mul(g, ginv) == X.F12_ONE and g != X.F12_ONE
    return (("1", X.F12_ONE), ("e(G1, G2)", g), ("1 / e(G1, G2)", ginv))


def gt_inputs(seed=79):
    rnd = random.Random(seed)
    return [(n + (", lifted" if k else ""), _lifted(rnd, f) if k else f12_regs(f)) for n, f in gt_values() for k in range(2)]


def _place(regs_list, at):
    return {at + i: r for i, r in enumerate(regs_list)}


def emitter_case(kind, what, layout, operands, result, want, run_b=True, result_check=None):
    """layout: the emitter's register arguments (after base); operands: {first register: registers}; result: (first register,
    count); want(pre) -> the Fq12 the result must be (six registers, or three padded). Registers 0 and p.regs are guards."""
    inputs = {}
    for at, regs in operands.items():
        inputs.update(_place(regs, at))
    used = max(list(inputs) + [result[0] + result[1] - 1])
    base = used + 1
    args = [base] + list(layout)
    p_regs, prog = emit(kind, args)
    regs = p_regs + 1
    outs = sorted({0, p_regs} | set(inputs) | set(range(result[0], result[0] + result[1])))
    res_regs = list(range(result[0], result[0] + result[1]))

    def check(got, pre):
        for r in got:
            if r not in res_regs:
                assert got[r] == pre[r], "register %d changed" % r
        out = [got[r] for r in res_regs]
        if result_check:
            result_check(out, pre)
        else:
            f = regs_f12(out) if len(out) == 6 else regs_f6(out)
            assert f == want(pre), "wrong element of Fq12"
    return Case(EMITTER_NAMES[kind], what, kind, args, prog, regs, inputs, (), outs, check, run_b=run_b)


def _f12_at(pre, at):
    return regs_f12([pre[at + i] for i in range(6)])


def _f6_at(pre, at):
    return regs_f6([pre[at + i] for i in range(3)])


def _v_times(f):
    return X.f12_mul(f, X.f12_from_fq2((1, 0), 2))  # v = w^2


def emitter_cases(seed=83):
    rnd = random.Random(seed)
    cs = []
    i12, i6, igt = f12_inputs(), f6_inputs(), gt_inputs()
    A, B_, D = 1, 7, 13  # out of place: a at 1.., b at 7.., the destination at 13.. (register 0 is a guard)
    for n, (name, a) in enumerate(i12):
        b = i12[(n + 3) % len(i12)][1]
        bn = i12[(n + 3) % len(i12)][0]
        # unary Fq12 emitters: out of place and in place
        for kind, want in ((E12_SQR, lambda f: X.f12_mul(f, f)), (E12_INV, f12_inv)):
            for what, (d, s) in (("out of place", (D, A)), ("r == a", (A, A))):
                cs.append(emitter_case(kind, name + ", " + what, (d, s), {s: a}, (d, 6), lambda pre, s=s, want=want: want(_f12_at(pre, s))))
        for k in (1, 2, 3):
            for what, (d, s) in (("out of place", (D, A)), ("r == a", (A, A))):
                cs.append(emitter_case(E12_FROBENIUS, "k = %d, %s, %s" % (k, name, what), (d, s, k), {s: a}, (d, 6),
                                       lambda pre, s=s, k=k: f12_pow(_f12_at(pre, s), Q**k)))
        for what, (d, s) in (("out of place", (D, A)), ("r == a", (A, A))):
            cs.append(emitter_case(E12_CONJ, name + ", " + what, (d, s), {s: a}, (d, 6),
                                   (lambda pre, s=s: f12_pow(_f12_at(pre, s), Q**6)) if n >= 6 else
                                   (lambda pre, s=s: X.f12_from_tower([(-x) % Q if i >= 6 else x for i, x in enumerate(X.f12_to_tower(_f12_at(pre, s)))]))))
        # e12_mul: out of place, r == a, r == b, a == b, all equal
        for what, (d, s, t) in (("out of place", (D, A, B_)), ("r == a", (A, A, B_)), ("r == b", (B_, A, B_)), ("a == b", (D, A, A)), ("r == a == b", (A, A, A))):
            ops = {A: a} if t == s else {A: a, B_: b}
            cs.append(emitter_case(E12_MUL, "%s . %s, %s" % (name, bn, what), (d, s, t), ops, (d, 6),
                                   lambda pre, s=s, t=t: X.f12_mul(_f12_at(pre, s), _f12_at(pre, t))))
        # e12_mul_034: l0 = (y, 0) at 7, l3 at 8, l4 at 9
        l0 = [stored(rnd.randrange(Q), rnd.randrange(2)), fqx_zero()]
        l3, l4 = stored2((rnd.randrange(Q), rnd.randrange(Q)), (n & 1, 1)), stored2((rnd.randrange(Q), rnd.randrange(Q)), (1, n & 1))
        if n == 5:
            l0, l3, l4 = [digits(2 * Q - 1), fqx_zero()], TOP_REG(), TOP_REG()
        if n == 0:
            l0, l3, l4 = ZERO_REG(), ZERO_REG(), ZERO_REG()

        def line_of(pre):
            f = X.f12_add(X.f12_from_fq2(res2(pre[7]), 0), X.f12_from_fq2(res2(pre[8]), 1))
            return X.f12_add(f, X.f12_from_fq2(res2(pre[9]), 3))
        for what, d in (("out of place", D), ("r == a", A), ("r over l0, l3, l4", 7)):
            cs.append(emitter_case(E12_MUL_034, name + ", " + what, (d, A, 7, 8, 9), {A: a, 7: [l0, l3, l4]}, (d, 6),
                                   lambda pre: X.f12_mul(_f12_at(pre, A), line_of(pre))))
    # the Fq6 emitters: a at 1..3, b at 4..6, the destination at 7..9
    A6, B6, D6 = 1, 4, 7
    for n, (name, a) in enumerate(i6):
        b = i6[(n + 2) % len(i6)][1]
        for kind, want in ((E6_MUL_V, _v_times), (E6_SQR, lambda f: X.f12_mul(f, f)), (E6_INV, f12_inv)):
            for what, (d, s) in (("out of place", (D6, A6)), ("r == a", (A6, A6))):
                cs.append(emitter_case(kind, name + ", " + what, (d, s), {s: a}, (d, 3), lambda pre, s=s, want=want: want(_f6_at(pre, s))))
        for what, (d, s, t) in (("out of place", (D6, A6, B6)), ("r == a", (A6, A6, B6)), ("r == b", (B6, A6, B6)), ("a == b", (D6, A6, A6)), ("r == a == b", (A6, A6, A6))):
            ops = {A6: a} if t == s else {A6: a, B6: b}
            cs.append(emitter_case(E6_MUL, name + ", " + what, (d, s, t), ops, (d, 3), lambda pre, s=s, t=t: X.f12_mul(_f6_at(pre, s), _f6_at(pre, t))))
        b0, b1 = (TOP_REG(), TOP_REG()) if n == 4 else (stored2((rnd.randrange(Q), rnd.randrange(Q)), (1, 0)), stored2((rnd.randrange(Q), rnd.randrange(Q)), (0, 1)))
        for what, d in (("out of place", D6), ("r == a", A6), ("r over b0, b1", 4)):
            cs.append(emitter_case(E6_MUL_01, name + ", " + what, (d, A6, 4, 5), {A6: a, 4: [b0, b1]}, (d, 3),
                                   lambda pre: X.f12_mul(_f6_at(pre, A6), X.f12_add(X.f12_from_fq2(res2(pre[4]), 0), X.f12_from_fq2(res2(pre[5]), 2)))))
        # e4_sqr: (a0 + a1 s)^2 in Fq2[s]/(s^2 - xi); c0, c1 fresh registers
        def e4_check(out, pre):
            x, y = res2(pre[1]), res2(pre[2])
            xx, yy, xy = a_word(P_SQR, x, x), a_word(P_SQR, y, y), a_word(P_MUL, x, y)
            c0 = a_word(P_ADD, xx, a_word(P_MULXI, yy, yy))
            for c, want in zip(out[0] + out[1], c0 + a_word(P_ADD, xy, xy)):
                _coeff(c, want, *PROD, "e4_sqr")
        cs.append(emitter_case(E4_SQR, name, (3, 4, 1, 2), {1: a[:2]}, (3, 2), None, result_check=e4_check))
    # inside the cyclotomic subgroup
    for n, (name, a) in enumerate(igt):
        for what, (d, s) in (("out of place", (D, A)), ("r == a", (A, A))):
            cs.append(emitter_case(E12_CYCLOTOMIC_SQR, name + ", " + what, (d, s), {s: a}, (d, 6), lambda pre, s=s: X.f12_mul(_f12_at(pre, s), _f12_at(pre, s))))
            cs.append(emitter_case(E12_CONJ, name + ": the inverse, " + what, (d, s), {s: a}, (d, 6), lambda pre, s=s: f12_inv(_f12_at(pre, s))))
        cs.append(emitter_case(E12_POW_U, name, (D, A), {A: a}, (D, 6), lambda pre: f12_pow(_f12_at(pre, A), X.U), run_b=n in (2, 3)))
    return cs


def prepared_lines(q):
    """The line coefficients of one G2 point in the order the Miller program reads them, (-lambda, lambda x_T - y_T) per
    step, from pairing_ref's own chord-and-tangent arithmetic."""
    t, out = q, []

    def step(addend):
        nonlocal t
        lam = X.g2_slope(t, addend)
        c0, c1 = X.f2_sub((0, 0), lam), X.f2_sub(X.f2_mul(lam, t[0]), t[1])
        out.extend(line_words(v) for v in (c0[0], c0[1], c1[0], c1[1]))
        t = X.g2_add(t, addend)
    for bit in bin(X.ATE)[3:]:
        step(t)
        if bit == "1":
            step(q)
    q1 = X.g2_frobenius(q)
    step(q1)
    step(X.g2_neg(X.g2_frobenius(q1)))
    return out


A1, B1 = 0x9E3779B97F4A7C15F39CC0605CEDC834, 0x1082276BF3A27251F86C6A11D0C18E95


def program_cases(seed=89):
    rnd = random.Random(seed)
    cs = []
    pairs = [(X.G1_GEN, X.G2_GEN), (X.g1_mul(X.G1_GEN, A1), X.g2_mul(X.G2_GEN, B1))]
    m_regs, m_prog = emit(MILLER_PROGRAM)
    f_regs, f_prog = emit(FINAL_EXP_PROGRAM)
    u_regs, u_prog = emit(MUL_PROGRAM)
    F_OUT = list(range(MILLER_F, MILLER_F + 6))
    for n, (p, q) in enumerate(pairs):
        lines = prepared_lines(q)
        assert len(lines) == 4 * sum(1 for w in m_prog if w >> 24 == P_LINE)
        for lift in (0, 1):
            xp = [M.fq29_from_r256(words(p[0] * R256 % Q)), fqx_zero()] if not lift else [stored(p[0], 1), fqx_zero()]
            yp = [M.fq29_from_r256(words(p[1] * R256 % Q)), fqx_zero()] if not lift else [stored(p[1], 1), fqx_zero()]

            def check(got, pre, p=p, q=q):
                assert got[MILLER_XP] == pre[MILLER_XP] and got[MILLER_YP] == pre[MILLER_YP] and got[m_regs] == pre[m_regs], "a register changed"
                assert X.final_exp(regs_f12([got[r] for r in F_OUT])) == X.pairing(p, q), "the Miller value is off by more than a factor of a proper subfield"
            cs.append(Case("miller_program", "pair %d%s" % (n, ", x_P and y_P lifted" if lift else ""), MILLER_PROGRAM, (), m_prog, m_regs + 1,
                           {MILLER_XP: xp, MILLER_YP: yp}, lines, [MILLER_XP, MILLER_YP] + F_OUT + [m_regs], check, run_b=(n == 0)))
    fins = [("the Miller value of pair %d, lifted" % n, _lifted(rnd, X.miller(p, q))) for n, (p, q) in enumerate(pairs)]
    fins += [("1", f12_regs(X.F12_ONE)), ("0", f12_regs(_tower([0] * 12))), ("all twelve at 2p-1", [TOP_REG() for _ in range(6)])]
    for n, (name, a) in enumerate(fins):
        def check(got, pre):
            assert got[f_regs] == pre[f_regs], "the guard register changed"
            assert regs_f12([got[r] for r in range(6)]) == X.final_exp(regs_f12([pre[r] for r in range(6)])), "not f^((p^12 - 1)/r)"
        cs.append(Case("final_exp_program", name, FINAL_EXP_PROGRAM, (), f_prog, f_regs + 1, _place(a, FINAL_A), (), list(range(6)) + [f_regs], check, run_b=n in (0, 4)))
    i12 = f12_inputs(97)
    for n, (name, a) in enumerate(i12):
        b = i12[(n + 5) % len(i12)][1]

        def check(got, pre):
            assert got[u_regs] == pre[u_regs] and all(got[r] == pre[r] for r in range(6, 12)), "a register changed"
            assert regs_f12([got[r] for r in range(6)]) == X.f12_mul(_f12_at(pre, 0), _f12_at(pre, 6)), "not the product"
        ins = _place(a, FINAL_A)
        ins.update(_place(b, FINAL_B))
        cs.append(Case("mul_program", name, MUL_PROGRAM, (), u_prog, u_regs + 1, ins, (), list(range(12)) + [u_regs], check))
    return cs


@functools.lru_cache(maxsize=None)
def build_cases():
    """Every case, in launch order: the harness makes one launch of each run of cases with the same (kind, regs)."""
    _seen_tops.clear()
    cs = single_word_cases() + emitter_cases() + program_cases()
    order = {}
    for c in cs:
        order.setdefault((c.kind, c.regs), len(order))
    cs.sort(key=lambda c: order[(c.kind, c.regs)])
    groups = {}
    for c in cs:
        groups[(c.kind, c.regs)] = groups.get((c.kind, c.regs), 0) + 1
    assert min(groups.values()) >= 2, "a launch with one case: no lane of another case beside it"
    return tuple(cs)
