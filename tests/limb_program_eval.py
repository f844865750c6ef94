"""What a program of the quotient-domain interpreter computes, over Python integers mod r — before and after the host pass
(program.hip finalize_limb_program), so that a test can show that the pass preserves the value: its grouping by hot column,
the `* hot[k]` it takes out of a term, the powers of y that replace the Horner fold. Operands are drawn per (kind, arg) from
a seed: the same column word names the same value in both programs.

  raw programs        a stack machine; ACC is h = h * y + tos, STORE records an output
  finalised programs  WACC j adds tos * y^(K-1-j) to the wide sum (K = the number of WACC words); WFLUSH k does
                      h (=|+=) wide [* hot[k]] by bit 4 (a further `=` starts another piece: the pieces' h are summed);
                      REDUCE is the identity, SUB_BIG and NEG_BIG are SUB and NEG

and a seeded generator of valid raw programs over the opcodes a program may hold before the pass."""
import random

from limb_program_check import NAME, word

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


class Env:
    """Random operands: col(arg), const(arg), hot[k], y."""

    def __init__(self, seed):
        self.seed = seed
        self.y = self._draw("y", 0)
        self.hot = [self._draw("hot", k) for k in range(4)]

    def _draw(self, kind, arg):
        return random.Random("%d/%s/%d" % (self.seed, kind, arg)).randrange(R)

    def col(self, arg):
        return self._draw("col", arg)

    def const(self, arg):
        return self._draw("const", arg)


def evaluate(words, env):
    """(h, {STORE index: value}) of a raw or a finalised program."""
    K = sum(1 for w in words if NAME[w >> 24] == "WACC")
    st, outs = [], {}
    h, done, wide, flushed = 0, 0, 0, False
    for w in words:
        op, arg = NAME[w >> 24], w & 0xFFFFFF
        if op == "PUSH_COL":
            st.append(env.col(arg))
        elif op == "PUSH_CONST":
            st.append(env.const(arg))
        elif op == "PUSH_HOT":
            st.append(env.hot[arg])
        elif op == "MUL_COL":
            st[-1] = st[-1] * env.col(arg) % R
        elif op == "MUL_CONST":
            st[-1] = st[-1] * env.const(arg) % R
        elif op == "MUL_HOT":
            st[-1] = st[-1] * env.hot[arg] % R
        elif op == "ADD_COL":
            st[-1] = (st[-1] + env.col(arg)) % R
        elif op == "ADD_CONST":
            st[-1] = (st[-1] + env.const(arg)) % R
        elif op == "SUB_COL":
            st[-1] = (st[-1] - env.col(arg)) % R
        elif op == "ADD":
            b = st.pop()
            st[-1] = (st[-1] + b) % R
        elif op in ("SUB", "SUB_BIG"):
            b = st.pop()
            st[-1] = (st[-1] - b) % R
        elif op == "MUL":
            b = st.pop()
            st[-1] = st[-1] * b % R
        elif op in ("NEG", "NEG_BIG"):
            st[-1] = -st[-1] % R
        elif op == "SQR":
            st[-1] = st[-1] * st[-1] % R
        elif op == "REDUCE":
            pass
        elif op == "ACC":
            h = (h * env.y + st.pop()) % R
        elif op == "STORE":
            outs[arg] = st.pop()
        elif op == "WACC":
            wide = (wide + st.pop() * pow(env.y, K - 1 - (arg & 0x7FFFFF), R)) % R
        elif op == "WFLUSH":
            g = wide * (env.hot[arg & 7] if arg & 7 < 4 else 1) % R
            if arg & 16:
                assert flushed or h == 0
                done, h = (done + h) % R, g  # the piece before this one is complete
            else:
                assert flushed, "the first flush must overwrite h"
                h = (h + g) % R
            wide, flushed = 0, True
        elif op == "PICK":
            st.append(st[-1 - arg])
        elif op == "NIP":
            del st[len(st) - 1 - arg:len(st) - 1]
        elif op == "END":
            pass
        else:
            raise AssertionError("no such instruction: %r" % (op,))
    assert not st and wide == 0
    return (done + h) % R, outs


# ------------------------------------------------------------------------------------------------ the generator
class _Gen:
    """Expressions as word lists. `sz` is the stack size where the expression starts: it leaves sz + 1. Biased toward what
    makes bounds grow: long fused sums, differences of differences, products of sums."""

    def __init__(self, rnd):
        self.rnd = rnd

    def col(self):
        return self.rnd.randrange(1 << 24)

    def leaf(self, sz):
        x = self.rnd.random()
        if sz > 0 and x < 0.2:
            return [word("PICK", self.rnd.randrange(sz))]
        if x < 0.75:
            return [word("PUSH_COL", self.col())]
        if x < 0.9:
            return [word("PUSH_CONST", self.rnd.randrange(64))]
        return [word("PUSH_HOT", self.rnd.randrange(4))]

    def fused(self):
        x = self.rnd.random()
        if x < 0.45:
            return word("ADD_COL", self.col())
        if x < 0.6:
            return word("ADD_CONST", self.rnd.randrange(64))
        if x < 0.8:
            return word("SUB_COL", self.col())
        if x < 0.9:
            return word("MUL_COL", self.col())
        if x < 0.95:
            return word("MUL_CONST", self.rnd.randrange(64))
        return word("MUL_HOT", self.rnd.randrange(4))

    def long_sum(self, sz, budget):
        out = self.expr(sz, budget // 2)
        for _ in range(self.rnd.choice((3, 7, 8, 9, 20, 38, 39, 40, 41, 45, 90))):
            out.append(word("ADD_COL", self.col()) if self.rnd.random() < 0.7 else word("ADD_CONST", self.rnd.randrange(64)))
        return out

    def expr(self, sz, budget):
        rnd = self.rnd
        if budget <= 0 or sz >= 10:
            return self.leaf(sz)
        x = rnd.random()
        if x < 0.15:
            return self.leaf(sz)
        if x < 0.35:
            return self.long_sum(sz, budget)
        if x < 0.5:
            return self.expr(sz, budget - 1) + [self.fused() for _ in range(rnd.randrange(1, 6))]
        if x < 0.8:
            a = self.expr(sz, budget - 1)
            b = self.expr(sz + 1, budget - 1)
            return a + b + [word(rnd.choice(("ADD", "SUB", "SUB", "MUL", "MUL")))]
        if x < 0.87:
            return self.expr(sz, budget - 1) + [word("NEG")]
        if x < 0.93:
            return self.expr(sz, budget - 1) + [word("SQR")]
        # shared values under a result: k values, an expression that may PICK them, NIP k
        k = rnd.randrange(1, 3)
        out = []
        for i in range(k):
            out += self.expr(sz + i, budget - 2)
        return out + self.expr(sz + k, budget - 1) + [word("NIP", k)]


def random_program(seed):
    """A valid raw program: terms closed by ACC (some through a closing `* hot[k]`), or values closed by STORE, or — now and
    then — both, the stored values first or last. MUL_HOT also occurs inside terms (fused) and PUSH_HOT as a leaf."""
    rnd = random.Random(seed)
    g = _Gen(rnd)
    kind = rnd.choice(("acc",) * 6 + ("store", "store", "mixed"))
    words, nstore = [], 0
    for t in range(rnd.choice((1, 2, 3, 5, 8, 14, 30))):
        words += g.expr(0, rnd.randrange(1, 6))
        store = kind == "store" or (kind == "mixed" and rnd.random() < 0.3)
        if store:
            words.append(word("STORE", nstore))
            nstore += 1
        else:
            if rnd.random() < 0.4:
                words.append(word("MUL_HOT", rnd.randrange(4)))
            words.append(word("ACC"))
    return words
