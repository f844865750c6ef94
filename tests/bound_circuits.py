"""Constraint systems whose gate and lookup expressions drive the host compiler (csrc/program.hip emit_tree,
emit_compressed, finalize_limb_program) to each of its decisions, from both sides of each threshold, written against the
product's ConstraintSystem mirror as tests/circuits.py does.

Every gate polynomial is  s * (out - f)  with `out` an advice column of its own, so a satisfying witness exists whatever f
is. emit_tree turns it into  [f] NEG ADD_COL(out) MUL_COL(s)  — or PUSH_COL(out) SUB_COL(f) MUL_COL(s) when f is a column —
and each gate below records, as `expect`, the run-length form of the instructions its term must have in the finalised
h(X) program, derived by walking finalize_limb_program's rules by hand (bounds in units of p: a leaf 1, a product 2, a
sum the sum, a - col three more, -x 3 or 10, the weak reduction 1.01):

  a fused addition reduces first when the sum would pass 40; ADD of two entries likewise; a value above 8 is reduced
  before a push buries it; a product of bounds of 160 or more reduces its top operand; a subtrahend below 2 takes
  NEG / SUB, below 9 NEG_BIG / SUB_BIG, and is reduced first otherwise (a product's bound is exactly 2: NEG_BIG).

tests/test_gpu_bound_gates.py asserts those sequences on the program of the key the device runs, so "the device executed
this decision" is a checked fact."""
import numpy as np

import circuits

R = circuits.R
Circuit = circuits.Circuit


def ev(e, row, fixed, advice, n, challenges=()):
    op = e[0]
    if op == "const":
        return e[1] % R
    if op == "fixed":
        return fixed[e[1]][(row + e[2]) % n]
    if op == "advice":
        return advice[e[1]][(row + e[2]) % n]
    if op == "challenge":
        return challenges[e[1]] % R
    if op == "neg":
        return -ev(e[1], row, fixed, advice, n, challenges) % R
    if op == "sum":
        return (ev(e[1], row, fixed, advice, n, challenges) + ev(e[2], row, fixed, advice, n, challenges)) % R
    if op == "product":
        return ev(e[1], row, fixed, advice, n, challenges) * ev(e[2], row, fixed, advice, n, challenges) % R
    if op == "scaled":
        return ev(e[1], row, fixed, advice, n, challenges) * e[2] % R
    raise ValueError(op)


class Builder:
    """The leaves a gate's f is made of: X(i) is the i-th (free advice column, rotation) pair, cycling."""

    def __init__(self, plonk, cs, m, free, rots, fx):
        self.E, self.cs, self.m, self.free, self.rots, self.fx = plonk.Expression, cs, m, free, rots, fx
        self.at = 0

    def X(self, i=None, rot=None):
        if i is None:
            i, self.at = self.at, self.at + 1
        col = self.free[i % len(self.free)]
        return self.m.query_advice(col, self.rots[(i // len(self.free)) % len(self.rots)] if rot is None else rot)

    def F(self, rot=0):
        return self.m.query_fixed(self.fx, rot)

    def C(self, v):
        return self.E.constant(v)

    def lsum(self, count):
        """((x0 + x1) + x2) + ...: PUSH_COL and count - 1 ADD_COL, bound `count`."""
        e = self.X()
        for _ in range(count - 1):
            e = e + self.X()
        return e

    def csum(self, count):
        """x0 + c + c' + ...: PUSH_COL and count - 1 ADD_CONST."""
        e = self.X()
        for i in range(count - 1):
            e = e + self.C((R - 1, 1, 1 << 253)[i % 3])
        return e


TAIL = " ADD_COL MUL_COL"


def threshold_gates():
    """(name, f(B), expected instructions of the gate's term)."""
    return [
        ("add_col_40", lambda B: B.lsum(40), "PUSH_COL ADD_COL*39 REDUCE NEG" + TAIL),
        ("add_col_41", lambda B: B.lsum(41), "PUSH_COL ADD_COL*39 REDUCE ADD_COL NEG_BIG" + TAIL),
        ("add_const_40", lambda B: B.csum(40), "PUSH_COL ADD_CONST*39 REDUCE NEG" + TAIL),
        ("add_const_41", lambda B: B.csum(41), "PUSH_COL ADD_CONST*39 REDUCE ADD_CONST NEG_BIG" + TAIL),
        ("sub_col_40", lambda B: B.lsum(37) - B.X(), "PUSH_COL ADD_COL*36 SUB_COL REDUCE NEG" + TAIL),
        ("sub_col_41", lambda B: B.lsum(38) - B.X(), "PUSH_COL ADD_COL*37 REDUCE SUB_COL NEG_BIG" + TAIL),
        ("add_8_32", lambda B: B.lsum(8) + B.lsum(32), "PUSH_COL ADD_COL*7 PUSH_COL ADD_COL*31 ADD REDUCE NEG" + TAIL),
        ("add_8_33", lambda B: B.lsum(8) + B.lsum(33), "PUSH_COL ADD_COL*7 PUSH_COL ADD_COL*32 REDUCE ADD REDUCE NEG" + TAIL),
        ("sink_8", lambda B: B.lsum(8) + B.lsum(2), "PUSH_COL ADD_COL*7 PUSH_COL ADD_COL ADD REDUCE NEG" + TAIL),
        ("sink_9", lambda B: B.lsum(9) + B.lsum(2), "PUSH_COL ADD_COL*8 REDUCE PUSH_COL ADD_COL ADD NEG_BIG" + TAIL),
        ("mul_8_19", lambda B: B.lsum(8) * B.lsum(19), "PUSH_COL ADD_COL*7 PUSH_COL ADD_COL*18 MUL NEG_BIG" + TAIL),
        ("mul_8_20", lambda B: B.lsum(8) * B.lsum(20), "PUSH_COL ADD_COL*7 PUSH_COL ADD_COL*19 REDUCE MUL NEG_BIG" + TAIL),
        ("neg_col", lambda B: (-B.X()) * B.X(), "PUSH_COL NEG MUL_COL NEG_BIG" + TAIL),
        ("neg_sum_2", lambda B: B.lsum(2), "PUSH_COL ADD_COL NEG_BIG" + TAIL),
        ("neg_sum_8", lambda B: B.lsum(8), "PUSH_COL ADD_COL*7 NEG_BIG" + TAIL),
        ("neg_sum_9", lambda B: B.lsum(9), "PUSH_COL ADD_COL*8 REDUCE NEG" + TAIL),
        ("inner_neg_sum_8", lambda B: -B.lsum(8) + B.X(), "PUSH_COL ADD_COL*7 NEG_BIG ADD_COL REDUCE NEG" + TAIL),
        ("inner_neg_sum_9", lambda B: -B.lsum(9) + B.X(), "PUSH_COL ADD_COL*8 REDUCE NEG ADD_COL NEG_BIG" + TAIL),
        # rotations at the edge of a k = 5 domain (and of nothing else: -31 = 1, 31 = -1 modulo n)
        ("rot_n_minus_1", lambda B: B.X(0, 31) * B.X(1, -31) + B.X(2, 0), "PUSH_COL MUL_COL ADD_COL NEG_BIG" + TAIL),
    ]


def branch_gates():
    """Every fusion branch of emit_tree, for ADD and for MUL."""
    c5, c7 = 5, R - 7
    return [
        ("f_is_a_column", lambda B: B.X(), "PUSH_COL SUB_COL MUL_COL"),
        ("add_col_col", lambda B: B.X() + B.X(), "PUSH_COL ADD_COL NEG_BIG" + TAIL),
        ("mul_col_col", lambda B: B.X() * B.X(), "PUSH_COL MUL_COL NEG_BIG" + TAIL),
        ("add_col_fixed", lambda B: B.X() + B.F(1), "PUSH_COL ADD_COL NEG_BIG" + TAIL),
        ("add_col_const", lambda B: B.X() + B.C(c5), "PUSH_COL ADD_CONST NEG_BIG" + TAIL),
        ("mul_col_const", lambda B: B.X() * B.C(c7), "PUSH_COL MUL_CONST NEG_BIG" + TAIL),
        ("add_const_col", lambda B: B.C(c7) + B.X(), "PUSH_CONST ADD_COL NEG_BIG" + TAIL),
        ("mul_const_col", lambda B: B.C(c5) * B.X(), "PUSH_CONST MUL_COL NEG_BIG" + TAIL),
        ("add_const_const", lambda B: B.C(c5) + B.C(c7), "PUSH_CONST ADD_CONST NEG_BIG" + TAIL),
        ("mul_const_const", lambda B: B.C(c5) * B.C(c7), "PUSH_CONST MUL_CONST NEG_BIG" + TAIL),
        ("add_leaf_subtree", lambda B: B.X() + B.X() * B.X(), "PUSH_COL MUL_COL ADD_COL NEG_BIG" + TAIL),
        ("mul_leaf_subtree", lambda B: B.X() * (B.X() + B.X()), "PUSH_COL ADD_COL MUL_COL NEG_BIG" + TAIL),
        ("add_const_subtree", lambda B: B.C(c7) + B.X() * B.X(), "PUSH_COL MUL_COL ADD_CONST NEG_BIG" + TAIL),
        ("mul_const_subtree", lambda B: B.C(c7) * (B.X() + B.X()), "PUSH_COL ADD_COL MUL_CONST NEG_BIG" + TAIL),
        ("add_subtree_leaf", lambda B: B.X() * B.X() + B.X(), "PUSH_COL MUL_COL ADD_COL NEG_BIG" + TAIL),
        ("mul_subtree_leaf", lambda B: (B.X() + B.X()) * B.X(), "PUSH_COL ADD_COL MUL_COL NEG_BIG" + TAIL),
        ("add_subtree_const", lambda B: B.X() * B.X() + B.C(c5), "PUSH_COL MUL_COL ADD_CONST NEG_BIG" + TAIL),
        ("mul_subtree_const", lambda B: (B.X() + B.X()) * B.C(c5), "PUSH_COL ADD_COL MUL_CONST NEG_BIG" + TAIL),
        ("add_subtree_subtree", lambda B: B.X() * B.X() + B.X() * B.X(), "PUSH_COL MUL_COL PUSH_COL MUL_COL ADD NEG_BIG" + TAIL),
        ("mul_subtree_subtree", lambda B: (B.X() + B.X()) * (B.X() + B.X()), "PUSH_COL ADD_COL PUSH_COL ADD_COL MUL NEG_BIG" + TAIL),
        ("leaf_minus_col", lambda B: B.X() - B.X(), "PUSH_COL SUB_COL NEG_BIG" + TAIL),
        ("const_minus_col", lambda B: B.C(c5) - B.X(), "PUSH_CONST SUB_COL NEG_BIG" + TAIL),
        ("subtree_minus_col", lambda B: B.X() * B.X() - B.X(), "PUSH_COL MUL_COL SUB_COL NEG_BIG" + TAIL),
        ("neg_col_plus_col", lambda B: (-B.X()) + B.X(), "PUSH_COL NEG ADD_COL NEG_BIG" + TAIL),
        ("neg_col_plus_subtree", lambda B: (-B.X()) + B.X() * B.X(), "PUSH_COL NEG PUSH_COL MUL_COL ADD NEG_BIG" + TAIL),
        ("col_times_neg_col", lambda B: B.X() * (-B.X()), "PUSH_COL NEG MUL_COL NEG_BIG" + TAIL),
        ("scale_leaf", lambda B: B.X() * 7, "PUSH_COL MUL_CONST NEG_BIG" + TAIL),
        ("scale_subtree", lambda B: (B.X() + B.X()) * (R - 1), "PUSH_COL ADD_COL MUL_CONST NEG_BIG" + TAIL),
        ("neg_neg", lambda B: -B.X(), "PUSH_COL NEG NEG_BIG" + TAIL),
        ("neg_neg_neg", lambda B: -(-B.X()), "PUSH_COL NEG NEG_BIG REDUCE NEG" + TAIL),
        ("neg_of_subtree_in_a_sum", lambda B: B.X() * B.X() + (-(B.X() + B.X())), "PUSH_COL MUL_COL PUSH_COL ADD_COL NEG_BIG ADD REDUCE NEG" + TAIL),
    ]


def rotation_gates():
    """k = 7: the rotations at the ends of the 8-bit encoding, -128 and 127, and +-(n - 1), beside 0 and +-1."""
    return [
        ("rot_edges", lambda B: B.X(0, -128) * B.X(1, 127) + B.X(2, -127) + B.X(0, 127), "PUSH_COL MUL_COL ADD_COL*2 NEG_BIG" + TAIL),
        ("rot_near", lambda B: B.X(1, 1) * B.X(2, -1) + B.X(3, 0) - B.X(3, 1), "PUSH_COL MUL_COL ADD_COL SUB_COL NEG_BIG" + TAIL),
        ("rot_fixed", lambda B: B.F(-128) * B.X(3, -1) + B.F(127), "PUSH_COL MUL_COL ADD_COL NEG_BIG" + TAIL),
    ]


def long_sum_gates():
    """A left-nested sum of 300 leaves: REDUCE before the 41st and then every 39 addends (1.01 + 39 = 40.01 passes 40)."""
    seq = "PUSH_COL ADD_COL*39" + " REDUCE ADD_COL*38" * 6 + " REDUCE ADD_COL*32"
    assert 40 + 38 * 6 + 32 == 300
    return [("long_sum_300", lambda B: B.lsum(300), seq + " REDUCE NEG" + TAIL)]


def deep_gates(levels):
    """(x*y) + ((x*y) + (... + (x*y))): emit_tree keeps the operands' order, so all `levels` products are pushed before the
    first ADD — a stack of `levels` entries in both interpreters."""
    def f(B):
        terms = [B.X() * B.X() for _ in range(levels)]
        e = terms[-1]
        for t in reversed(terms[:-1]):
            e = t + e
        return e
    return [("deep_%d" % levels, f, None)]


def deep_gate_circuit(plonk, k, levels):
    return gate_circuit(plonk, k, deep_gates(levels), seed=7)


def gate_circuit(plonk, k, gates, seed=1, pad_fixed=0, repeat=1, lookups=None, rots=(0, 1, -1), extreme_fixed=None):
    """A circuit of the gates above. pad_fixed: every polynomial gets that many `+ z` behind it, z a fixed column of zeros
    (ADD_COL each: a term whose bound is 2 + pad_fixed instead of a product's 2). repeat: the list of polynomials is
    repeated (a copy is the same polynomial but for the rotations of its padding). lookups(cs, B-maker) may add lookups and returns their assignment.
    extreme_fixed: every fixed column holds this field element on every row — it is then the constant polynomial, and the
    key is for quotient evaluations on arbitrary polynomials only (no witness satisfies it)."""
    rnd = np.random.RandomState(100 + seed)
    cs = plonk.ConstraintSystem()
    free = [cs.advice_column() for _ in range(4)]
    fx, zero, sel = cs.fixed_column(), cs.fixed_column(), cs.selector()
    outs = [cs.advice_column() for _ in gates]
    for col in (free[0], free[1], outs[0], fx):
        cs.enable_equality(col)
    defs = []

    def make(m):
        polys = []
        for rep in range(repeat):
            for (name, f, _), out in zip(gates, outs):
                B = Builder(plonk, cs, m, free, rots, fx)
                fe = f(B)
                if rep == 0:
                    defs.append((out, fe.to_tuple()))
                p = m.query_selector(sel) * (m.query_advice(out, 0) - fe)
                for i in range(pad_fixed):
                    p = p + m.query_fixed(zero, (0, 1, -1)[(i + rep) % 3])
                polys.append(p)
        return polys

    cs.create_gate(make)
    assign_lookups = lookups(plonk, cs) if lookups else None
    c = Circuit(cs, k)
    c.gate_names = [g[0] for g in gates] * repeat
    pad = "" if not pad_fixed else " ADD_COL" if pad_fixed == 1 else " ADD_COL*%d" % pad_fixed
    c.gate_expect = [None if g[2] is None else g[2] + pad for g in gates] * repeat
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    n, u = c.n, c.usable
    all_rots = sorted({r for _, r in cs.advice_queries} | {r for _, r in cs.fixed_queries})
    rows = [row for row in range(u) if all(0 <= (row + r) % n < u for r in all_rots)]
    assert len(rows) >= 8
    for row in range(u):
        c.fixed[fx.index][row] = int(rnd.randint(0, 1 << 30)) if row % 3 else R - 1 - row
    for row in rows:
        c.fixed[sel.index][row] = 1
    for col in free:
        for row in range(u):
            c.advice[col.index][row] = int(rnd.randint(0, 1 << 62)) * int(rnd.randint(1, 1 << 62)) % R if row % 4 else R - 1 - row
    # copies between free cells (made equal here) and from a fixed cell
    c.advice[free[0].index][5] = c.advice[free[0].index][2]
    c.copy(free[0], 2, free[0], 5)
    c.advice[free[1].index][3] = c.advice[free[0].index][2]
    c.copy(free[0], 2, free[1], 3)
    c.advice[free[1].index][7] = c.fixed[fx.index][4]
    c.copy(fx, 4, free[1], 7)
    if assign_lookups:
        assign_lookups(c, rnd)
    for out, f in defs:
        for row in range(u):
            c.advice[out.index][row] = ev(f, row, c.fixed, c.advice, n) if row in rows else int(rnd.randint(0, 1 << 30))
    c.out_columns = [o.index for o in outs]
    c.gate_rows = rows
    c.instances = []
    if extreme_fixed is None:
        circuits.check_satisfied(c)
    else:
        c.fixed = [[extreme_fixed % R] * n for _ in c.fixed]
    return c


def seven_lookups(plonk, cs):
    """Seven lookups of one, two and three columns whose input and table expressions reach the lookup term of h(X) with
    bounds 1, 2, 8, 9 and 12 (the term multiplies them, so its OP_SUB always meets a product: SUB_BIG), their `* theta`
    folds, constant tables that are expressions, a negated and a scaled component. With the permutation's terms they put
    15 terms into the l_0 group and 15 or more into the l_active group: two sixth-term carries inside each."""
    a, b = cs.advice_column(), cs.advice_column()
    t1, t2, t3, z = cs.fixed_column(), cs.fixed_column(), cs.fixed_column(), cs.fixed_column()
    E = plonk.Expression

    def S(m, count):
        e = m.query_advice(a, 0)
        for i in range(count - 1):
            e = e + m.query_advice(b if i % 2 == 0 else a, 0)
        return e

    def T(m, col, pad):
        e = m.query_fixed(col, 0)
        for _ in range(pad):
            e = e + m.query_fixed(z, 0)
        return e

    cs.lookup(lambda m: [(m.query_advice(a, 0), m.query_fixed(t1, 0))])
    cs.lookup(lambda m: [(S(m, 7), T(m, t1, 6))])
    cs.lookup(lambda m: [(S(m, 9), T(m, t1, 8))])
    cs.lookup(lambda m: [(S(m, 2), T(m, t1, 0)), (S(m, 2) * 2, m.query_fixed(t2, 0))])
    cs.lookup(lambda m: [(S(m, 8), T(m, t1, 7)), (S(m, 8) * 2, T(m, t2, 1)), (-S(m, 8), m.query_fixed(t3, 0))])
    cs.lookup(lambda m: [(S(m, 12), T(m, t1, 11)), (S(m, 6) + S(m, 6), T(m, t1, 2)), ((-S(m, 6)) * 2, T(m, t3, 3))])  # S(12) = 2 S(6)
    cs.lookup(lambda m: [(m.query_advice(a, 0) * 3 + E.constant(0), m.query_fixed(t1, 0) * 3)])

    def assign(c, rnd):
        for row in range(c.usable):
            c.fixed[t1.index][row], c.fixed[t2.index][row], c.fixed[t3.index][row] = row, 2 * row, -row % R
            c.advice[a.index][row], c.advice[b.index][row] = int(rnd.randint(0, 2)), int(rnd.randint(0, 2))
        assert c.usable > 12
    return assign


def phased_circuit(plonk, k=5, seed=1):
    """A challenge as an operand of every fusion branch that takes a constant: gates q * (out - f) with out in phase 1."""
    import phased_circuits as PC

    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    E = plonk.Expression
    gates = [
        ("chal_plus_col", lambda m, ch: E.challenge(ch) + m.query_advice(a, 0), "PUSH_CONST ADD_COL NEG_BIG" + TAIL),
        ("col_plus_chal", lambda m, ch: m.query_advice(a, 1) + E.challenge(ch), "PUSH_COL ADD_CONST NEG_BIG" + TAIL),
        ("chal_times_col", lambda m, ch: E.challenge(ch) * m.query_advice(b, 0), "PUSH_CONST MUL_COL NEG_BIG" + TAIL),
        ("col_times_chal", lambda m, ch: m.query_advice(b, -1) * E.challenge(ch), "PUSH_COL MUL_CONST NEG_BIG" + TAIL),
        ("chal_plus_chal", lambda m, ch: E.challenge(ch) + E.challenge(ch), "PUSH_CONST ADD_CONST NEG_BIG" + TAIL),
        ("chal_times_chal", lambda m, ch: E.challenge(ch) * E.challenge(ch), "PUSH_CONST MUL_CONST NEG_BIG" + TAIL),
        ("chal_plus_subtree", lambda m, ch: E.challenge(ch) + m.query_advice(a, 0) * m.query_advice(b, 0), "PUSH_COL MUL_COL ADD_CONST NEG_BIG" + TAIL),
        ("subtree_times_chal", lambda m, ch: (m.query_advice(a, 0) + m.query_advice(b, 0)) * E.challenge(ch), "PUSH_COL ADD_COL MUL_CONST NEG_BIG" + TAIL),
        ("chal_minus_col", lambda m, ch: E.challenge(ch) - m.query_advice(a, 0), "PUSH_CONST SUB_COL NEG_BIG" + TAIL),
        ("neg_chal", lambda m, ch: (-E.challenge(ch)) + m.query_advice(b, 0), "PUSH_CONST NEG ADD_COL NEG_BIG" + TAIL),
    ]
    outs = [cs.advice_column_in(1) for _ in gates]
    ch = cs.challenge_usable_after(0)
    q = cs.selector()
    cs.enable_equality(a)
    cs.enable_equality(outs[0])
    defs = []

    def make(m):
        polys = []
        for (name, f, _), out in zip(gates, outs):
            fe = f(m, ch)
            defs.append((out, fe.to_tuple()))
            polys.append(m.query_selector(q) * (m.query_advice(out, 0) - fe))
        return polys

    cs.create_gate(make)
    c = PC.PhasedCircuit(cs, k)
    c.gate_names, c.gate_expect = [g[0] for g in gates], [g[2] for g in gates]
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    n, u = c.n, c.usable
    rows = list(range(1, u - 1))
    for row in rows:
        c.fixed[q.index][row] = 1
    c.copy(a, 2, a, 6)
    c.copy(outs[0], 2, outs[0], 6)

    def fill(phase, chal, advice):
        if phase != 1:
            return
        for out, f in defs:
            for row in rows:
                advice[out.index][row] = ev(f, row, c.fixed, advice, n, [chal[ch.index]])

    def assign(seed_):
        rnd = np.random.RandomState(500 + seed_)
        adv = [[0] * n for _ in range(cs.num_advice)]
        for col in (a, b):
            for row in range(u):
                adv[col.index][row] = int(rnd.randint(0, 1 << 62)) * int(rnd.randint(1, 1 << 62)) % R
        adv[a.index][6] = adv[a.index][2]  # ... and with it rows 2 and 6 of outs[0] = ch + a
        return adv, fill

    c.advice, c.fill = assign(seed)
    c.witness_for = assign
    c.instances = []
    return c


def deep_lookup_circuit(plonk, k, levels):
    """One lookup whose input is the right-nested sum of `levels` products a * b (a, b in {0, 1}) against the table {0, levels}:
    `levels` stack entries in the Lagrange-domain compression program, and levels + 2 in h(X), where the lookup term holds
    two values below its compressed input."""
    def lookups(plonk_, cs):
        a, b = cs.advice_column(), cs.advice_column()
        t = cs.fixed_column()

        def inp(m):
            terms = [m.query_advice(a, 0) * m.query_advice(b, 0) for _ in range(levels)]
            e = terms[-1]
            for x in reversed(terms[:-1]):
                e = x + e
            return e

        cs.lookup(lambda m: [(inp(m), m.query_fixed(t, 0))])

        def assign(c, rnd):
            for row in range(c.usable):
                c.fixed[t.index][row] = levels if row % 2 else 0  # every term is the same a * b: the sum is 0 or `levels`
                c.advice[a.index][row], c.advice[b.index][row] = int(rnd.randint(0, 2)), int(row % 2)
        return assign
    return gate_circuit(plonk, k, branch_gates()[:2], lookups=lookups)


CIRCUITS = {
    # name: (maker(plonk, **kw), keygen environment)
    "thresholds": lambda plonk, **kw: gate_circuit(plonk, 5, threshold_gates(), seed=1, **kw),
    "branches": lambda plonk, **kw: gate_circuit(plonk, 5, branch_gates(), seed=2, **kw),
    "rotations7": lambda plonk, **kw: gate_circuit(plonk, 7, rotation_gates(), seed=3, rots=(0,), **kw),
    "lookups7": lambda plonk, **kw: gate_circuit(plonk, 5, branch_gates()[:3], seed=4, lookups=seven_lookups, **kw),
    "many150": lambda plonk, **kw: gate_circuit(plonk, 5, threshold_gates()[10:15], seed=5, pad_fixed=38, repeat=30, **kw),
    "long_sum": lambda plonk, **kw: gate_circuit(plonk, 5, long_sum_gates(), seed=6, **kw),
}
