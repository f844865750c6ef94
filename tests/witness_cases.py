"""Programs and operands shared by the witness-program tests (tests/test_witness_*.py, tests/test_gpu_witness.py). Values
come from tests/witness_ref.py; nothing here calls the library except through the builder class it is handed."""
import random

import witness_ref as WR

R = WR.R
# the operands every op is exercised on: the ends of the field, and values around the word boundaries of both limb widths
EDGE = [0, 1, 2, R - 1, R - 2] + [(1 << 32) * j + d for j in (1, 2, 0xFFFFFFFF, 1 << 190) for d in (-1, 1)] + \
       [(1 << 64) * j + d for j in (1, 3, (1 << 64) - 1, 1 << 128, 1 << 189) for d in (-1, 1)]
EDGE = [v % R for v in EDGE]
BITS_EDGES = [(0, 1), (253, 1), (255, 1), (0, 254), (0, 256), (31, 2), (63, 2), (64, 64), (127, 129)]


def draw_operand(rng):
    return rng.choice(EDGE) if rng.random() < 0.7 else rng.randrange(R)


def random_program(W, rng, n_nodes, n_inputs=6, k=4, num_advice=3, ops=None, near=0.5, n_consts=4, recent=0.0):
    """A random DAG over all ops: n_inputs inputs and a few edge constants first, then n_nodes nodes whose operands are drawn
    with probability `near` from the leaves (so that the ops see the edge operands themselves), with probability `recent` from
    the last four nodes (deep programs), else from anywhere earlier."""
    p = W(k, num_advice)
    leaves = [p.input() for _ in range(n_inputs)] + [p.const(rng.choice(EDGE)) for _ in range(n_consts)]
    ops = ops or list(range(WR.ADD, WR.XOR + 1))
    for _ in range(n_nodes):
        op = rng.choice(ops)
        n = len(p.nodes)

        def pick():
            u = rng.random()
            return rng.choice(leaves) if u < near else rng.randrange(max(0, n - 4), n) if u < near + recent else rng.randrange(n)
        if op == WR.BITS:
            lo, ln = rng.choice(BITS_EDGES) if rng.random() < 0.5 else (lambda lo: (lo, rng.randint(1, 256 - lo)))(rng.randrange(256))
            p.bits(pick(), lo, ln)
        elif op == WR.SELECT:
            p.select(pick(), pick(), pick())
        elif WR.ARITY[op] == 1:
            {WR.NEG: p.neg, WR.INV: p.inv, WR.IS_ZERO: p.is_zero}[op](pick())
        else:
            {WR.ADD: p.add, WR.SUB: p.sub, WR.MUL: p.mul, WR.EQ: p.eq, WR.LT: p.lt, WR.AND: p.and_, WR.XOR: p.xor}[op](pick(), pick())
    return p


def random_inputs(rng, n_proofs, n_inputs):
    return [[draw_operand(rng) for _ in range(n_inputs)] for _ in range(n_proofs)]


def edge_program(W):
    """The op edges (BITS at the word and field boundaries, XOR past r, AND / XOR / LT / INV / SELECT / SUB / NEG at 0, 1, r - 1), one node each, over TWO inputs a, b (so that a batch over pairs of edge operands
    covers them) and the constants the edges name. Returns (program, input pairs)."""
    p = W(4, 2)
    a, b = p.input(), p.input()
    zero, one, rm1 = p.const(0), p.const(1), p.const(R - 1)
    for lo, ln in BITS_EDGES:
        p.bits(a, lo, ln)
        p.bits(rm1, lo, ln)
    p.xor(rm1, one)  # = r -> 0
    for x in (a, b):
        for c in (zero, rm1):
            p.and_(x, c), p.xor(x, c), p.and_(c, x), p.xor(c, x)
    p.and_(a, b), p.xor(a, b)
    p.lt(rm1, zero), p.lt(zero, rm1), p.lt(a, a), p.lt(a, b), p.lt(b, a), p.eq(a, b), p.eq(a, a)
    p.inv(zero), p.inv(one), p.inv(rm1), p.inv(a)
    for c in (zero, one, rm1, a):
        p.select(c, a, b)
    p.sub(zero, one), p.neg(zero), p.neg(a), p.is_zero(a), p.is_zero(zero), p.sub(a, b), p.add(a, b), p.mul(a, b)
    top, bottom = 1 << 224, 1  # operands that differ only in the top word / only in the bottom word
    base = 0x0123456789ABCDEF0123456789ABCDEF0123456789ABCDEF01234567
    pairs = [(x, y) for x in EDGE[:9] for y in EDGE[:9]] + [(base, base + top), (base + top, base), (base, base + bottom), (base + bottom, base),
                                                           (base, base)]
    return p, pairs


def chain_program(W, depth, width=1, k=4, num_advice=2):
    """`depth` levels of `width` nodes each: alternating MUL and ADD of the previous level with an input."""
    p = W(k, num_advice)
    x, y = p.input(), p.input()
    prev = [p.add(x, p.const(j + 1)) for j in range(width)]
    for d in range(depth - 1):
        prev = [(p.mul if d % 2 == 0 else p.add)(prev[j], y if j % 2 == 0 else prev[(j + 1) % width]) for j in range(width)]
    return p


def widths_program(W, widths, k=4, num_advice=2):
    """One level per entry of `widths` (after the leaves), level i of widths[i] nodes, each over one node of the level before
    (so the level is exact) and one node from anywhere earlier — 1, 2 and many levels back."""
    p = W(k, num_advice)
    x, y = p.input(), p.input()
    levels = [[x, y]]
    rng = random.Random(len(widths) * 1000 + sum(widths))
    for i, w in enumerate(widths):
        prev = levels[-1]
        cur = []
        for j in range(w):
            far = rng.choice(levels[rng.randrange(len(levels))])
            op = (p.mul, p.add, p.sub, p.xor)[(i + j) % 4]
            cur.append(op(prev[j % len(prev)], far))
        levels.append(cur)
    # a node whose operands sit 1, 2 and many levels back
    if len(levels) >= 4:
        p.select(levels[-1][0], levels[-2][0], levels[1][0])
    return p


def expose_all(p):
    for i in range(len(p.nodes)):
        p.expose(i)
    return p
