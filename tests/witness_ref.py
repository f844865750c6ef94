"""The reference for witness programs (include/amdzk.h "witness programs"): an interpreter over Python integers written from
the op table of the header — not from csrc/witness.hpp —, the longest-path depth, and restatements of the documented fusing
rule and workspace formula. A program here is anything with `.nodes` (tuples (op, a, b, c)), `.constants` (integers),
`.cells` ((node, column, row)) and `.publics`: the package's WitnessProgram is one. Every comparison against this file is
exact equality of canonical values."""
import numpy as np

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
RINV = pow(1 << 256, -1, R)
(INPUT, CONST, ADD, SUB, MUL, NEG, INV, SELECT, IS_ZERO, EQ, LT, BITS, AND, XOR) = range(14)
OP_NAMES = "INPUT CONST ADD SUB MUL NEG INV SELECT IS_ZERO EQ LT BITS AND XOR".split()
ARITY = {INPUT: 0, CONST: 0, ADD: 2, SUB: 2, MUL: 2, NEG: 1, INV: 1, SELECT: 3, IS_ZERO: 1, EQ: 2, LT: 2, BITS: 1, AND: 2, XOR: 2}


def node_value(op, a, b, c, v, inputs, constants):
    """The header's table, row by row. v: the values of the earlier nodes; a, b, c: the node's fields."""
    if op == INPUT:
        return inputs[a] % R
    if op == CONST:
        return constants[a] % R
    if op == ADD:
        return (v[a] + v[b]) % R
    if op == SUB:
        return (v[a] - v[b]) % R
    if op == MUL:
        return v[a] * v[b] % R
    if op == NEG:
        return -v[a] % R
    if op == INV:
        return pow(v[a], R - 2, R)  # 0 for 0
    if op == SELECT:
        return v[b] if v[a] != 0 else v[c]
    if op == IS_ZERO:
        return int(v[a] == 0)
    if op == EQ:
        return int(v[a] == v[b])
    if op == LT:
        return int(v[a] < v[b])
    if op == BITS:
        return (v[a] >> b) % (1 << c)
    if op == AND:
        return v[a] & v[b]
    if op == XOR:
        return (v[a] ^ v[b]) % R
    raise ValueError("unknown op %r" % (op,))


def evaluate(prog, inputs):
    """The canonical value of every node for one proof. inputs: integers."""
    v = []
    for op, a, b, c in prog.nodes:
        v.append(node_value(op, a, b, c, v, inputs, prog.constants))
    return v


def node_levels(nodes):
    """level[i]: 0 for INPUT and CONST, else one more than the highest operand's (the longest path down to an input)."""
    lv = []
    for op, a, b, c in nodes:
        ops = (a, b, c)[:ARITY[op]]
        lv.append(1 + max(lv[o] for o in ops) if ops else 0)
    return lv


def level_widths(nodes):
    lv = node_levels(nodes)
    w = [0] * (max(lv) + 1 if lv else 0)
    for x in lv:
        w[x] += 1
    return w


def run_cut(n_proofs, fit):
    """The fewest equal runs: R runs of P = ceil(n / R) proofs when at most `fit` proofs go into one run."""
    runs = -(-n_proofs // fit)
    per = -(-n_proofs // runs)
    return [min(per, n_proofs - i) for i in range(0, n_proofs, per)]


def launches(prog, run_sizes, fused_width):
    """The documented rule: per run of P proofs, every level wider than fused_width items (nodes x P) is a launch, every
    maximal stretch of consecutive levels of at most fused_width items is one; plus the scatter and the gather."""
    widths = level_widths(prog.nodes)
    total = 0
    for P in run_sizes:
        in_stretch = False
        for w in widths:
            if w * P > fused_width:
                total += 1
                in_stretch = False
            elif not in_stretch:
                total += 1
                in_stretch = True
        total += (1 if prog.cells else 0) + (1 if prog.publics else 0)
    return total


def scratch_bytes(prog, per_run):
    return (len(prog.nodes) + len(prog.publics)) * per_run * 32 + 256


# ---- Montgomery words <-> integers (R = 2^256), without the oracle library
def to_words(values):
    """integers -> (n, 4) uint64 Montgomery words"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, x in enumerate(values):
        m = (x % R) * (1 << 256) % R
        for j in range(4):
            out[i, j] = (m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def raw_words(values):
    """integers < 2^256 as they are -> (n, 4) uint64 (for words that are NOT below the modulus)"""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, x in enumerate(values):
        for j in range(4):
            out[i, j] = (x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_words(arr):
    """(..., 4) uint64 Montgomery words -> flat list of canonical integers; words >= r are a failure of the producer"""
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4)
    out = []
    for row in a:
        m = sum(int(row[j]) << (64 * j) for j in range(4))
        assert m < R, "a value that is not below the modulus"
        out.append(m * RINV % R)
    return out
