"""Circuits at the extreme SHAPES of a constraint system — the counts that are 0 or 1 where every other fixture has a few:
no advice column, no fixed column, no gate, the smallest domain (n = 8, 2 usable rows), ten permutation sets of one
column, eight lookups, a lookup six pairs wide, rotations of n - 1 and n + 1, unqueried columns, tables that are part of
the witness. Written like tests/circuits.py against the package's ConstraintSystem, Circuit and Assembly; every builder
returns a Circuit with a satisfying witness (check_satisfied has accepted it). Nothing here touches a device.

SHAPES: name -> (builder(plonk), the constraint kinds the shape has); REFUSALS: the two shapes no prover accepts."""
import circuits
import witness_check_ref as W

R = circuits.R
Circuit, check_satisfied = circuits.Circuit, circuits.check_satisfied


def _finish(plonk, cs, k):
    c = Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    return c


def square_min_rows(plonk):
    """S1: the square circuit on n = 8: 2 usable rows, 3 permutation columns in 3 sets."""
    c = circuits.square_circuit(plonk, 3)
    check_satisfied(c)
    return c


def perm_only(plonk, k):
    """S2 (and R2 at k = 2): two advice columns tied crosswise at row 0 and the last usable row; nothing else."""
    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    cs.enable_equality(a)
    cs.enable_equality(b)
    c = _finish(plonk, cs, k)
    u = c.usable
    if u < 1:  # R2: no row to assign; keygen refuses the description
        c.instances = []
        return c
    for row in range(u):
        c.advice[a.index][row] = 1000 + row
        c.advice[b.index][row] = 2000 + row
    c.advice[b.index][u - 1] = c.advice[a.index][0]
    c.advice[b.index][0] = c.advice[a.index][u - 1]
    c.copy(a, 0, b, u - 1)
    c.copy(a, u - 1, b, 0)
    c.instances = []
    check_satisfied(c)
    return c


def perm_ten_sets(plonk):
    """S3: nine advice columns and one instance column, all in the permutation and nothing else: degree 3, so one column
    per set, ten sets. Copies at row 0, at the last usable row and to the instance cell."""
    cs = plonk.ConstraintSystem()
    adv = [cs.advice_column() for _ in range(9)]
    inst = cs.instance_column()
    for col in adv + [inst]:
        cs.enable_equality(col)
    c = _finish(plonk, cs, 4)
    u = c.usable
    c.copy(inst, 0, adv[0], 0)
    c.copy(adv[0], 0, adv[8], u - 1)
    c.copy(adv[1], 0, adv[2], u - 1)
    c.copy(adv[3], u - 1, adv[4], u - 1)
    c.copy(adv[5], 3, adv[6], 0)
    c.copy(adv[7], u - 1, adv[7], 0)

    def assign(seed):
        advice = [[(7919 * (seed + 1) + 101 * j + row) % R for row in range(u)] + [0] * (c.n - u) for j in range(9)]
        advice[8][u - 1] = advice[0][0]
        advice[2][u - 1] = advice[1][0]
        advice[4][u - 1] = advice[3][u - 1]
        advice[6][0] = advice[5][3]
        advice[7][0] = advice[7][u - 1]
        return advice, [[advice[0][0]]]

    c.advice, c.instances = assign(0)
    c._witness_fn = assign
    check_satisfied(c)
    return c


def lookup_only(plonk, k):
    """S4: one lookup of an advice column in a fixed column; no gate, no permutation."""
    cs = plonk.ConstraintSystem()
    a, t = cs.advice_column(), cs.fixed_column()
    cs.lookup(lambda m: [(m.query_advice(a, 0), m.query_fixed(t, 0))])
    c = _finish(plonk, cs, k)
    u = c.usable
    for row in range(u):
        c.fixed[t.index][row] = 3 + 5 * row
        c.advice[a.index][row] = 3 + 5 * ((row * 7 + 1) % u)
    c.instances = []
    check_satisfied(c)
    return c


def lookups_eight(plonk):
    """S5: eight lookups of one pair, each with an advice and a table column of its own."""
    cs = plonk.ConstraintSystem()
    pairs = [(cs.advice_column(), cs.fixed_column()) for _ in range(8)]
    for a, t in pairs:
        cs.lookup(lambda m, a=a, t=t: [(m.query_advice(a, 0), m.query_fixed(t, 0))])
    c = _finish(plonk, cs, 4)
    u = c.usable
    for j, (a, t) in enumerate(pairs):
        for row in range(u):
            c.fixed[t.index][row] = 100 * (j + 1) + row % (j + 2)  # j + 2 distinct values: tables with repeats
            c.advice[a.index][row] = 100 * (j + 1) + (row * 3 + j) % (j + 2)
    c.instances = []
    check_satisfied(c)
    return c


def lookup_six_wide(plonk):
    """S6: one lookup of six (input, table) pairs: theta runs to its fifth power."""
    cs = plonk.ConstraintSystem()
    ins = [cs.advice_column() for _ in range(6)]
    tabs = [cs.fixed_column() for _ in range(6)]
    cs.lookup(lambda m: [(m.query_advice(a, 0), m.query_fixed(t, 0)) for a, t in zip(ins, tabs)])
    c = _finish(plonk, cs, 4)
    u = c.usable
    for row in range(u):
        src = (row * 3 + 2) % u
        for j in range(6):
            c.fixed[tabs[j].index][row] = (row + 1) * (j + 1) + (1 << (40 * j)) % R
            c.advice[ins[j].index][row] = (src + 1) * (j + 1) + (1 << (40 * j)) % R
    c.instances = []
    check_satisfied(c)
    return c


def no_advice(plonk):
    """S7: no advice column. Gate s * (inst(0) * inst(+1) - f(0)) over one instance column, the selector and one fixed column."""
    cs = plonk.ConstraintSystem()
    inst, s, f = cs.instance_column(), cs.selector(), cs.fixed_column()
    cs.create_gate(lambda m: [m.query_selector(s) * (m.query_instance(inst, 0) * m.query_instance(inst, 1) - m.query_fixed(f, 0))])
    c = _finish(plonk, cs, 4)
    u = c.usable
    vals = [11 + 3 * row for row in range(u)]
    c.instances[inst.index] = vals
    for row in range(u - 1):
        c.fixed[s.index][row] = 1
        c.fixed[f.index][row] = vals[row] * vals[row + 1] % R
    check_satisfied(c)
    return c


def far_rotation(plonk, r):
    """S8: gate s * (b(0) - a(+r) * a(-r)) at k = 5, enabled on the usable rows whose two rotated rows are usable modulo n;
    a and b are in the permutation (its products are opened at rotation +1) and a is looked up in a fixed table (its
    permuted input is opened at rotation -1): with r = n - 1 and r = n + 1 the gate's rotations name those very points."""
    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    s, t = cs.selector(), cs.fixed_column()
    cs.enable_equality(a)
    cs.enable_equality(b)
    cs.create_gate(lambda m: [m.query_selector(s) * (m.query_advice(b, 0) - m.query_advice(a, r) * m.query_advice(a, -r))])
    cs.lookup(lambda m: [(m.query_advice(a, 0), m.query_fixed(t, 0))])
    c = _finish(plonk, cs, 5)
    n, u = c.n, c.usable
    for row in range(u):
        c.fixed[t.index][row] = 2 + row
        c.advice[a.index][row] = 2 + (row * 5 + 3) % u
        c.advice[b.index][row] = 900 + row
    c.advice[a.index][u - 1] = c.advice[a.index][0]
    c.copy(a, 0, a, u - 1)
    on = [row for row in range(u) if (row + r) % n < u and (row - r) % n < u]
    assert on
    for row in on:
        c.fixed[s.index][row] = 1
        c.advice[b.index][row] = c.advice[a.index][(row + r) % n] * c.advice[a.index][(row - r) % n] % R
    src, dst = on[0], next(row for row in range(1, u) if row not in on)  # a gate output tied to a cell no gate reads
    c.advice[b.index][dst] = c.advice[b.index][src]
    c.copy(b, src, b, dst)
    c.instances = []
    c.gate_rows = on
    check_satisfied(c)
    return c


def unused_columns(plonk):
    """S9: the square gate, its output tied to an instance value, and three columns nothing queries: an advice and a fixed
    column of non-zero values, and a second instance column of exactly `usable` values."""
    cs = plonk.ConstraintSystem()
    a, sq, idle_a = cs.advice_column(), cs.advice_column(), cs.advice_column()
    inst, idle_i = cs.instance_column(), cs.instance_column()
    s, idle_f = cs.selector(), cs.fixed_column()
    for col in (a, sq, inst):
        cs.enable_equality(col)
    cs.create_gate(lambda m: [m.query_selector(s) * (m.query_advice(sq, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))])
    c = _finish(plonk, cs, 4)
    n, u = c.n, c.usable
    for row in range(u):
        c.fixed[s.index][row] = 1 if row % 2 == 0 else 0
        c.fixed[idle_f.index][row] = 5000 + row
    c.copy(inst, 0, sq, 0)
    c.copy(a, 2, a, u - 1)

    def assign(seed):
        advice = [[0] * n for _ in range(3)]
        for row in range(u):
            advice[a.index][row] = 5 + 17 * seed + row
            advice[idle_a.index][row] = 7000 + 13 * seed + row
        advice[a.index][u - 1] = advice[a.index][2]
        for row in range(u):
            advice[sq.index][row] = advice[a.index][row] ** 2 % R if row % 2 == 0 else 31 + row
        return advice, [[advice[sq.index][0]], [900 + 7 * seed + row for row in range(u)]]

    c.advice, c.instances = assign(0)
    c._witness_fn = assign
    check_satisfied(c)
    return c


def tables_interleaved(plonk):
    """S10: three lookups whose tables are an advice column, a fixed column, an advice column: the constant table is not the
    leading one. The third reads its input at rotation +1 and its table at rotation -1. A prover overwrites the rows >= usable
    of every advice column with blinding values, so the third lookup's input carries a selector that is off on the last
    usable row (which reads row `usable`), and its table holds the disabled rows' 0 at a row that the rotated read of a
    usable row reaches (table row 0 reads row n - 1: a blinding value, which matches nothing and need not)."""
    cs = plonk.ConstraintSystem()
    x0, t0, x1, x2, t2 = (cs.advice_column() for _ in range(5))
    f1, q = cs.fixed_column(), cs.selector()
    cs.lookup(lambda m: [(m.query_advice(x0, 0), m.query_advice(t0, 0))])
    cs.lookup(lambda m: [(m.query_advice(x1, 0), m.query_fixed(f1, 0))])
    cs.lookup(lambda m: [(m.query_selector(q) * m.query_advice(x2, 1), m.query_advice(t2, -1))])
    c = _finish(plonk, cs, 4)
    u = c.usable
    for row in range(u):
        c.advice[t0.index][row] = 40 + 2 * row
        c.advice[x0.index][row] = 40 + 2 * ((row * 3 + 1) % u)
        c.fixed[f1.index][row] = 70 + row % 4
        c.advice[x1.index][row] = 70 + (row + 1) % 4
    # table tuples of lookup 2 at rows 1 .. u - 1 are t2[0 .. u - 2]; t2[0] = 0 serves the disabled row
    for row in range(u - 1):
        c.advice[t2.index][row] = 0 if row == 0 else 300 + row
    c.advice[t2.index][u - 1] = 999  # read by no usable row's table tuple
    for row in range(u - 1):  # the input at row reads x2[row + 1]
        c.fixed[q.index][row] = 1
        c.advice[x2.index][row + 1] = c.advice[t2.index][(row * 5 + 2) % (u - 1)]
    c.advice[x2.index][0] = 12345  # read by no input
    c.instances = []
    check_satisfied(c)
    return c


def nothing_constrained(plonk):
    """R1: one advice column and nothing else: h(X) is zero and a piece of it commits to the identity."""
    cs = plonk.ConstraintSystem()
    a = cs.advice_column()
    c = _finish(plonk, cs, 4)
    for row in range(c.usable):
        c.advice[a.index][row] = 1 + row
    c.instances = []
    return c


SHAPES = {
    "square_min_rows": (square_min_rows, {"gate"}),  # its copy cycles are all of length 1
    "perm_only-k3": (lambda plonk: perm_only(plonk, 3), {"copy"}),
    "perm_only-k4": (lambda plonk: perm_only(plonk, 4), {"copy"}),
    "perm_ten_sets": (perm_ten_sets, {"copy"}),
    "lookup_only-k3": (lambda plonk: lookup_only(plonk, 3), {"lookup"}),
    "lookup_only-k4": (lambda plonk: lookup_only(plonk, 4), {"lookup"}),
    "lookups_eight": (lookups_eight, {"lookup"}),
    "lookup_six_wide": (lookup_six_wide, {"lookup"}),
    "no_advice": (no_advice, {"gate"}),
    "far_rotation-11": (lambda plonk: far_rotation(plonk, 11), {"gate", "lookup", "copy"}),
    "far_rotation-31": (lambda plonk: far_rotation(plonk, 31), {"gate", "lookup", "copy"}),
    "far_rotation-33": (lambda plonk: far_rotation(plonk, 33), {"gate", "lookup", "copy"}),
    "unused_columns": (unused_columns, {"gate", "copy"}),
    "tables_interleaved": (tables_interleaved, {"lookup"}),
}
NAMES = list(SHAPES)
REFUSALS = {"nothing_constrained": nothing_constrained, "too_few_rows": lambda plonk: perm_only(plonk, 2)}
_made = {}


def shape(plonk, name):
    """The circuit of SHAPES[name] or REFUSALS[name], built once per process and never modified."""
    if name not in _made:
        _made[name] = (SHAPES[name][0] if name in SHAPES else REFUSALS[name])(plonk)
    return _made[name]


# ------------------------------------------------------------------------------------ one corrupted cell per kind
KIND = {"gate": W.GATE, "lookup": W.LOOKUP, "copy": W.COPY}


def _queries(e, op, out):
    if e[0] == op:
        out.append((e[1], e[2]))
    elif e[0] in ("neg", "scaled"):
        _queries(e[1], op, out)
    elif e[0] in ("sum", "product"):
        _queries(e[1], op, out)
        _queries(e[2], op, out)
    return out


def corrupt(c, way):
    """(advice, instances, reference report) of c's witness with ONE cell changed, as witness_check_cases.corrupt chooses it
    on the larger circuits: 'gate' a cell an enabled gate reads (an instance cell where the circuit has no advice column),
    'lookup' a cell a lookup input reads, set far outside every table, 'copy' an advice cell of a copy cycle of more than
    one cell. The first candidate whose reference report has an entry of the way's kind; an AssertionError if none has."""
    n, u = c.n, c.usable
    cand = []  # (op, column, row, value)
    if way == "gate":
        for g in c.desc["gates"]:
            for op in ("advice", "instance"):
                for col, rot in _queries(g, op, []):
                    cells = c.advice[col] if op == "advice" else list(c.instances[col]) + [0] * n
                    cand += [(op, col, (row + rot) % n, cells[(row + rot) % n] + 1) for row in range(u)]
    elif way == "lookup":
        for lk in c.desc["lookups"]:
            for e in lk["inputs"]:
                for col, rot in _queries(e, "advice", []):
                    cand += [("advice", col, (row + rot) % n, R - 12345 - row) for row in range(u)]
    else:
        cols = W.Walk(c).perm_columns()
        for i, (kind, col) in enumerate(cols):
            if kind == 0:
                cand += [("advice", col, row, c.advice[col][row] + 1) for row in range(n) if tuple(c.assembly.mapping[i][row]) != (i, row)]
    for op, col, row, value in cand:
        adv, inst = [list(a) for a in c.advice], [list(v) for v in c.instances]
        if op == "advice":
            adv[col][row] = value % R
        elif row < len(inst[col]):
            inst[col][row] = value % R
        else:
            continue
        rep = W.report(c, advice=adv, instances=inst)
        if any(e[0] == KIND[way] for e in rep):
            return adv, inst, rep
    raise AssertionError("no cell to corrupt by way of %s" % way)


# ------------------------------------------------------------------------------------ the oracle's keys and proofs
TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
SEED = 5
KINDS = [("blake2b", "shplonk"), ("evm", "gwc")]
_keys, _proofs = {}, {}


def oracle_key(plonk, name):
    """The pure-Python oracle's key of a shape (oracle/ must be on sys.path), made once per process."""
    import plonk_ref as PR

    if name not in _keys:
        c = shape(plonk, name)
        _keys[name] = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    return _keys[name]


def oracle_proof(plonk, name, transcript, multiopen, seed=SEED):
    """The pure-Python oracle's proof of a shape's own witness, made once per process."""
    import plonk_ref as PR

    key = (name, transcript, multiopen, seed)
    if key not in _proofs:
        c = shape(plonk, name)
        _proofs[key] = PR.create_proof(oracle_key(plonk, name), c.instances, c.advice, seed=seed, transcript=transcript, multiopen=multiopen)
    return _proofs[key]


def flipped(proof):
    """The proof with its last byte's lowest bit flipped."""
    return proof[:-1] + bytes([proof[-1] ^ 1])


def wrong_instances(c):
    """c's instances with the first value there is incremented, or None when no column holds a value."""
    bad = [list(v) for v in c.instances]
    for col in bad:
        if col:
            col[0] = (col[0] + 1) % R
            return bad
    return None
