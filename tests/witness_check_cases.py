"""Witnesses that do NOT satisfy their circuit, for the tests of the witness check: one corrupted advice cell per case,
chosen on the CPU with the reference (tests/witness_check_ref.py) only, and two hand-made fixtures for the row and lookup
edge cases. Nothing here touches a device."""
import numpy as np

import circuits
import witness_check_ref as W

R = circuits.R
RANDOM_SEEDS = list(range(53))  # circuits.random_circuit(k = 6): the satisfied fixtures and the circuits that get corrupted
WAYS = ("gate", "lookup", "copy")
# The circuits of RANDOM_SEEDS that HAVE a cell to corrupt each way (every one has a gate; some have no lookup, or no copy
# cycle of length >= 3 across column kinds) — found once on the CPU with corrupt() below and written down, so that every
# case named here exists: a test fails, and skips nothing, if corrupt() finds none.
WAY_SEEDS = {
    "gate": RANDOM_SEEDS,
    "lookup": [1, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 17, 18, 19, 20, 21, 23, 25, 27, 28, 29, 30, 31, 32, 33, 34, 35, 37, 38, 39, 41, 42, 43,
               44, 45, 48, 49, 50, 51],
    "copy": [2, 7, 9, 17, 20, 21, 23, 24, 27, 38, 46, 47, 48, 49, 50, 51, 52],
}
CORRUPTED_CASES = [(seed, way) for way in WAYS for seed in WAY_SEEDS[way]]
_cache = {}


def random_circuit(plonk, seed):
    if seed not in _cache:
        _cache[seed] = circuits.random_circuit(plonk, 6, seed=seed)
    return _cache[seed]


def with_cell(c, col, row, value):
    adv = [list(a) for a in c.advice]
    adv[col][row] = value % R
    return adv


def advice_queries(e, out):
    if e[0] == "advice":
        out.append((e[1], e[2]))
    elif e[0] in ("neg", "scaled"):
        advice_queries(e[1], out)
    elif e[0] in ("sum", "product"):
        advice_queries(e[1], out)
        advice_queries(e[2], out)
    return out


def _first_that_reports(c, kind, candidates):
    """The first candidate (col, row, value) whose corrupted witness has an entry of `kind` in the reference's report."""
    for col, row, value in candidates:
        adv = with_cell(c, col, row, value)
        rep = W.report(c, advice=adv)
        if any(e[0] == kind for e in rep):
            return adv, rep
    return None


def corrupt(c, way):
    """(advice, reference report) of c's witness with one advice cell changed, or None when the circuit has no such cell:
    'gate'   a cell that an enabled gate reads (a query of a gate polynomial, at a row where the polynomial then fails);
    'lookup' a cell a lookup input reads, set to a value far outside every table;
    'copy'   an advice cell of a copy cycle of length >= 3 whose cells lie in columns of more than one kind."""
    n, u = c.n, c.usable
    if way == "gate":
        cand = []
        for g in c.desc["gates"]:
            for col, rot in advice_queries(g, []):
                cand += [(col, (row + rot) % n, c.advice[col][(row + rot) % n] + 1) for row in (5, u // 2, u - 4)]
        return _first_that_reports(c, W.GATE, cand)
    if way == "lookup":
        cand = []
        for lk in c.desc["lookups"]:
            for e in lk["inputs"]:
                for col, rot in advice_queries(e, []):
                    cand += [(col, (row + rot) % n, R - 12345 - row) for row in range(0, u, 3)]
        return _first_that_reports(c, W.LOOKUP, cand)
    cols = W.Walk(c).perm_columns()
    seen = set()
    for i in range(len(cols)):
        for j in range(n):
            if (i, j) in seen:
                continue
            cyc, cell = [], (i, j)
            while cell not in seen:
                seen.add(cell)
                cyc.append(cell)
                cell = tuple(c.assembly.mapping[cell[0]][cell[1]])
            if len(cyc) >= 3 and len({cols[ci][0] for ci, _ in cyc}) >= 2:
                adv_cells = [(cols[ci][1], cj) for ci, cj in cyc if cols[ci][0] == 0]
                if adv_cells:
                    col, row = adv_cells[0]
                    got = _first_that_reports(c, W.COPY, [(col, row, c.advice[col][row] + 1)])
                    if got:
                        return got
    return None


def tallies(plonk):
    """Per way of corrupting: (cases, reference entries of the way's own kind over those cases). A case without a cell to
    corrupt is an error here, not a smaller count."""
    out = {}
    kind = {"gate": W.GATE, "lookup": W.LOOKUP, "copy": W.COPY}
    for w in WAYS:
        reps = [corrupt(random_circuit(plonk, s), w) for s in WAY_SEEDS[w]]
        assert all(r is not None for r in reps), (w, [s for s, r in zip(WAY_SEEDS[w], reps) if r is None])
        out[w] = (len(reps), sum(1 for r in reps for e in r[1] if e[0] == kind[w]))
    return out


def edge_circuit(plonk, k, seed=0):
    """One gate q * (b - (a(-1) + a(+1))) on every usable row: at row 0 it reads row n - 1, at row u - 1 row u. The rows
    >= u hold non-zero junk in a and b, and q is ON there with b wrong: the gate is violated at every row >= u and at no
    usable row. A third column d is tied to a by copy constraints that reach row 127 (and row 128 where it exists): the
    rows on both sides of a 128-row boundary, of which row 127 is not usable at k = 7 and still checked for copies."""
    rnd = np.random.RandomState(300 + seed)
    cs = plonk.ConstraintSystem()
    a, b, d = cs.advice_column(), cs.advice_column(), cs.advice_column()
    q = cs.selector()
    cs.enable_equality(a)
    cs.enable_equality(d)
    cs.create_gate(lambda m: [m.query_selector(q) * (m.query_advice(b, 0) - (m.query_advice(a, -1) + m.query_advice(a, 1)))])
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    n, u = c.n, c.usable
    for row in range(n):
        c.fixed[q.index][row] = 1
        c.advice[a.index][row] = int(rnd.randint(1, 1 << 62))
        c.advice[d.index][row] = int(rnd.randint(1, 1 << 62))
    for row in range(n):
        c.advice[b.index][row] = (c.advice[a.index][(row - 1) % n] + c.advice[a.index][(row + 1) % n] + (1 if row >= u else 0)) % R
    for src, dst in ((3, 127), (4, 128)):
        if dst < n:
            c.advice[d.index][dst] = c.advice[a.index][src]
            c.copy(a, src, d, dst)
    c.instances = []
    c.a, c.b, c.d = a.index, b.index, d.index
    return c


def lookup_edge_circuit(plonk, k, seed=0):
    """Three lookups over advice x, y, w and fixed t1, t2: lookup 0 is x in t1 (one fixed table expression: sorted at
    keygen), lookup 1 is (x, y) in (t1, t2) (theta-compressed, sorted per check), lookup 2 is x in w (a table that is part
    of the witness). t1 holds 777 at row u only — a value no usable table row has."""
    rnd = np.random.RandomState(400 + seed)
    cs = plonk.ConstraintSystem()
    x, y, w = cs.advice_column(), cs.advice_column(), cs.advice_column()
    t1, t2 = cs.fixed_column(), cs.fixed_column()
    cs.lookup(lambda m: [(m.query_advice(x, 0), m.query_fixed(t1, 0))])
    cs.lookup(lambda m: [(m.query_advice(x, 0), m.query_fixed(t1, 0)), (m.query_advice(y, 0), m.query_fixed(t2, 0))])
    cs.lookup(lambda m: [(m.query_advice(x, 0), m.query_advice(w, 0))])
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    n, u = c.n, c.usable
    for i in range(u):
        c.fixed[t1.index][i] = i % 37
        c.fixed[t2.index][i] = (i % 37) * 1000 + 1
    for i in range(u, n):
        c.fixed[t1.index][i] = 777
        c.fixed[t2.index][i] = 777001
    for row in range(n):
        p = int(rnd.randint(0, min(u, 37)))
        c.advice[x.index][row], c.advice[y.index][row] = c.fixed[t1.index][p], c.fixed[t2.index][p]
        c.advice[w.index][row] = c.fixed[t1.index][row] if row < u else 777
    c.instances = []
    c.x, c.y, c.w = x.index, y.index, w.index
    return c
