"""The reference of amdzk_check_witness: Python integers, the walk of workloads.check_satisfied, but COLLECTING one
(kind, index, first_row, count) per failing constraint instead of asserting at the first failure.

Semantics (include/amdzk.h; upstream's MockProver::verify_at_rows(usable, usable) without its region bookkeeping), with
n = 2^k and u = n - (blinding_factors + 1):
  gates    gate polynomial g fails at row r < u when it is non-zero there; rotations wrap modulo n, cells at rows >= u are
           read as they are (instance columns are zero beyond their values);
  lookups  lookup l fails at row r < u when the tuple of its input expressions at r equals no tuple of its table
           expressions at a row < u — tuples compared exactly, no theta;
  copies   permutation column i fails at row j < n when cell (i, j) differs from the cell mapping[i][j] names.
Entries are ordered by kind (GATE, LOOKUP, COPY), then index."""
GATE, LOOKUP, COPY = 0, 1, 2
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


class Walk:
    """The cells of one witness of circuit `c` (circuits.Circuit) and the evaluation of its expressions on them."""

    def __init__(self, c, advice=None, instances=None, challenges=None):
        self.c, self.desc, self.n, self.u = c, c.desc, c.n, c.usable
        self.fixed = c.fixed
        self.advice = c.advice if advice is None else advice
        instances = c.instances if instances is None else instances
        self.inst = [list(v) + [0] * (c.n - len(v)) for v in instances]
        self.challenges = list(challenges) if challenges is not None else []

    def ev(self, e, row):
        op = e[0]
        if op == "const":
            return e[1] % R
        if op == "fixed":
            return self.fixed[e[1]][(row + e[2]) % self.n]
        if op == "advice":
            return self.advice[e[1]][(row + e[2]) % self.n]
        if op == "instance":
            return self.inst[e[1]][(row + e[2]) % self.n]
        if op == "challenge":
            return self.challenges[e[1]] % R
        if op == "neg":
            return (-self.ev(e[1], row)) % R
        if op == "sum":
            return (self.ev(e[1], row) + self.ev(e[2], row)) % R
        if op == "product":
            return self.ev(e[1], row) * self.ev(e[2], row) % R
        if op == "scaled":
            return self.ev(e[1], row) * e[2] % R
        raise ValueError("unknown expression node %r" % (op,))

    def value(self, kind, index, row):
        return self.advice[index][row] if kind == 0 else self.fixed[index][row] if kind == 1 else self.inst[index][row]

    def perm_columns(self):
        return [(col.kind, col.index) if hasattr(col, "kind") else tuple(col) for col in self.desc["permutation_columns"]]

    # ---- single rows (what the metric-shape test asks about a reported first_row)
    def gate_fails_at(self, g, row):
        return self.ev(self.desc["gates"][g], row) != 0

    def table(self, l):
        lk = self.desc["lookups"][l]
        return {tuple(self.ev(e, row) for e in lk["tables"]) for row in range(self.u)}

    def lookup_fails_at(self, l, row, table=None):
        lk = self.desc["lookups"][l]
        return tuple(self.ev(e, row) for e in lk["inputs"]) not in (self.table(l) if table is None else table)

    def copy_fails_at(self, i, row):
        cols = self.perm_columns()
        pi, pj = self.c.assembly.mapping[i][row]
        return self.value(*cols[i], row) != self.value(*cols[pi], pj)

    # ---- the whole report
    def report(self):
        out = []

        def collect(kind, index, rows):
            rows = list(rows)
            if rows:
                out.append((kind, index, rows[0], len(rows)))

        for g in range(len(self.desc["gates"])):
            collect(GATE, g, (row for row in range(self.u) if self.gate_fails_at(g, row)))
        for l in range(len(self.desc["lookups"])):
            table = self.table(l)
            collect(LOOKUP, l, (row for row in range(self.u) if self.lookup_fails_at(l, row, table)))
        for i in range(len(self.perm_columns())):
            collect(COPY, i, (row for row in range(self.n) if self.copy_fails_at(i, row)))
        return out


def report(c, advice=None, instances=None, challenges=None):
    """[(kind, index, first_row, count)] of the witness (c's own by default) under the semantics above."""
    return Walk(c, advice, instances, challenges).report()
