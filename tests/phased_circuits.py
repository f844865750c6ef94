"""Circuits with challenge phases for the prover tests, written against the product's ConstraintSystem mirror
(advice_column_in / challenge_usable_after / Expression.challenge). Advice columns are declared phase after phase
(tests/phased_oracle.py relies on it; the library does not).

A PhasedCircuit is a circuits.Circuit whose advice of the later phases is not assigned up front: `fill(phase, challenges,
advice)` computes the columns of `phase` from the challenges known so far ({index: int}), in place — what the device's
phase callback and the CPU harness both call.

  rlc_circuit           two phase-0 columns a, b, one phase-1 column r = a + ch * b (an RLC chip in miniature) and one
                        challenge, used in a gate q * (r - (a + ch * b)), on both sides of a lookup (a + ch * b against
                        t0 + ch * t1) and, through r, in a copy constraint; three_phases adds a phase-2 column
                        s = r * ch2 + ch * a and a second challenge usable after phase 1
  random_phased_circuit a random phased constraint system with a satisfying witness
"""
import numpy as np

import circuits
import phased_oracle as PO

R = circuits.R


class PhasedCircuit(circuits.Circuit):
    fill = None

    def witness_for(self, seed):
        """(advice with the later phases still zero, fill) of another witness of the same layout."""
        raise NotImplementedError


def rlc_circuit(plonk, k=5, seed=1, three_phases=False, ignore_challenge=False, interleaved=False):
    """interleaved: the columns are declared a, r, b(, s) — phases 0, 1, 0(, 2) — instead of phase after phase. Queries,
    gates, lookups and the permutation are made in the same order either way, so the proof is the same bytes."""
    cs = plonk.ConstraintSystem()
    if interleaved:
        a = cs.advice_column()
        r = cs.advice_column_in(1)
        b = cs.advice_column()
    else:
        a, b = cs.advice_column(), cs.advice_column()
        r = cs.advice_column_in(1)
    ch = cs.challenge_usable_after(0)
    s = ch2 = None
    if three_phases:
        s = cs.advice_column_in(2)
        ch2 = cs.challenge_usable_after(1)
    q, t0, t1 = cs.selector(), cs.fixed_column(), cs.fixed_column()
    cs.enable_equality(a)
    cs.enable_equality(r)
    E = plonk.Expression

    def gates(m):
        rlc = m.query_advice(a, 0) + E.challenge(ch) * m.query_advice(b, 0)
        out = [m.query_selector(q) * (m.query_advice(r, 0) - rlc)]
        if three_phases:
            out.append(m.query_selector(q) * (m.query_advice(s, 0) - (m.query_advice(r, 0) * E.challenge(ch2) + E.challenge(ch) * m.query_advice(a, 1))))
        return out

    cs.create_gate(gates)
    cs.lookup(lambda m: [(m.query_advice(a, 0) + E.challenge(ch) * m.query_advice(b, 0),
                          m.query_fixed(t0, 0) + E.challenge(ch) * m.query_fixed(t1, 0))])
    c = PhasedCircuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    u = c.usable
    for i in range(u):
        c.fixed[t0.index][i] = i % 11
        c.fixed[t1.index][i] = ((i % 11) ** 2 + 1) % R
    for row in range(u - 1):  # the last usable row is left off: the three-phase gate reads a at the next row
        c.fixed[q.index][row] = 1
    r1, r2 = 1, u // 2
    c.copy(r, r1, r, r2)
    c.copy(a, r1, a, r2)

    def assign(seed_):
        rnd = np.random.RandomState(seed_)
        adv = [[0] * c.n for _ in range(cs.num_advice)]
        for row in range(u):  # every usable row looks (a, b) up: a pair of the table
            j = int(rnd.randint(0, min(u, 11)))
            adv[a.index][row], adv[b.index][row] = c.fixed[t0.index][j], c.fixed[t1.index][j]
        adv[a.index][r2], adv[b.index][r2] = adv[a.index][r1], adv[b.index][r1]

        def fill(phase, chal, advice):
            if phase == 1:
                x = 5 if ignore_challenge else chal[ch.index]
                for row in range(u):
                    advice[r.index][row] = (advice[a.index][row] + x * advice[b.index][row]) % R
            elif phase == 2 and three_phases:
                for row in range(u):
                    advice[s.index][row] = (advice[r.index][row] * chal[ch2.index] + chal[ch.index] * advice[a.index][(row + 1) % c.n]) % R
        return adv, fill

    c.advice, c.fill = assign(seed)
    c.witness_for = assign
    c.instances = []
    return c


def random_phased_circuit(plonk, k=5, seed=0):
    """Random shapes: 1-3 phase-0 columns and 0-2 phase-0 lookup-input columns, 1-2 phase-1 columns, in 40 % of the seeds
    1-2 phase-2 columns; one challenge after every phase that has a later one (sometimes two after phase 0) and sometimes
    one after the LAST phase (usable by gates and lookups without feeding any column); 0-1 instance columns. Every
    later-phase column `out` is defined by a gate sel * (out - f) with f a random expression (degree <= 3 and sums of such,
    rotations -2..2, constants, scaled terms, negations) over the columns of earlier phases, the fixed and instance columns
    and the challenges known before out's phase. One lookup per lookup-input column, with a challenge on both sides
    (input v * ch + v against table t0 * ch + t1: no table is constant). A permutation over a random subset of the columns
    of all three kinds and all phases, with copies between free cells of phase-0 columns and of one later-phase column.
    Rows 0, 1 and the last two usable rows carry no gate, so that rotated queries stay inside the usable rows."""
    rnd = np.random.RandomState(7000 + seed)
    ri = lambda lo, hi: int(rnd.randint(lo, hi + 1))
    cs = plonk.ConstraintSystem()
    E = plonk.Expression
    nph = 3 if rnd.rand() < 0.4 else 2
    cols = {0: [cs.advice_column() for _ in range(ri(1, 3))]}
    lk_in = [cs.advice_column() for _ in range(ri(0, 2))]  # phase-0 inputs of the lookups
    chals = {}  # phase -> challenges usable after it
    for p in range(1, nph):
        chals[p - 1] = [cs.challenge_usable_after(p - 1) for _ in range(2 if (p == 1 and rnd.rand() < 0.3) else 1)]
        cols[p] = [cs.advice_column_in(p) for _ in range(ri(1, 2))]
    if rnd.rand() < 0.3:
        chals[nph - 1] = [cs.challenge_usable_after(nph - 1)]
    fixed = [cs.fixed_column() for _ in range(ri(1, 2))]
    inst = [cs.instance_column() for _ in range(ri(0, 1))]
    sel = cs.selector()
    tabs = [(cs.fixed_column(), cs.fixed_column()) for _ in lk_in]

    def known_before(p):
        return [c for q in range(p) for c in chals.get(q, [])]

    def rand_leaf(m, p):
        readable = [c for q in range(p) for c in cols[q]] + (lk_in if p > 0 else [])
        x = rnd.rand()
        rot = ri(-2, 2) if rnd.rand() < 0.5 else 0
        if x < 0.55 or not readable:
            return m.query_advice(readable[ri(0, len(readable) - 1)], rot) if readable else m.query_fixed(fixed[0], rot)
        if x < 0.7:
            return m.query_fixed(fixed[ri(0, len(fixed) - 1)], rot)
        if x < 0.8 and inst:
            return m.query_instance(inst[0], rot)
        kn = known_before(p)
        if kn:
            return E.challenge(kn[ri(0, len(kn) - 1)])
        return E.constant(ri(1, 1 << 20))

    def rand_expr(m, p, deg):
        if deg <= 1:
            e = rand_leaf(m, p)
            x = rnd.rand()
            if x < 0.2:
                e = e * ri(2, 1 << 16)
            elif x < 0.3:
                e = -e
            elif x < 0.45:
                e = e + rand_leaf(m, p)
            return e
        left = ri(1, deg - 1)
        e = rand_expr(m, p, left) * rand_expr(m, p, deg - left)
        if rnd.rand() < 0.5:
            e = e + rand_expr(m, p, ri(1, deg))
        return e

    defs = []  # (out column, phase, expression tuple) in definition order

    def gates(m):
        out = []
        for p in range(1, nph):
            for col in cols[p]:
                f = rand_expr(m, p, ri(1, 3))
                if p == nph - 1 and chals.get(p - 1):  # the last challenge is used at least once
                    f = f + E.challenge(chals[p - 1][-1]) * m.query_advice(cols[0][0], 0)
                defs.append((col, p, f.to_tuple()))
                out.append(m.query_selector(sel) * (m.query_advice(col, 0) - f))
        for chl in chals.get(nph - 1, []):  # a challenge behind the last phase: a gate that is zero for every witness
            x = m.query_advice(cols[nph - 1][0], 0)
            out.append(m.query_selector(sel) * (E.challenge(chl) * (x - x)))
        return out

    cs.create_gate(gates)
    first = known_before(nph)[0]
    for li, col in enumerate(lk_in):
        t0, t1 = tabs[li]
        cs.lookup(lambda m, col=col, t0=t0, t1=t1: [(m.query_advice(col, 0) * E.challenge(first) + m.query_advice(col, 0),
                                                    m.query_fixed(t0, 0) * E.challenge(first) + m.query_fixed(t1, 0))])
    all_adv = [c for p in range(nph) for c in cols[p]] + lk_in
    perm = [c for c in all_adv + fixed + inst if rnd.rand() < 0.6]
    for col in perm:
        cs.enable_equality(col)
    c = PhasedCircuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    u, n = c.usable, c.n
    rows = list(range(2, u - 2))  # rows whose rotated queries stay inside the usable rows
    for row in rows:
        c.fixed[sel.index][row] = 1
    for col in fixed:
        for row in range(u):
            c.fixed[col.index][row] = ri(0, 1 << 30)
    for t0, t1 in tabs:
        for row in range(u):
            c.fixed[t0.index][row] = c.fixed[t1.index][row] = row % 13  # input v: v * ch + v is in the table t0 * ch + t1
    c.instances = [[ri(0, 1 << 30) for _ in range(ri(1, 4))] for _ in inst]
    # copy constraints: rows 0 and 1 carry no gate (their cells are free). Phase-0 cells are made equal by the witness;
    # rows 0 and 1 of a later-phase column are never assigned, so both stay zero.
    p0 = [col for col in perm if col.kind == 0 and col in cols[0] + lk_in][:2]
    later = [col for col in perm if col.kind == 0 and col not in cols[0] + lk_in][:1]
    for col in p0 + later:
        c.copy(col, 0, col, 1)
    nch = len(cs.challenge_phase)

    def fill(phase, chal, advice):
        for col, p, f in defs:
            if p != phase:
                continue
            spec = PO.specialise({"gates": [f], "lookups": []}, [chal.get(i, 0) for i in range(nch)])["gates"][0]
            for row in rows:
                advice[col.index][row] = PO.PR.evaluate_expr(spec, lambda cc, r_: c.fixed[cc][(row + r_) % n], lambda cc, r_: advice[cc][(row + r_) % n],
                                                             lambda cc, r_: (c.instances[cc] + [0] * n)[(row + r_) % n])

    def assign(seed_):
        rw = np.random.RandomState(9000 + seed_)
        adv = [[0] * n for _ in range(cs.num_advice)]
        for col in cols[0] + lk_in:
            for row in range(u):
                adv[col.index][row] = int(rw.randint(0, 13)) if col in lk_in else int(rw.randint(0, 1 << 30))
        for col in p0:
            adv[col.index][1] = adv[col.index][0]
        return adv, fill

    c.advice, c.fill = assign(seed)
    c.witness_for = assign
    return c
