"""A gadget circuit whose every advice cell is a node of a witness program (tests/test_gpu_witness_e2e.py), written the
way the reference's halo2-base circuits are: ONE vertical gate column G with q * (G[r] + G[r+1] * G[r+2] - G[r+3]), one
8-bit range-lookup column L, constants in a fixed column K, and copy constraints between all of them and the instance
column. From two 64-bit inputs x, y and the host's hints q, rem (x * y = q * M + rem) it checks the product limb-wise, in
32-bit limbs: every limb of x, y, q, rem recomposed from range-checked bytes, the three limb equations closed by carries
that are themselves range-checked (a carry may be negative: it is checked with an offset), and rem < M through the bytes
of M - 1 - rem. The same calls lay out the circuit (selector rows, copies, constants) and record the program.

k = 9: an 8-bit table needs 256 usable rows, and 2^8 rows leave fewer than that after the blinding rows."""
import circuits

M = 0xFFFFFFFF00000001
CARRY_OFFSET = 1 << 34  # |carry| < 2^33, so carry + 2^34 is a 35-bit natural number: five bytes


class MulModGadget:
    def __init__(self, plonk, W, k=9):
        cs = plonk.ConstraintSystem()
        self.G, self.L = cs.advice_column(), cs.advice_column()
        self.q = cs.selector()
        self.T, self.K = cs.fixed_column(), cs.fixed_column()
        self.I = cs.instance_column()
        for col in (self.G, self.L, self.K, self.I):
            cs.enable_equality(col)
        G, L, q, T = self.G, self.L, self.q, self.T
        cs.create_gate(lambda m: [m.query_selector(q) * (m.query_advice(G, 0) + m.query_advice(G, 1) * m.query_advice(G, 2) - m.query_advice(G, 3))])
        cs.lookup(lambda m: [(m.query_advice(L, 0), m.query_fixed(T, 0))])
        self.c = c = circuits.Circuit(cs, k)
        c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
        assert c.usable >= 256
        for i in range(256):
            c.fixed[T.index][i] = i
        self.p = W(k, 2)
        self.g_row = self.l_row = self.k_row = 0
        self.home = {}     # node -> its first cell (column, row): later placements are copied to it
        self.consts = {}   # value -> node
        self.assigned = set()
        self.instance_nodes = []
        self._build()

    # ---- layout
    def _place(self, node, col, row):
        self.p.assign(node, col.index, row)
        self.assigned.add((col.index, row))
        if node in self.home:
            hc, hr = self.home[node]
            self.c.copy(hc, hr, col, row)
        else:
            self.home[node] = (col, row)

    def const(self, v):
        if v not in self.consts:
            node = self.p.const(v)
            self.consts[v] = node
            self.c.fixed[self.K.index][self.k_row] = v
            self.home[node] = (self.K, self.k_row)  # every use in an advice cell is copied to the fixed cell
            self.k_row += 1
        return self.consts[v]

    def gate(self, a, b, c, d):
        """a + b * c = d on four new rows of G."""
        r = self.g_row
        self.c.fixed[self.q.index][r] = 1
        for i, node in enumerate((a, b, c, d)):
            self._place(node, self.G, r + i)
        self.g_row += 4
        return d

    def mul_add(self, a, b, c):
        return self.gate(a, b, c, self.p.add(a, self.p.mul(b, c)))

    def range_byte(self, node):
        self._place(node, self.L, self.l_row)
        self.l_row += 1
        return node

    def recompose(self, whole, lo, nbytes):
        """`nbytes` range-checked bytes of node `whole` from bit `lo`, summed back by the gate; returns the limb's node."""
        p = self.p
        limb = p.bits(whole, lo, 8 * nbytes)
        acc = self.const(0)
        for i in range(nbytes):
            byte = self.range_byte(p.bits(whole, lo + 8 * i, 8))
            weight = self.const(1 << (8 * i))
            nxt = limb if i == nbytes - 1 else p.add(acc, p.mul(byte, weight))
            acc = self.gate(acc, byte, weight, nxt)
        return limb

    def carry(self, lhs, rhs):
        """(lhs - rhs) / 2^32 as a field element, possibly negative, with carry + CARRY_OFFSET range-checked in five bytes."""
        p = self.p
        shifted = p.add(p.sub(lhs, rhs), self.const(CARRY_OFFSET << 32))
        off = self.recompose(shifted, 32, 5)
        cy = p.sub(off, self.const(CARRY_OFFSET))
        self.gate(cy, self.const(CARRY_OFFSET), self.const(1), off)
        return cy

    def _build(self):
        p = self.p
        x, y, qh, rem = p.input(), p.input(), p.input(), p.input()
        zero, one, two32 = self.const(0), self.const(1), self.const(1 << 32)
        m0, m1 = self.const(M & 0xFFFFFFFF), self.const(M >> 32)
        (x0, x1), (y0, y1), (q0, q1), (r0, r1) = [(self.recompose(v, 0, 4), self.recompose(v, 32, 4)) for v in (x, y, qh, rem)]
        t0 = self.mul_add(zero, x0, y0)
        t1 = self.mul_add(self.mul_add(zero, x0, y1), x1, y0)
        t2 = self.mul_add(zero, x1, y1)
        u0 = self.mul_add(r0, q0, m0)
        u1 = self.mul_add(self.mul_add(r1, q0, m1), q1, m0)
        u2 = self.mul_add(zero, q1, m1)
        c0 = self.carry(t0, u0)
        self.gate(u0, c0, two32, t0)
        s1 = self.mul_add(c0, t1, one)
        c1 = self.carry(s1, u1)
        self.gate(u1, c1, two32, s1)
        self.gate(c1, t2, one, u2)
        # rem < M: M - 1 - rem is a 64-bit natural number
        rfull = self.mul_add(r0, r1, two32)
        slack = p.sub(self.const(M - 1), rfull)
        self.gate(rfull, self.recompose(slack, 0, 8), one, self.const(M - 1))
        xfull = self.mul_add(x0, x1, two32)
        for i, node in enumerate((rfull, xfull)):
            p.expose(node)
            self.instance_nodes.append(node)
            self.c.copy(self.I, i, *self.home[node])
        assert self.g_row <= self.c.usable and self.l_row <= self.c.usable
        # every other advice cell is a node too: the constant 0
        for col in (self.G, self.L):
            for row in range(self.c.n):
                if (col.index, row) not in self.assigned:
                    p.assign(zero, col.index, row)

    # ---- witnesses
    @staticmethod
    def inputs(x, y, hint_error=0):
        qh, rem = divmod(x * y, M)
        assert qh < 1 << 64
        return [x, y, qh, rem + hint_error]

    def witness(self, values):
        """(advice columns, instance columns) as integers from the reference's node values."""
        adv = [[0] * self.c.n for _ in range(2)]
        for node, col, row in self.p.cells:
            adv[col][row] = values[node]
        return adv, [[values[n] for n in self.instance_nodes]]
