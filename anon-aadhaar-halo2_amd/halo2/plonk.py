"""Mirror of halo2_proofs::plonk::{ConstraintSystem, Expression, Column, keygen, create_proof}
(v2023_01_20 [UP], /root/reference/Cargo.lock:469-471) — the interface the reference's circuits
implement and call: `Circuit::configure(meta)` (/root/reference/src/lib.rs:295-326,
src/signal.rs:27-49, src/conditional_secrets.rs:81-187, src/timestamp.rs:58-138).

This module is host-side description only: it records columns, queries, gates, lookups and the
permutation exactly the way upstream's ConstraintSystem does (query indices in first-use order,
`degree()`, `blinding_factors()`), and flattens the result into the arrays the C ABI takes
(`amdzk_circuit_*`, include/amdzk.h). All O(n) proving work happens on the device.

Selectors are modelled after upstream's selector compression has run, i.e. as fixed columns.
Field constants are Python ints (canonical); they are converted to Montgomery limbs at export.
"""
import collections
from dataclasses import dataclass, field
from typing import List, Tuple

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

ADVICE, FIXED, INSTANCE = 0, 1, 2  # upstream's `Any` ordering: Advice < Fixed < Instance


@dataclass(frozen=True)
class Column:
    kind: int
    index: int


@dataclass(frozen=True)
class Challenge:
    """plonk::Challenge: squeezed once the advice columns of `phase` (and of the phases before it) are committed."""
    index: int
    phase: int


class Expression:
    """plonk::Expression: Constant | Fixed | Advice | Instance | Challenge | Negated | Sum | Product | Scaled."""

    __slots__ = ("op", "a", "b")

    def __init__(self, op, a=None, b=None):
        self.op, self.a, self.b = op, a, b

    @staticmethod
    def constant(v):
        return Expression("const", v % R)

    @staticmethod
    def challenge(ch):
        """Expression::Challenge(ch): `ch` is what ConstraintSystem.challenge_usable_after returned."""
        return Expression("challenge", ch.index if isinstance(ch, Challenge) else int(ch))

    def __neg__(self):
        return Expression("neg", self)

    def __add__(self, o):
        return Expression("sum", self, _lift(o))

    def __radd__(self, o):
        return Expression("sum", _lift(o), self)

    def __sub__(self, o):
        return Expression("sum", self, Expression("neg", _lift(o)))

    def __rsub__(self, o):
        return Expression("sum", _lift(o), Expression("neg", self))

    def __mul__(self, o):
        if isinstance(o, int):
            return Expression("scaled", self, o % R)
        return Expression("product", self, o)

    def __rmul__(self, o):
        return self.__mul__(o)

    def degree(self):
        op = self.op
        if op in ("const", "challenge"):
            return 0
        if op in ("fixed", "advice", "instance"):
            return 1
        if op == "neg":
            return self.a.degree()
        if op == "sum":
            return max(self.a.degree(), self.b.degree())
        if op == "product":
            return self.a.degree() + self.b.degree()
        if op == "scaled":
            return self.a.degree()
        raise ValueError(op)

    def to_tuple(self):
        op = self.op
        if op == "const":
            return ("const", self.a)
        if op == "challenge":
            return ("challenge", self.a)
        if op in ("fixed", "advice", "instance"):
            return (op, self.a, self.b)  # (column index, rotation)
        if op == "neg":
            return ("neg", self.a.to_tuple())
        if op in ("sum", "product"):
            return (op, self.a.to_tuple(), self.b.to_tuple())
        if op == "scaled":
            return ("scaled", self.a.to_tuple(), self.b)
        raise ValueError(op)


def _lift(o):
    return o if isinstance(o, Expression) else Expression.constant(o)


class VirtualCells:
    """What `meta.create_gate(|meta| ...)` / `meta.lookup(|meta| ...)` closures receive."""

    def __init__(self, cs):
        self.cs = cs

    def query_advice(self, col, rot=0):
        assert col.kind == ADVICE
        if self.cs._query(self.cs.advice_queries, col, rot):
            self.cs.num_advice_queries[col.index] += 1
        return Expression("advice", col.index, rot)

    def query_fixed(self, col, rot=0):
        assert col.kind == FIXED
        self.cs._query(self.cs.fixed_queries, col, rot)
        return Expression("fixed", col.index, rot)

    def query_selector(self, col):
        return self.query_fixed(col, 0)

    def query_instance(self, col, rot=0):
        assert col.kind == INSTANCE
        self.cs._query(self.cs.instance_queries, col, rot)
        return Expression("instance", col.index, rot)


class ConstraintSystem:
    def __init__(self):
        self.num_fixed = self.num_advice = self.num_instance = 0
        self.advice_queries: List[Tuple[Column, int]] = []
        self.fixed_queries: List[Tuple[Column, int]] = []
        self.instance_queries: List[Tuple[Column, int]] = []
        self.num_advice_queries: List[int] = []
        self.gates: List[Expression] = []       # one entry per polynomial constraint, in order
        self.lookups: List[Tuple[List[Expression], List[Expression]]] = []
        self.permutation_columns: List[Column] = []
        self.minimum_degree = None
        self.advice_column_phase: List[int] = []
        self.challenge_phase: List[int] = []

    # ---- columns
    def advice_column(self):
        return self.advice_column_in(0)

    def _phase_has_advice(self, phase):
        return phase in self.advice_column_phase

    def advice_column_in(self, phase):
        """ConstraintSystem::advice_column_in: phases are 0, 1, 2; a phase above 0 needs a column in the phase before it."""
        if phase not in (0, 1, 2):
            raise ValueError("advice_column_in: phase %r (phases are 0, 1, 2)" % (phase,))
        if phase > 0 and not self._phase_has_advice(phase - 1):
            raise ValueError("advice_column_in: no advice column in phase %d, the one before phase %d" % (phase - 1, phase))
        self.num_advice += 1
        self.num_advice_queries.append(0)
        self.advice_column_phase.append(phase)
        return Column(ADVICE, self.num_advice - 1)

    def challenge_usable_after(self, phase):
        """ConstraintSystem::challenge_usable_after: the phase must already have an advice column."""
        if phase not in (0, 1, 2) or not self._phase_has_advice(phase):
            raise ValueError("challenge_usable_after: no advice column in phase %r" % (phase,))
        self.challenge_phase.append(phase)
        return Challenge(len(self.challenge_phase) - 1, phase)

    def fixed_column(self):
        self.num_fixed += 1
        return Column(FIXED, self.num_fixed - 1)

    selector = fixed_column  # post-compression model

    def instance_column(self):
        self.num_instance += 1
        return Column(INSTANCE, self.num_instance - 1)

    def _query(self, lst, col, rot):
        """query_*_index: register (column, rotation) on first use; True if it was new."""
        if (col, rot) in lst:
            return False
        lst.append((col, rot))
        return True

    def enable_equality(self, col):
        """ConstraintSystem::enable_equality: query at Rotation::cur() + add to the permutation."""
        if col.kind == ADVICE:
            VirtualCells(self).query_advice(col, 0)
        elif col.kind == FIXED:
            VirtualCells(self).query_fixed(col, 0)
        else:
            VirtualCells(self).query_instance(col, 0)
        if col not in self.permutation_columns:
            self.permutation_columns.append(col)

    def create_gate(self, fn):
        polys = fn(VirtualCells(self))
        if isinstance(polys, Expression):
            polys = [polys]
        assert polys, "create_gate: gates must contain at least one constraint"
        self.gates.extend(polys)

    def lookup(self, fn):
        """fn(meta) -> [(input_expr, table_expr), ...]"""
        pairs = fn(VirtualCells(self))
        self.lookups.append(([p[0] for p in pairs], [p[1] for p in pairs]))
        return len(self.lookups) - 1

    # ---- derived quantities (upstream formulas)
    def degree(self):
        d = 3  # permutation::Argument::required_degree() is the constant 3 upstream
        for inputs, tables in self.lookups:
            di = max([1] + [e.degree() for e in inputs])
            dt = max([1] + [e.degree() for e in tables])
            d = max(d, max(4, 2 + di + dt))
        for g in self.gates:
            d = max(d, g.degree())
        return max(d, self.minimum_degree or 1)

    def blinding_factors(self):
        factors = max(self.num_advice_queries) if self.num_advice_queries else 1
        return max(3, factors) + 2

    def minimum_rows(self):
        return self.blinding_factors() + 3

    def describe(self, k):
        """Plain-data description of the constraint system (what a Rust fork would export)."""
        cols = lambda qs: [(c.index, r) for c, r in qs]
        phases = {}
        if self.challenge_phase or any(self.advice_column_phase):  # phase-0 circuits keep the description they always had
            phases = {"advice_column_phase": list(self.advice_column_phase), "challenge_phase": list(self.challenge_phase)}
        return {
            **phases,
            "k": k,
            "num_fixed": self.num_fixed, "num_advice": self.num_advice, "num_instance": self.num_instance,
            "blinding_factors": self.blinding_factors(), "cs_degree": self.degree(),
            "advice_queries": cols(self.advice_queries), "fixed_queries": cols(self.fixed_queries),
            "instance_queries": cols(self.instance_queries),
            "gates": [g.to_tuple() for g in self.gates],
            "lookups": [{"inputs": [e.to_tuple() for e in i], "tables": [e.to_tuple() for e in t]} for i, t in self.lookups],
            "permutation_columns": [(c.kind, c.index) for c in self.permutation_columns],
        }


class Assembly:
    """plonk::permutation::keygen::Assembly: the copy-constraint cycles. mapping[col][row] =
    (col', row') with columns indexed by their position in `permutation_columns`."""

    def __init__(self, n, ncols):
        self.n, self.ncols = n, ncols
        self.mapping = [[(c, r) for r in range(n)] for c in range(ncols)]
        self.aux = [[(c, r) for r in range(n)] for c in range(ncols)]
        self.sizes = [[1] * n for _ in range(ncols)]

    def copy(self, lc, lr, rc, rr):
        """Assembly::copy (upstream's union by size of two cycles)."""
        left_cycle, right_cycle = self.aux[lc][lr], self.aux[rc][rr]
        if left_cycle == right_cycle:
            return
        if self.sizes[left_cycle[0]][left_cycle[1]] < self.sizes[right_cycle[0]][right_cycle[1]]:
            left_cycle, right_cycle = right_cycle, left_cycle
        self.sizes[left_cycle[0]][left_cycle[1]] += self.sizes[right_cycle[0]][right_cycle[1]]
        i, j = right_cycle
        while True:
            self.aux[i][j] = left_cycle
            i, j = self.mapping[i][j]
            if (i, j) == right_cycle:
                break
        tmp = self.mapping[lc][lr]
        self.mapping[lc][lr] = self.mapping[rc][rr]
        self.mapping[rc][rr] = tmp


# ------------------------------------------------------------------------------------------------
# Export to the C ABI (include/amdzk.h: amdzk_circuit) and the keygen / create_proof entry points.
import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

from .. import ffi as _ffi  # noqa: E402

_XOP = {"const": 1, "fixed": 2, "advice": 3, "instance": 4, "neg": 5, "sum": 6, "product": 7, "scaled": 8, "challenge": 9}


class _CCircuit(C.Structure):
    _fields_ = [("k", C.c_uint32), ("num_fixed", C.c_uint32), ("num_advice", C.c_uint32), ("num_instance", C.c_uint32),
                ("blinding_factors", C.c_uint32), ("cs_degree", C.c_uint32),
                ("num_advice_queries", C.c_uint32), ("advice_queries", C.c_void_p),
                ("num_fixed_queries", C.c_uint32), ("fixed_queries", C.c_void_p),
                ("num_instance_queries", C.c_uint32), ("instance_queries", C.c_void_p),
                ("num_gates", C.c_uint32), ("num_lookups", C.c_uint32), ("num_exprs", C.c_uint32),
                ("lookup_shape", C.c_void_p), ("expr_offsets", C.c_void_p), ("expr_words", C.c_void_p),
                ("num_constants", C.c_uint32), ("constants", C.c_void_p),
                ("num_perm_columns", C.c_uint32), ("perm_columns", C.c_void_p)]


def _mont_limbs(v):
    v = (v % R) * (1 << 256) % R
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def flatten_circuit(desc):
    """describe() dict -> (amdzk_circuit, keepalive list)."""
    consts, words, offsets = {}, [], [0]

    def cidx(v):
        return consts.setdefault(v % R, len(consts))

    def emit(e):
        op = e[0]
        if op == "const":
            words.append((_XOP[op] << 24) | cidx(e[1]))
        elif op == "challenge":
            assert 0 <= e[1] < (1 << 24)
            words.append((_XOP[op] << 24) | e[1])
        elif op in ("fixed", "advice", "instance"):
            assert -128 <= e[2] < 128 and e[1] < (1 << 16)
            words.append((_XOP[op] << 24) | (e[1] << 8) | (e[2] + 128))
        elif op == "neg":
            emit(e[1])
            words.append(_XOP[op] << 24)
        elif op in ("sum", "product"):
            emit(e[1])
            emit(e[2])
            words.append(_XOP[op] << 24)
        elif op == "scaled":
            emit(e[1])
            words.append((_XOP[op] << 24) | cidx(e[2]))
        else:
            raise ValueError(op)

    exprs = list(desc["gates"])
    shape = []
    for lk in desc["lookups"]:
        shape += [len(lk["inputs"]), len(lk["tables"])]
        exprs += list(lk["inputs"]) + list(lk["tables"])
    for e in exprs:
        emit(e)
        offsets.append(len(words))
    arrs = {
        "aq": np.array(desc["advice_queries"], dtype=np.int32).reshape(-1, 2),
        "fq": np.array(desc["fixed_queries"], dtype=np.int32).reshape(-1, 2),
        "iq": np.array(desc["instance_queries"], dtype=np.int32).reshape(-1, 2),
        "shape": np.array(shape, dtype=np.uint32),
        "off": np.array(offsets, dtype=np.uint32),
        "words": np.array(words, dtype=np.uint32),
        "consts": np.array([_mont_limbs(v) for v, _ in sorted(consts.items(), key=lambda kv: kv[1])], dtype=np.uint64).reshape(-1, 4),
        "perm": np.array(desc["permutation_columns"], dtype=np.uint32).reshape(-1, 2),
    }
    arrs = {k_: np.ascontiguousarray(v) for k_, v in arrs.items()}
    p = lambda a: a.ctypes.data if a.size else None
    c = _CCircuit(desc["k"], desc["num_fixed"], desc["num_advice"], desc["num_instance"], desc["blinding_factors"], desc["cs_degree"],
                  len(arrs["aq"]), p(arrs["aq"]), len(arrs["fq"]), p(arrs["fq"]), len(arrs["iq"]), p(arrs["iq"]),
                  len(desc["gates"]), len(desc["lookups"]), len(exprs), p(arrs["shape"]), p(arrs["off"]), p(arrs["words"]),
                  len(arrs["consts"]), p(arrs["consts"]), len(arrs["perm"]), p(arrs["perm"]))
    return c, arrs


def flatten_phases(desc):
    """describe() dict -> (amdzk_phases or None, keepalive): None for a description without a phase table."""
    if "advice_column_phase" not in desc:
        return None, None
    ap = np.ascontiguousarray(desc["advice_column_phase"], dtype=np.uint8)
    cp = np.ascontiguousarray(desc["challenge_phase"], dtype=np.uint8)
    assert len(ap) == desc["num_advice"]
    ph = _ffi.Phases(len(cp), ap.ctypes.data if ap.size else None, cp.ctypes.data if cp.size else None)
    return ph, (ap, cp)


def _env_keygen_flags():
    """The key's modes as amdzk_keygen takes them from the environment (AMDZK_FULL_COSETS, AMDZK_SERIAL)."""
    import os
    on = lambda name, empty: (os.environ[name] == "" and empty) or os.environ[name].lstrip("+-").isdigit() and int(os.environ[name]) != 0
    return (KEYGEN_FULL_COSETS if "AMDZK_FULL_COSETS" in os.environ and on("AMDZK_FULL_COSETS", True) else 0) | \
        (KEYGEN_SERIAL if "AMDZK_SERIAL" in os.environ and on("AMDZK_SERIAL", False) else 0)


class ProvingKey:
    """plonk::keygen::{keygen_vk, keygen_pk} result, resident on the device."""

    def __init__(self, ctx, params, desc, fixed_values, mapping, transcript_repr, flags=None, phases=None):
        """fixed_values: (num_fixed, n, 4) uint64 Montgomery; mapping: Assembly.mapping;
        transcript_repr: (4,) uint64 Montgomery Fr. flags: None = amdzk_keygen (the key's modes from the environment),
        else amdzk_keygen_ex with KEYGEN_FULL_COSETS / KEYGEN_SERIAL or'ed together. A description with a phase table
        (advice_column_in / challenge_usable_after), or an explicit `phases` (ffi.Phases), goes through amdzk_keygen_phased."""
        self.ctx, self.params, self.desc = ctx, params, desc
        n = 1 << desc["k"]
        cc, keep = flatten_circuit(desc)
        fv = np.ascontiguousarray(fixed_values, dtype=np.uint64).reshape(desc["num_fixed"], n, 4) if desc["num_fixed"] else np.zeros((0, n, 4), np.uint64)
        mp = np.ascontiguousarray(np.array(mapping, dtype=np.uint32).reshape(-1, n, 2)) if len(desc["permutation_columns"]) else np.zeros((0, n, 2), np.uint32)
        tr = np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4)
        h = C.c_void_p()
        ph, keep_ph = flatten_phases(desc) if phases is None else (phases, None)
        if ph is not None:
            ctx._chk(ctx.L.amdzk_keygen_phased(ctx.h, params.h, C.byref(cc), C.byref(ph), fv.ctypes.data if fv.size else None,
                                               mp.ctypes.data if mp.size else None, tr.ctypes.data, _env_keygen_flags() if flags is None else int(flags),
                                               C.byref(h)))
        elif flags is None:
            ctx._chk(ctx.L.amdzk_keygen(ctx.h, params.h, C.byref(cc), fv.ctypes.data if fv.size else None,
                                        mp.ctypes.data if mp.size else None, tr.ctypes.data, C.byref(h)))
        else:
            ctx._chk(ctx.L.amdzk_keygen_ex(ctx.h, params.h, C.byref(cc), fv.ctypes.data if fv.size else None,
                                           mp.ctypes.data if mp.size else None, tr.ctypes.data, int(flags), C.byref(h)))
        self.h = h
        del keep

    @classmethod
    def from_sigma(cls, ctx, params, desc, fixed_values, sigma_values, transcript_repr, flags=None, phases=None):
        """amdzk_keygen_sigma: the key from the sigma columns — permutation::ProvingKey::permutations, (num_perm_columns, n, 4)
        uint64 Montgomery, Lagrange form — instead of Assembly.mapping: what a process that has read a cached key holds. The
        same key as ProvingKey(...) from the mapping. flags: None = the modes from the environment."""
        n = 1 << desc["k"]
        cc, keep = flatten_circuit(desc)
        fv = np.ascontiguousarray(fixed_values, dtype=np.uint64).reshape(desc["num_fixed"], n, 4) if desc["num_fixed"] else np.zeros((0, n, 4), np.uint64)
        sg = None if sigma_values is None else np.ascontiguousarray(sigma_values, dtype=np.uint64).reshape(-1, n, 4)
        assert sg is None or sg.shape[0] == len(desc["permutation_columns"])
        tr = np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4)
        ph, keep_ph = flatten_phases(desc) if phases is None else (phases, None)
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_keygen_sigma(ctx.h, params.h, C.byref(cc), C.byref(ph) if ph is not None else None, fv.ctypes.data if fv.size else None,
                                          sg.ctypes.data if sg is not None and sg.size else None, tr.ctypes.data,
                                          _env_keygen_flags() if flags is None else int(flags), C.byref(h)))
        pk = object.__new__(cls)
        pk.ctx, pk.params, pk.desc, pk.h = ctx, params, desc, h
        del keep, keep_ph
        return pk

    @classmethod
    def read(cls, ctx, params, data, flags=None):
        """amdzk_pk_read: the key of a file made by write(), under `params` (the SRS the key was made with: anything else is
        refused). `desc` is rebuilt from the file. flags: None = the modes from the environment, as for a new key."""
        buf = None if data is None else np.frombuffer(data, dtype=np.uint8)
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_pk_read(ctx.h, params.h, buf.ctypes.data if buf is not None else None, buf.size if buf is not None else 0,
                                     _env_keygen_flags() if flags is None else int(flags), C.byref(h)))
        pk = object.__new__(cls)
        pk.ctx, pk.params, pk.desc, pk.h = ctx, params, blob_desc(data), h
        return pk

    def export(self, what):
        """amdzk_pk_export: the key's own columns as (columns, n, 4) uint64 Montgomery. 0: fixed (Lagrange), 1: sigma
        (Lagrange), 2: fixed coefficients, 3: sigma coefficients. Every handle of a key returns the same columns."""
        cnt = C.c_size_t(0)
        self.ctx._chk(self.ctx.L.amdzk_pk_export(self.ctx.h, self.h, what, None, 0, C.byref(cnt)))
        out = np.zeros((cnt.value, 4), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_pk_export(self.ctx.h, self.h, what, out.ctypes.data, cnt.value, C.byref(cnt)))
        return out.reshape(-1, 1 << self.desc["k"], 4)

    def write(self):
        """amdzk_pk_write: the key file (include/amdzk.h has the layout) as bytes."""
        size = int(self.ctx.L.amdzk_pk_serialized_size(self.h))
        out = np.zeros(size, np.uint8)
        written = C.c_size_t(0)
        self.ctx._chk(self.ctx.L.amdzk_pk_write(self.ctx.h, self.h, out.ctypes.data, size, C.byref(written)))
        assert written.value == size
        return out.tobytes()

    def clone_workspace(self):
        """amdzk_pk_clone_workspace: a key that shares this key's material and owns one more circuit instance's per-proof
        workspace — the second, third, ... instance of create_proof_multi, or one more proof of this circuit in flight.
        Free it and this key in any order: the last handle frees the key material."""
        c = object.__new__(ProvingKey)
        c.ctx, c.params, c.desc = self.ctx, self.params, self.desc
        h = C.c_void_p()
        self.ctx._chk(self.ctx.L.amdzk_pk_clone_workspace(self.ctx.h, self.h, C.byref(h)))
        c.h = h
        return c

    def commitments(self):
        """(fixed_commitments, permutation_commitments) as (m, 8) uint64 affine points."""
        f = np.zeros((self.desc["num_fixed"], 8), np.uint64)
        p = np.zeros((len(self.desc["permutation_columns"]), 8), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_pk_commitments(self.h, f.ctypes.data if f.size else None, p.ctypes.data if p.size else None))
        return f, p

    def inspect(self, what):
        """Test hook (amdzk_pk_inspect): what the last create_proof left in the key's workspace. 0: the committed
        polynomials in coefficient form (NP, n, 4), arena order advice | instance | A' | S' | Z_perm | Z_lookup;
        1: the challenges theta, beta, gamma, y (4, 4); 2: the pieces of h(X) (cs_degree - 1, n, 4)."""
        cnt = C.c_size_t(0)
        self.ctx._chk(self.ctx.L.amdzk_pk_inspect(self.ctx.h, self.h, what, None, 0, C.byref(cnt)))
        out = np.zeros((cnt.value, 4), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_pk_inspect(self.ctx.h, self.h, what, out.ctypes.data, cnt.value, C.byref(cnt)))
        n = 1 << self.desc["k"]
        return out if what in (1, 3) else out.reshape(-1, n, 4)

    def quotient_eval(self, polys, theta, beta, gamma, y):
        """evaluate_h + the quotient (amdzk_quotient_eval_dev): committed polynomials in coefficient form (NP, n, 4)
        and the challenges -> the pieces of h(X) (cs_degree - 1, n, 4)."""
        n = 1 << self.desc["k"]
        polys = np.ascontiguousarray(polys, dtype=np.uint64).reshape(-1, n, 4)
        d_in = self.ctx.alloc(polys.nbytes).upload(polys)
        qdeg = self.desc["cs_degree"] - 1
        d_out = self.ctx.alloc(qdeg * n * 32)
        ch = [np.ascontiguousarray(c, dtype=np.uint64).reshape(4) for c in (theta, beta, gamma, y)]
        try:
            self.ctx._chk(self.ctx.L.amdzk_quotient_eval_dev(self.ctx.h, self.h, d_in.ptr, n, ch[0].ctypes.data, ch[1].ctypes.data,
                                                             ch[2].ctypes.data, ch[3].ctypes.data, d_out.ptr))
            return d_out.download((qdeg, n, 4))
        finally:
            d_in.free(); d_out.free()

    def perm_cells(self):
        """(listed cells, sparse): the cells of the permutation products that are off the identity permutation, and whether
        this key's proofs form the products from them alone (amdzk_perm_products_dev's query)."""
        m, sp = C.c_size_t(0), C.c_int32(0)
        self.ctx._chk(self.ctx.L.amdzk_perm_products_dev(self.ctx.h, self.h, None, None, -1, None, C.byref(m), C.byref(sp)))
        return m.value, bool(sp.value)

    def perm_products(self, beta, gamma, route=-1):
        """amdzk_perm_products_dev: the permutation product columns before blinding, rows 0 ... usable, (nsets, usable + 1, 4),
        from the columns of the key's last proof. route 0: every row; 1: the listed cells alone; -1: as the key's proofs."""
        chunk = self.desc["cs_degree"] - 2
        nsets = (len(self.desc["permutation_columns"]) + chunk - 1) // chunk
        rows = (1 << self.desc["k"]) - self.desc["blinding_factors"]
        out = np.zeros((nsets, rows, 4), np.uint64)
        b, g = (np.ascontiguousarray(c, dtype=np.uint64).reshape(4) for c in (beta, gamma))
        self.ctx._chk(self.ctx.L.amdzk_perm_products_dev(self.ctx.h, self.h, b.ctypes.data, g.ctypes.data, int(route),
                                                         out.ctypes.data if out.size else None, None, None))
        return out

    def get_vk(self):
        """ProvingKey::get_vk (amdzk_vk_from_pk): the key's VerifyingKey, which outlives this key and its params."""
        h = C.c_void_p()
        self.ctx._chk(self.ctx.L.amdzk_vk_from_pk(self.ctx.h, self.h, C.byref(h)))
        return VerifyingKey(self.ctx, h, self.desc)

    def free(self):
        if self.h:
            self.ctx.L.amdzk_pk_free(self.ctx.h, self.h)
            self.h = None


class VerifyingKey:
    """plonk::VerifyingKey with the G of its params (amdzk_vk): all verify_proofs / decide_proofs read of a key. Host data
    only; it refers to no ParamsKZG and no ProvingKey. Made by keygen_vk, ProvingKey.get_vk or VerifyingKey.read."""

    def __init__(self, ctx, h, desc):
        self.ctx, self.h, self.desc = ctx, h, desc

    def commitments(self):
        """(fixed_commitments, permutation_commitments) as (m, 8) uint64 affine points."""
        f = np.zeros((self.desc["num_fixed"], 8), np.uint64)
        p = np.zeros((len(self.desc["permutation_columns"]), 8), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_vk_commitments(self.h, f.ctypes.data if f.size else None, p.ctypes.data if p.size else None))
        return f, p

    def write(self, vparams=None):
        """amdzk_vk_write: the key file (include/amdzk.h has the layout) as bytes; with vparams (kzg.ParamsVerifierKZG) the
        file carries [1]_2 and [s]_2 too, and is then all a verifier process needs."""
        g2, s_g2 = (None, None) if vparams is None else vparams.points
        size = int(self.ctx.L.amdzk_vk_serialized_size(self.h, 0 if vparams is None else 1))
        out = np.zeros(max(1, size), np.uint8)
        written = C.c_size_t(0)
        self.ctx._chk(self.ctx.L.amdzk_vk_write(self.ctx.h, self.h, None if g2 is None else g2.ctypes.data, None if s_g2 is None else s_g2.ctypes.data,
                                                out.ctypes.data, size, C.byref(written)))
        assert written.value == size
        return out[:size].tobytes()

    @classmethod
    def read(cls, ctx, data):
        """amdzk_vk_read: (vk, g2, s_g2) of a file made by write(); g2 / s_g2 are (16,) uint64 or None when the file has no
        pair. Needs no params. `desc` is rebuilt from the file."""
        buf = None if data is None else np.frombuffer(data, dtype=np.uint8)
        h, has = C.c_void_p(), C.c_int(0)
        g2, s_g2 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        ctx._chk(ctx.L.amdzk_vk_read(ctx.h, buf.ctypes.data if buf is not None and buf.size else None, buf.size if buf is not None else 0, C.byref(h),
                                     g2.ctypes.data, s_g2.ctypes.data, C.byref(has)))
        return cls(ctx, h, blob_desc(data)), (g2 if has.value else None), (s_g2 if has.value else None)

    def free(self):
        if self.h:
            self.ctx.L.amdzk_vk_free(self.ctx.h, self.h)
            self.h = None


def keygen_vk(ctx, params, desc, fixed_values, mapping=None, sigma_values=None, transcript_repr=None, phases=None):
    """plonk::keygen_vk (amdzk_keygen_vk): the VerifyingKey alone, from Assembly.mapping or from the sigma columns (exactly
    one of the two when the circuit has permutation columns), without making a proving key: the device holds the fixed and
    sigma columns while the call runs and nothing afterwards. The key ProvingKey(...).get_vk() gives for the same inputs."""
    if transcript_repr is None:
        raise ValueError("keygen_vk: transcript_repr is required ((4,) uint64 Montgomery Fr, as for ProvingKey)")
    n = 1 << desc["k"]
    cc, keep = flatten_circuit(desc)
    fv = np.ascontiguousarray(fixed_values, dtype=np.uint64).reshape(desc["num_fixed"], n, 4) if desc["num_fixed"] else np.zeros((0, n, 4), np.uint64)
    mp = None if mapping is None else np.ascontiguousarray(np.array(mapping, dtype=np.uint32).reshape(-1, n, 2))
    sg = None if sigma_values is None else np.ascontiguousarray(sigma_values, dtype=np.uint64).reshape(-1, n, 4)
    tr = np.ascontiguousarray(transcript_repr, dtype=np.uint64).reshape(4)
    ph, keep_ph = flatten_phases(desc) if phases is None else (phases, None)
    h = C.c_void_p()
    ctx._chk(ctx.L.amdzk_keygen_vk(ctx.h, params.h, C.byref(cc), C.byref(ph) if ph is not None else None, fv.ctypes.data if fv.size else None,
                                   mp.ctypes.data if mp is not None and mp.size else None, sg.ctypes.data if sg is not None and sg.size else None,
                                   tr.ctypes.data, C.byref(h)))
    del keep, keep_ph
    return VerifyingKey(ctx, h, desc)


KEYGEN_FULL_COSETS, KEYGEN_SERIAL = 1, 2  # include/amdzk.h AMDZK_KEYGEN_*
TRANSCRIPT_BLAKE2B, TRANSCRIPT_KECCAK256_EVM = 0, 1
MULTIOPEN_GWC = 0x100  # OR into `transcript`: poly::kzg::multiopen::ProverGWC instead of ProverSHPLONK


def blob_info(data):
    """amdzk_pk_blob_info: the shape of a key file — pure host code, no device needed. Runs every check ProvingKey.read makes
    before it touches the device (magic, version, exact length, digest, a consistent header); AmdzkError for a file it
    refuses, with the reason ProvingKey.read would give (amdzk_pk_blob_check: "pk_read: digest mismatch ...")."""
    buf = np.frombuffer(data, dtype=np.uint8) if data is not None else None
    ptr, size = (buf.ctypes.data, buf.size) if buf is not None and buf.size else (None, 0)
    out = [C.c_uint32(0) for _ in range(5)]
    rc = _ffi.lib().amdzk_pk_blob_info(ptr, size, *[C.byref(o) for o in out])
    if rc != 0:
        msg = C.create_string_buffer(256)
        _ffi.lib().amdzk_pk_blob_check(ptr, size, msg, len(msg))
        raise _ffi.AmdzkError(rc, msg.value.decode())
    return dict(zip(("k", "num_fixed", "num_advice", "num_perm_columns", "num_challenges"), (o.value for o in out)))


def vk_blob_info(data):
    """amdzk_vk_blob_info: the shape of a verifying-key file and whether it carries the G2 pair — pure host code, no device
    needed, every check VerifyingKey.read makes; AmdzkError with amdzk_vk_blob_check's reason ("vk_read: ...") for a file it
    refuses."""
    buf = np.frombuffer(data, dtype=np.uint8) if data is not None else None
    ptr, size = (buf.ctypes.data, buf.size) if buf is not None and buf.size else (None, 0)
    out, has = [C.c_uint32(0) for _ in range(5)], C.c_int(0)
    rc = _ffi.lib().amdzk_vk_blob_info(ptr, size, *[C.byref(o) for o in out], C.byref(has))
    if rc != 0:
        msg = C.create_string_buffer(256)
        _ffi.lib().amdzk_vk_blob_check(ptr, size, msg, len(msg))
        raise _ffi.AmdzkError(rc, msg.value.decode())
    info = dict(zip(("k", "num_fixed", "num_advice", "num_perm_columns", "num_challenges"), (o.value for o in out)))
    info["has_g2"] = bool(has.value)
    return info


def blob_desc(data):
    """The describe() dict in a key file's header (what flatten_circuit / flatten_phases had flattened), for a file
    blob_info / ProvingKey.read accepted — or vk_blob_info / VerifyingKey.read: the two files share these sections."""
    mv, pos = memoryview(data), [12]  # behind the magic and the format version

    def arr(count, dtype=np.uint32):
        a = np.frombuffer(mv, dtype=dtype, count=count, offset=pos[0])
        pos[0] += a.nbytes
        return a

    k, nf, na, ni, bf, deg = (int(v) for v in arr(6))
    queries = [[(int(c), int(r)) for c, r in arr(2 * int(arr(1)[0]), np.int32).reshape(-1, 2)] for _ in range(3)]
    ngates, nlookups, nexprs = (int(v) for v in arr(3))
    shape, off = arr(2 * nlookups), arr(nexprs + 1)
    words = arr(int(off[-1]))
    rinv = pow(1 << 256, -1, R)
    consts = [sum(int(x) << (64 * i) for i, x in enumerate(c)) * rinv % R for c in arr(4 * int(arr(1)[0]), np.uint64).reshape(-1, 4)]
    perm = [(int(a), int(b)) for a, b in arr(2 * int(arr(1)[0])).reshape(-1, 2)]
    names = {v: k_ for k_, v in _XOP.items()}

    def expr(e):
        st = []
        for w in words[int(off[e]):int(off[e + 1])]:
            op, pl = names[int(w) >> 24], int(w) & 0xFFFFFF
            if op == "const":
                st.append(("const", consts[pl]))
            elif op == "challenge":
                st.append(("challenge", pl))
            elif op in ("fixed", "advice", "instance"):
                st.append((op, pl >> 8, (pl & 0xFF) - 128))
            elif op == "neg":
                st.append(("neg", st.pop()))
            elif op == "scaled":
                st.append(("scaled", st.pop(), consts[pl]))
            else:
                b = st.pop()
                st.append((op, st.pop(), b))
        return st[0]

    exprs = [expr(e) for e in range(nexprs)]
    lookups, e = [], ngates
    for l in range(nlookups):
        a, b = int(shape[2 * l]), int(shape[2 * l + 1])
        lookups.append({"inputs": exprs[e:e + a], "tables": exprs[e + a:e + a + b]})
        e += a + b
    phases = {}
    if int(arr(1, np.uint8)[0]):
        nch = int(arr(1)[0])
        phases = {"advice_column_phase": [int(v) for v in arr(na, np.uint8)], "challenge_phase": [int(v) for v in arr(nch, np.uint8)]}
    return {**phases, "k": k, "num_fixed": nf, "num_advice": na, "num_instance": ni, "blinding_factors": bf, "cs_degree": deg,
            "advice_queries": queries[0], "fixed_queries": queries[1], "instance_queries": queries[2], "gates": exprs[:ngates],
            "lookups": lookups, "permutation_columns": perm}


def _guard(errors):
    """Wrap a Python callable for use as a C callback: an exception is kept in `errors` and turned into a non-zero return
    (nothing may unwind through the library)."""
    def guard(fn):
        def run(*a):
            try:
                return int(fn(*a) or 0)
            except BaseException as e:  # noqa: B902 - reported by the caller of create_proof
                errors.append(e)
                return 1
        return run
    return guard


def _write_transcript(tobj, errors):
    """An amdzk_transcript around the caller's TranscriptWrite object. Returns (struct, keep-alive)."""
    guard = _guard(errors)
    words = lambda p, cnt: np.array([p[i] for i in range(cnt)], dtype=np.uint64)

    def squeeze(_user, out):
        v = np.ascontiguousarray(tobj.squeeze_challenge(), dtype=np.uint64).reshape(4)
        for i in range(4):
            out[i] = int(v[i])
    cbs = [_ffi._T_IN(guard(lambda _u, p: tobj.common_point(words(p, 8)))), _ffi._T_IN(guard(lambda _u, p: tobj.common_scalar(words(p, 4)))),
           _ffi._T_IN(guard(lambda _u, p: tobj.write_point(words(p, 8)))), _ffi._T_IN(guard(lambda _u, p: tobj.write_scalar(words(p, 4)))),
           _ffi._T_IN(guard(squeeze))]
    tr = _ffi.Transcript(None, *cbs)
    return tr, cbs + [tr]


def _trampolines(synthesize, tobj, errors):
    """The C callbacks of amdzk_create_proof_opts around Python callables (_guard)."""
    guard = _guard(errors)
    phase_fn = _ffi.PHASE_FN()
    if synthesize is not None:
        def on_phase(_user, phase, ch, nch, stream):
            return synthesize(phase, np.array([[ch[4 * i + j] for j in range(4)] for i in range(nch)], dtype=np.uint64).reshape(nch, 4), stream)
        phase_fn = _ffi.PHASE_FN(guard(on_phase))
    tr, keep = None, [phase_fn]
    if tobj is not None:
        tr, keep_t = _write_transcript(tobj, errors)
        keep += keep_t
    return phase_fn, tr, keep


def create_proof_opts(ctx, pks, instances_list, d_advice_list, seed=0, scalars=None, advice_stride=None, transcript=TRANSCRIPT_BLAKE2B,
                      synthesize=None, transcript_object=None, opts_size=None):
    """amdzk_create_proof_opts. synthesize(phase, challenges (num_challenges, 4) uint64 Montgomery, hip_stream): fills the
    advice columns of `phase` (>= 1) of every instance on the device before it returns. transcript_object: the caller's
    TranscriptWrite — common_point / write_point take (8,) uint64 affine Montgomery words, common_scalar / write_scalar
    (4,), squeeze_challenge returns (4,), a residue below r; the proof bytes are then the object's and b"" is returned.
    The object's challenges are used as they are: words that are not below r raise AmdzkError (AMDZK_E_INVALID), beta = 0 on a
    key with permutation columns, x = 0 and SHPLONK's u on an opening point outside the first set AMDZK_E_UNSUPPORTED
    (include/amdzk.h, amdzk_transcript). `transcript` keeps its MULTIOPEN_GWC bit either way. opts_size: amdzk_proof_opts.size to report (tests)."""
    N = len(pks)
    assert N >= 1 and len(instances_list) == N and len(d_advice_list) == N
    n = 1 << pks[0].desc["k"]
    keep, inst_pp, lens_pp = [], (C.POINTER(C.c_void_p) * N)(), (C.POINTER(C.c_size_t) * N)()
    for c, instances in enumerate(instances_list):
        cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
        keep += [cols, ptrs, lens]
        inst_pp[c] = C.cast(ptrs, C.POINTER(C.c_void_p))
        lens_pp[c] = C.cast(lens, C.POINTER(C.c_size_t))
    keys = (C.c_void_p * N)(*[pk.h for pk in pks])
    adv = (C.c_void_p * N)(*[d.ptr if d is not None else None for d in d_advice_list])
    errors = []
    phase_fn, tr, keep_cb = _trampolines(synthesize, transcript_object, errors)
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4) if scalars is not None else None
    opts = _ffi.ProofOpts(C.sizeof(_ffi.ProofOpts) if opts_size is None else opts_size, transcript, C.pointer(tr) if tr is not None else None,
                          phase_fn, None, C.c_uint64(seed), sc.ctypes.data if sc is not None else None, sc.shape[0] if sc is not None else 0)
    need = C.c_size_t(0)
    cap = 1 << 22
    buf = (C.c_uint8 * cap)()
    rc = ctx.L.amdzk_create_proof_opts(ctx.h, keys, N, inst_pp, lens_pp, adv, advice_stride or n, C.byref(opts), buf, cap, C.byref(need))
    del keep, keep_cb
    if errors and rc != 0:
        raise errors[0]
    ctx._chk(rc)
    return bytes(buf[: need.value])


def create_proof(ctx, pk, instances, d_advice, seed, advice_stride=None, transcript=TRANSCRIPT_BLAKE2B, synthesize=None):
    """plonk::create_proof(params, pk, &[circuit], &[instances], ChaCha20Rng::seed_from_u64(seed), transcript).
    instances: list of (len, 4) uint64 arrays; d_advice: DeviceBuffer (or anything with .ptr) holding
    num_advice columns of n rows. Returns the proof bytes. `transcript` may be an object (the caller's TranscriptWrite:
    create_proof_opts) instead of a TRANSCRIPT_* number, and `synthesize` the callback of a key with challenge phases."""
    if synthesize is not None or not isinstance(transcript, int):
        tobj = None if isinstance(transcript, int) else transcript
        return create_proof_opts(ctx, [pk], [instances], [d_advice], seed=seed, advice_stride=advice_stride,
                                 transcript=transcript if tobj is None else getattr(tobj, "multiopen", 0), synthesize=synthesize,
                                 transcript_object=tobj)
    n = 1 << pk.desc["k"]
    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4) for c in instances]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
    need = C.c_size_t(0)
    cap = 1 << 20
    buf = (C.c_uint8 * cap)()
    ctx._chk(ctx.L.amdzk_create_proof_ex(ctx.h, pk.h, ptrs, lens, d_advice.ptr if d_advice is not None else None, advice_stride or n,
                                         C.c_uint64(seed), transcript, buf, cap, C.byref(need)))
    return bytes(buf[: need.value])


def create_proof_multi(ctx, pks, instances_list, d_advice_list, seed, advice_stride=None, transcript=TRANSCRIPT_BLAKE2B):
    """plonk::create_proof(params, pk, &[circuit; N], &[instances; N], ChaCha20Rng::seed_from_u64(seed), transcript):
    N instances of the key's circuit in one proof. pks: the key and N - 1 workspace clones of it
    (ProvingKey.clone_workspace); instances_list[c]: instance c's columns; d_advice_list[c]: its advice on the device."""
    N = len(pks)
    assert N >= 1 and len(instances_list) == N and len(d_advice_list) == N
    n = 1 << pks[0].desc["k"]
    keep, inst_pp, lens_pp = [], (C.POINTER(C.c_void_p) * N)(), (C.POINTER(C.c_size_t) * N)()
    for c, instances in enumerate(instances_list):
        cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
        keep += [cols, ptrs, lens]
        inst_pp[c] = C.cast(ptrs, C.POINTER(C.c_void_p))
        lens_pp[c] = C.cast(lens, C.POINTER(C.c_size_t))
    keys = (C.c_void_p * N)(*[pk.h for pk in pks])
    adv = (C.c_void_p * N)(*[d.ptr if d is not None else None for d in d_advice_list])
    need = C.c_size_t(0)
    cap = 1 << 22
    buf = (C.c_uint8 * cap)()
    ctx._chk(ctx.L.amdzk_create_proof_multi(ctx.h, keys, N, inst_pp, lens_pp, adv, advice_stride or n, C.c_uint64(seed), transcript, buf, cap,
                                            C.byref(need)))
    return bytes(buf[: need.value])


def _batch_args(pks, instances_list, d_advice_list, seeds, scalars):
    """What both batch entry points take per proof, as ctypes arrays: (keys, instances, instance_lens, d_advice, seeds array or
    None, scalars pointers or None, scalar count, keep-alive)."""
    N = len(pks)
    assert len(instances_list) == N and len(d_advice_list) == N
    keep, inst_pp, lens_pp = [], (C.POINTER(C.c_void_p) * max(1, N))(), (C.POINTER(C.c_size_t) * max(1, N))()
    for c, instances in enumerate(instances_list):
        cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in instances]
        ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
        lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
        keep += [cols, ptrs, lens]
        inst_pp[c] = C.cast(ptrs, C.POINTER(C.c_void_p))
        lens_pp[c] = C.cast(lens, C.POINTER(C.c_size_t))
    keys = (C.c_void_p * max(1, N))(*[pk.h for pk in pks])
    adv = (C.c_void_p * max(1, N))(*[d.ptr if d is not None else None for d in d_advice_list])
    sd = np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1) if seeds is not None else None
    assert sd is None or sd.shape[0] == N
    sc_ptrs, sc_count = None, 0
    if scalars is not None:
        assert len(scalars) == N
        sc = [np.ascontiguousarray(s_, dtype=np.uint64).reshape(-1, 4) for s_ in scalars]
        sc_ptrs = (C.c_void_p * max(1, N))(*[a.ctypes.data for a in sc])
        sc_count = min(a.shape[0] for a in sc) if sc else 0
        keep += [sc]
    return keys, inst_pp, lens_pp, adv, sd, sc_ptrs, sc_count, keep


def _batch_results(ctx, rc, N, buf, stride, lens_out, st):
    """Per proof its bytes or the AmdzkError of a proof that dropped out; a call refused as a whole raises."""
    msg = ctx.L.amdzk_last_error(ctx.h).decode() if rc != 0 else ""
    if rc != 0 and not msg.startswith("proof "):  # refused as a whole, or ended for all by the device: not one proof's failure
        ctx._chk(rc)
    out = []
    for b in range(N):
        if st[b] == 0:
            out.append(bytes(buf[b * stride: b * stride + lens_out[b]]))
        else:  # the library keeps the first failing proof's message; a later one gets its index and status
            out.append(_ffi.AmdzkError(st[b], msg if msg.startswith("proof %d:" % b) else "proof %d: failed" % b))
    return out


def create_proof_batch(ctx, pks, instances_list, d_advice_list, seeds, advice_stride=None, transcript=TRANSCRIPT_BLAKE2B, scalars=None,
                       opts_size=None, proof_stride=None):
    """amdzk_create_proof_batch: len(pks) independent proofs of one circuit in lock-step on ctx's stream — each step's
    commitments of all proofs in one MSM, one host wait per step. pks: the key and workspace clones of it; instances_list[b],
    d_advice_list[b], seeds[b]: proof b's, as for create_proof. scalars: per proof the caller's Fr::random draws
    (create_proof_with_scalars) instead of seeds. Returns one entry per proof: its bytes — those of create_proof on the
    same workspace — or the AmdzkError of a proof whose witness failed (the others are unaffected). A refused call
    raises. opts_size / proof_stride: what to report to the library (tests)."""
    N = len(pks)
    n = 1 << pks[0].desc["k"] if N else 0
    keys, inst_pp, lens_pp, adv, sd, sc_ptrs, sc_count, keep = _batch_args(pks, instances_list, d_advice_list, seeds, scalars)
    opts = _ffi.BatchOpts(C.sizeof(_ffi.BatchOpts) if opts_size is None else opts_size, transcript,
                          sd.ctypes.data if sd is not None and sd.size else None, sc_ptrs, sc_count)
    stride = proof_stride if proof_stride is not None else (int(ctx.L.amdzk_proof_size(pks[0].h, transcript)) if N else 0)
    buf = (C.c_uint8 * max(1, stride * N))()
    lens_out = (C.c_size_t * max(1, N))()
    st = (C.c_int * max(1, N))()
    rc = ctx.L.amdzk_create_proof_batch(ctx.h, keys, N, inst_pp, lens_pp, adv, advice_stride or n, C.byref(opts), buf, stride, lens_out, st)
    del keep
    return _batch_results(ctx, rc, N, buf, stride, lens_out, st)


def create_proof_batch_opts(ctx, pks, instances_list, d_advice_list, seeds=None, scalars=None, transcript=TRANSCRIPT_BLAKE2B, synthesize=None,
                            transcript_objects=None, advice_stride=None, opts_size=None, proof_stride=None):
    """amdzk_create_proof_batch_opts: create_proof_batch for keys with challenge phases, proofs with the caller's transcript
    and different circuits on one ParamsKZG. pks[b] / instances_list[b] / d_advice_list[b] / seeds[b] / scalars[b]: proof b's.
    synthesize(phase, wanted (n_proofs,) uint8, challenges (n_proofs, stride, 4) uint64 Montgomery, hip_stream): called once
    per phase >= 1 for the whole batch, fills that phase's columns of every wanted proof on the device; returns None, a list of
    per-proof codes (non-zero drops that proof alone) or a non-zero int (drops every wanted proof). transcript_objects: None,
    or per proof None (the built-in `transcript`) or the caller's TranscriptWrite (create_proof_opts) — that proof's entry is
    then b"". Returns what create_proof_batch returns: per proof its bytes or the AmdzkError of a proof that dropped out. An
    exception in a callback is raised once the library has returned. opts_size / proof_stride: what to report (tests)."""
    N = len(pks)
    n = 1 << pks[0].desc["k"] if N else 0
    keys, inst_pp, lens_pp, adv, sd, sc_ptrs, sc_count, keep = _batch_args(pks, instances_list, d_advice_list, seeds, scalars)
    errors = []
    guard = _guard(errors)
    phase_fn = _ffi.BATCH_PHASE_FN()
    if synthesize is not None:
        def on_phase(_user, phase, nproofs, wanted, ch, stride, proof_rc, stream):
            w = np.array([wanted[b] for b in range(nproofs)], dtype=np.uint8)
            chal = np.array([ch[i] for i in range(4 * nproofs * stride)], dtype=np.uint64).reshape(nproofs, stride, 4)
            r = synthesize(phase, w, chal, stream)
            if r is None or isinstance(r, int):
                return r
            for b, code in enumerate(r):
                proof_rc[b] = int(code or 0)
            return 0
        phase_fn = _ffi.BATCH_PHASE_FN(guard(on_phase))
    tr_pp = None
    if transcript_objects is not None:
        assert len(transcript_objects) == N
        tr_pp = (C.POINTER(_ffi.Transcript) * max(1, N))()
        for b, tobj in enumerate(transcript_objects):
            if tobj is not None:
                tr, keep_t = _write_transcript(tobj, errors)
                keep += keep_t
                tr_pp[b] = C.pointer(tr)
    opts = _ffi.BatchProofOpts(C.sizeof(_ffi.BatchProofOpts) if opts_size is None else opts_size, transcript,
                               sd.ctypes.data if sd is not None and sd.size else None, sc_ptrs, sc_count, tr_pp, phase_fn, None)
    own = [transcript_objects is not None and transcript_objects[b] is not None for b in range(N)]
    sizes = [int(ctx.L.amdzk_proof_size(pks[b].h, transcript)) for b in range(N) if not own[b]]
    stride = proof_stride if proof_stride is not None else max(sizes + [0])
    buf = (C.c_uint8 * max(1, stride * N))()
    lens_out = (C.c_size_t * max(1, N))()
    st = (C.c_int * max(1, N))()
    rc = ctx.L.amdzk_create_proof_batch_opts(ctx.h, keys, N, inst_pp, lens_pp, adv, advice_stride or n, C.byref(opts), buf, stride, lens_out, st)
    del keep
    if errors:
        raise errors[0]
    return _batch_results(ctx, rc, N, buf, stride, lens_out, st)


CHECK_GATE, CHECK_LOOKUP, CHECK_COPY = 0, 1, 2  # include/amdzk.h AMDZK_CHECK_*
CheckFailure = collections.namedtuple("CheckFailure", "kind index first_row count")


class WitnessReport:
    """What check_witness found: `failures`, one CheckFailure per failing constraint (kind: CHECK_GATE / CHECK_LOOKUP /
    CHECK_COPY; index: the gate polynomial, the lookup, the position in the permutation's columns; first_row: the smallest
    failing row; count: how many rows fail), ordered by kind and index; `ok` iff there is none."""

    def __init__(self, failures):
        self.failures = list(failures)

    @property
    def ok(self):
        return not self.failures

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "WitnessReport(ok)" if self.ok else "WitnessReport(%r)" % (self.failures,)


def check_witness(ctx, pk, instances, d_advice, theta_seed=0, challenges=None, advice_stride=None):
    """amdzk_check_witness: MockProver::verify's constraint checks on the device — every gate polynomial on the usable
    rows, every lookup input against its table, every copy constraint (include/amdzk.h has the exact semantics).
    instances / d_advice / advice_stride as for create_proof (the advice is read unblinded); theta_seed seeds the theta
    that compresses multi-expression lookups; challenges: (num_challenges, 4) uint64 Montgomery for a key with challenge
    phases. Overwrites the key's per-proof workspace. One call of the library, with room for every constraint of the key
    (gate polynomials + lookups + permutation columns). Returns a WitnessReport."""
    n = 1 << pk.desc["k"]
    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4) for c in instances]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
    ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4) if challenges is not None else None
    opts = _ffi.CheckOpts(C.sizeof(_ffi.CheckOpts), C.c_uint64(theta_seed), ch.ctypes.data if ch is not None and ch.size else None,
                          ch.shape[0] if ch is not None else 0)
    cap = len(pk.desc["gates"]) + len(pk.desc["lookups"]) + len(pk.desc["permutation_columns"])
    buf = (_ffi.CheckFailure * max(1, cap))()
    total = C.c_size_t(0)
    ctx._chk(ctx.L.amdzk_check_witness(ctx.h, pk.h, ptrs, lens, d_advice.ptr if d_advice is not None else None, advice_stride or n,
                                       C.byref(opts), buf, cap, C.byref(total)))
    assert total.value <= cap
    return WitnessReport(CheckFailure(f.kind, f.index, f.first_row, f.count) for f in buf[:total.value])


# include/amdzk.h AMDZK_PROOF_*
PROOF_WELL_FORMED, PROOF_BAD_LENGTH, PROOF_BAD_POINT, PROOF_BAD_SCALAR, PROOF_BAD_INSTANCE, PROOF_BAD_TRANSCRIPT = 0, 1, 2, 3, 4, 5
PROOF_STATUS_NAMES = ("WELL_FORMED", "BAD_LENGTH", "BAD_POINT", "BAD_SCALAR", "BAD_INSTANCE", "BAD_TRANSCRIPT")
ProofStatus = collections.namedtuple("ProofStatus", "status offset")


class Guard:
    """What verify_proof / verify_proofs return, upstream's GuardKZG up to the pairing: `lhs`, `rhs` — (8,) uint64 G1Affine
    words, Montgomery, all zero = the identity — with "every well-formed proof is valid iff e(lhs, [s]_2) = e(rhs, [1]_2)",
    and `statuses`, one ProofStatus per proof (malformed proofs are in neither sum). The pairing is the caller's."""

    def __init__(self, lhs, rhs, statuses):
        self.lhs, self.rhs, self.statuses = lhs, rhs, list(statuses)
        self.errors = []  # exceptions raised inside the caller's read transcripts (their proofs are PROOF_BAD_TRANSCRIPT)

    @property
    def well_formed(self):
        return all(s.status == PROOF_WELL_FORMED for s in self.statuses)

    def __repr__(self):
        return "Guard(statuses=%r)" % (self.statuses,)


def _verify_args(instances_list, proofs, transcript, n_circuits, combine_seed, combine_scalars, opts_size, transcripts=None, errors=None):
    """The arguments amdzk_verify_proofs and amdzk_verify_proofs_decide share: (instances, instance_lens, proofs, proof_lens,
    opts, statuses, keep-alive). transcripts: None, or per proof None / a TranscriptRead object (ffi.read_transcript), whose
    exceptions land in `errors`; a proof that has one may be None."""
    B, N = len(proofs), n_circuits
    proofs = [b"" if p is None else p for p in proofs]
    assert len(instances_list) == B
    keep, inst_pp, lens_pp = [], (C.POINTER(C.c_void_p) * max(1, B * N))(), (C.POINTER(C.c_size_t) * max(1, B * N))()
    for b, per_proof in enumerate(instances_list):
        per_circuit = [per_proof] if N == 1 else list(per_proof)
        assert len(per_circuit) == N
        for c, instances in enumerate(per_circuit):
            cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in instances]
            ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
            lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
            keep += [cols, ptrs, lens]
            inst_pp[b * N + c] = C.cast(ptrs, C.POINTER(C.c_void_p))
            lens_pp[b * N + c] = C.cast(lens, C.POINTER(C.c_size_t))
    bufs = [(C.c_uint8 * max(1, len(p))).from_buffer_copy(bytes(p) if len(p) else b"\0") for p in proofs]
    pp = (C.c_void_p * max(1, B))(*[C.addressof(b_) for b_ in bufs])
    pl = (C.c_size_t * max(1, B))(*[len(p) for p in proofs])
    sc = np.ascontiguousarray(combine_scalars, dtype=np.uint64).reshape(-1, 4) if combine_scalars is not None else None
    assert sc is None or sc.shape[0] == B
    trs = None
    if transcripts is not None:
        assert len(transcripts) == B
        trs = (C.POINTER(_ffi.TranscriptRead) * max(1, B))()
        for b, tobj in enumerate(transcripts):
            if tobj is not None:
                tr, alive = _ffi.read_transcript(tobj, errors if errors is not None else [])
                trs[b] = C.pointer(tr)
                keep.append(alive)
    opts = _ffi.VerifyOpts(C.sizeof(_ffi.VerifyOpts) if opts_size is None else opts_size, transcript, N, C.c_uint64(combine_seed),
                           sc.ctypes.data if sc is not None else None, trs)
    st = (_ffi.ProofStatus * max(1, B))()
    keep += [bufs, sc, trs]
    return inst_pp, lens_pp, pp, pl, opts, st, keep


def verify_proofs(ctx, pk, instances_list, proofs, transcript=TRANSCRIPT_BLAKE2B, n_circuits=1, combine_seed=0, combine_scalars=None,
                  opts_size=None, transcripts=None):
    """amdzk_verify_proofs (amdzk_verify_proofs_vk when pk is a VerifyingKey): plonk::verify_proof for a batch up to the one
    pairing. proofs[b]: bytes; instances_list[b]: proof
    b's instance columns as for create_proof — or, with n_circuits > 1, a list of n_circuits such lists (create_proof_multi).
    combine_scalars: (len(proofs), 4) uint64 Montgomery weights of the caller's; else they are drawn from combine_seed, which
    must then be unpredictable to whoever made the proofs (a single proof has weight 1). Returns a Guard; a refused call raises.
    transcripts: None, or per proof None (the bytes proofs[b]) or the caller's TranscriptRead object — common_scalar((4,) uint64),
    read_point() -> (8,), read_scalar() -> (4,), squeeze_challenge() -> (4,), Montgomery words; proofs[b] may then be None and of
    `transcript` only MULTIOPEN_GWC counts. An exception in a method makes that proof PROOF_BAD_TRANSCRIPT; Guard.errors keeps them.
    So does a squeezed challenge that is not below r, and a squeezed x that is 0 or has x^n = 1 (no exception is kept for those).
    opts_size: amdzk_verify_opts.size to report (tests)."""
    B = len(proofs)
    errors = []
    inst_pp, lens_pp, pp, pl, opts, st, keep = _verify_args(instances_list, proofs, transcript, n_circuits, combine_seed, combine_scalars, opts_size,
                                                            transcripts, errors)
    pair = np.zeros(16, dtype=np.uint64)
    fn = ctx.L.amdzk_verify_proofs_vk if isinstance(pk, VerifyingKey) else ctx.L.amdzk_verify_proofs
    ctx._chk(fn(ctx.h, pk.h, B, inst_pp, lens_pp, pp, pl, C.byref(opts), st, pair.ctypes.data))
    del keep
    g = Guard(pair[:8].copy(), pair[8:].copy(), [ProofStatus(s.status, s.offset) for s in st[:B]])
    g.errors = errors
    return g


DECIDE_COMBINED = 1  # AMDZK_DECIDE_COMBINED
DECIDE_RUN = 16      # AMDZK_DECIDE_RUN


def decide_proofs(ctx, pk, vparams, instances_list, proofs, transcript=TRANSCRIPT_BLAKE2B, n_circuits=1, combined=False, combine_seed=0,
                  combine_scalars=None, opts_size=None, transcripts=None):
    """amdzk_verify_proofs_decide (amdzk_verify_proofs_decide_vk when pk is a VerifyingKey): plonk::verify_proof for a batch WITH
    the pairing. vparams: kzg.ParamsVerifierKZG of the SRS
    the key was made on. combined=False: every proof by itself (SingleStrategy; deterministic, combine_* ignored);
    combined=True: upstream's BatchVerifier — one check with the weights of combine_seed / combine_scalars, which must be
    unpredictable to whoever made the proofs; every well-formed proof gets that check's result. Returns (verdicts, statuses):
    a list of bool and a list of ProofStatus; a malformed proof has verdict False. A refused call raises. transcripts: as for
    verify_proofs."""
    B = len(proofs)
    inst_pp, lens_pp, pp, pl, opts, st, keep = _verify_args(instances_list, proofs, transcript, n_circuits, combine_seed, combine_scalars, opts_size,
                                                            transcripts)
    verdicts = np.zeros(max(1, B), np.uint8)
    n_valid = C.c_size_t(0)
    fn = ctx.L.amdzk_verify_proofs_decide_vk if isinstance(pk, VerifyingKey) else ctx.L.amdzk_verify_proofs_decide
    ctx._chk(fn(ctx.h, pk.h, vparams.s_g2.h, vparams.g2.h, DECIDE_COMBINED if combined else 0, B, inst_pp, lens_pp,
                pp, pl, C.byref(opts), st, verdicts.ctypes.data, C.byref(n_valid)))
    del keep
    out = [bool(v) for v in verdicts[:B]]
    assert sum(out) == n_valid.value
    return out, [ProofStatus(s.status, s.offset) for s in st[:B]]


class VerifyItem:
    """One member of a mixed batch (amdzk_verify_item): `key` a ProvingKey or a VerifyingKey, `instances` the proof's instance
    columns as for create_proof (with n_circuits > 1 a list of n_circuits such lists), `proof` the bytes, `transcript` the kind
    flags of those bytes. reader: the caller's TranscriptRead object (verify_proofs); `proof` may then be None and of
    `transcript` only MULTIOPEN_GWC counts."""

    def __init__(self, key, instances, proof, transcript=TRANSCRIPT_BLAKE2B, n_circuits=1, reader=None):
        self.key, self.instances, self.proof, self.transcript, self.n_circuits, self.reader = key, instances, proof, transcript, n_circuits, reader


def _mixed_args(items, combine_seed, combine_scalars, opts_size, errors):
    """(amdzk_verify_item array, opts, statuses, keep-alive) of the two mixed calls."""
    B = len(items)
    arr = (_ffi.VerifyItem * max(1, B))()
    keep = []
    for b, it in enumerate(items):
        N = it.n_circuits or 1
        per_circuit = [it.instances] if N == 1 else list(it.instances)
        assert len(per_circuit) == N
        inst_pp, lens_pp = (C.POINTER(C.c_void_p) * N)(), (C.POINTER(C.c_size_t) * N)()
        for c, instances in enumerate(per_circuit):
            cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in instances]
            ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
            lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
            keep += [cols, ptrs, lens]
            inst_pp[c] = C.cast(ptrs, C.POINTER(C.c_void_p))
            lens_pp[c] = C.cast(lens, C.POINTER(C.c_size_t))
        proof = b"" if it.proof is None else bytes(it.proof)
        buf = (C.c_uint8 * max(1, len(proof))).from_buffer_copy(proof if len(proof) else b"\0")
        tr = None
        if it.reader is not None:
            t, alive = _ffi.read_transcript(it.reader, errors)
            tr = C.pointer(t)
            keep.append(alive)
        is_vk = isinstance(it.key, VerifyingKey)
        arr[b] = _ffi.VerifyItem(None if is_vk else it.key.h, it.key.h if is_vk else None, it.transcript, it.n_circuits, inst_pp, lens_pp,
                                 C.addressof(buf), len(proof), tr)
        keep += [inst_pp, lens_pp, buf, tr]
    sc = np.ascontiguousarray(combine_scalars, dtype=np.uint64).reshape(-1, 4) if combine_scalars is not None else None
    assert sc is None or sc.shape[0] == B
    opts = _ffi.VerifyMixedOpts(C.sizeof(_ffi.VerifyMixedOpts) if opts_size is None else opts_size, C.c_uint64(combine_seed),
                                sc.ctypes.data if sc is not None else None)
    keep.append(sc)
    return arr, opts, (_ffi.ProofStatus * max(1, B))(), keep


def verify_proofs_mixed(ctx, items, combine_seed=0, combine_scalars=None, opts_size=None):
    """amdzk_verify_proofs_mixed: verify_proofs over VerifyItems that each bring their own key — different circuits, k, transcript
    kinds and proof sizes in one call, all keys made over one G. Returns a Guard with sum_b rho_b (L_b, R_b); statuses[b] is what
    verify_proofs gives item b under its key. A refused call raises ("verify_proofs_mixed: ...")."""
    errors = []
    arr, opts, st, keep = _mixed_args(items, combine_seed, combine_scalars, opts_size, errors)
    pair = np.zeros(16, dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_verify_proofs_mixed(ctx.h, arr, len(items), C.byref(opts), st, pair.ctypes.data))
    del keep
    g = Guard(pair[:8].copy(), pair[8:].copy(), [ProofStatus(s.status, s.offset) for s in st[:len(items)]])
    g.errors = errors
    return g


def decide_proofs_mixed(ctx, vparams, items, combined=False, combine_seed=0, combine_scalars=None, opts_size=None):
    """amdzk_verify_proofs_decide_mixed: decide_proofs over VerifyItems with their own keys; one decode launch and one pairing
    launch for the whole batch. Returns (verdicts, statuses) as decide_proofs does."""
    B = len(items)
    arr, opts, st, keep = _mixed_args(items, combine_seed, combine_scalars, opts_size, [])
    verdicts = np.zeros(max(1, B), np.uint8)
    n_valid = C.c_size_t(0)
    ctx._chk(ctx.L.amdzk_verify_proofs_decide_mixed(ctx.h, vparams.s_g2.h, vparams.g2.h, DECIDE_COMBINED if combined else 0, arr, B, C.byref(opts), st,
                                                    verdicts.ctypes.data, C.byref(n_valid)))
    del keep
    out = [bool(v) for v in verdicts[:B]]
    assert sum(out) == n_valid.value
    return out, [ProofStatus(s.status, s.offset) for s in st[:B]]


def _kind_or_object(transcript, multiopen):
    """transcript= of verify_proof / decide_proof: the kind flags, or the caller's TranscriptRead object (then `multiopen`,
    0 or MULTIOPEN_GWC, names the opening scheme). Returns (flags, transcripts argument)."""
    if isinstance(transcript, (int, np.integer)):
        return int(transcript) | multiopen, None
    return multiopen | getattr(transcript, "multiopen", 0), [transcript]


def decide_proof(ctx, pk, vparams, instances, proof, transcript=TRANSCRIPT_BLAKE2B, n_circuits=1, multiopen=0):
    """plonk::verify_proof(params, vk, SingleStrategy, &[instances], transcript).is_ok(): True iff the proof is valid. Raises
    ValueError naming the status and the offset when the proof is malformed, as verify_proof does. transcript: the kind flags
    of the bytes `proof`, or the caller's TranscriptRead object (verify_proofs; `proof` may be None, multiopen = MULTIOPEN_GWC
    for GWC)."""
    flags, trs = _kind_or_object(transcript, multiopen)
    verdicts, statuses = decide_proofs(ctx, pk, vparams, [instances], [proof], transcript=flags, n_circuits=n_circuits, transcripts=trs)
    s = statuses[0]
    if s.status != PROOF_WELL_FORMED:
        raise ValueError("malformed proof: status %d (%s), offset %d" % (s.status, PROOF_STATUS_NAMES[s.status], s.offset))
    return verdicts[0]


def verify_proof(ctx, pk, instances, proof, transcript=TRANSCRIPT_BLAKE2B, n_circuits=1, multiopen=0):
    """plonk::verify_proof(params, vk, SingleStrategy, &[instances], transcript) up to the pairing: one proof, weight 1.
    Raises ValueError naming the status and the offset when the proof is malformed; returns its Guard otherwise (the proof
    is valid iff the caller's pairing check of guard.lhs / guard.rhs holds). transcript: as for decide_proof."""
    flags, trs = _kind_or_object(transcript, multiopen)
    g = verify_proofs(ctx, pk, [instances], [proof], transcript=flags, n_circuits=n_circuits, transcripts=trs)
    s = g.statuses[0]
    if s.status != PROOF_WELL_FORMED:
        raise ValueError("malformed proof: status %d (%s), offset %d" % (s.status, PROOF_STATUS_NAMES[s.status], s.offset))
    return g


def proof_size_multi(ctx, pk, n_circuits, transcript=TRANSCRIPT_BLAKE2B):
    fn = ctx.L.amdzk_vk_proof_size_multi if isinstance(pk, VerifyingKey) else ctx.L.amdzk_proof_size_multi
    return int(fn(pk.h, n_circuits, transcript))


def proof_size(ctx, pk, transcript=TRANSCRIPT_BLAKE2B):
    return proof_size_multi(ctx, pk, 1, transcript) if isinstance(pk, VerifyingKey) else int(ctx.L.amdzk_proof_size(pk.h, transcript))


def proof_random_count(ctx, pk):
    return int(ctx.L.amdzk_proof_random_count(pk.h))


def create_proof_with_scalars(ctx, pk, instances, d_advice, scalars, advice_stride=None, transcript=TRANSCRIPT_BLAKE2B):
    """create_proof with the caller's own RngCore: `scalars` = the Fr::random draws in upstream order."""
    n = 1 << pk.desc["k"]
    cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1, 4) for c in instances]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data if c.size else None for c in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[c.shape[0] for c in cols])
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    need = C.c_size_t(0)
    cap = 1 << 20
    buf = (C.c_uint8 * cap)()
    ctx._chk(ctx.L.amdzk_create_proof_scalars(ctx.h, pk.h, ptrs, lens, d_advice.ptr if d_advice is not None else None, advice_stride or n,
                                              sc.ctypes.data, sc.shape[0], transcript, buf, cap, C.byref(need)))
    return bytes(buf[: need.value])
