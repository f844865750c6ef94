"""GPU: the gate compiler (program.hip emit_tree, emit_compressed, finalize_limb_program) and the three interpreters that
run its output (expr_eval_limbs_kernel for h(X), expr_eval_kernel for the lookups' compressed expressions, expr_check_kernel
for the witness check) on circuits whose expressions reach every threshold of the lazy reduction from both sides
(tests/bound_circuits.py).

Two kinds of assertion. (1) The finalised h(X) program of the very key the device runs holds, gate by gate, the
instructions bound_circuits derived by hand, passes the independent walker, and the walker's margins sit on the pass's
thresholds — so every decision was executed, not merely possible. (2) What the device computes with those programs equals
the oracle bit for bit: quotient pieces in both coset modes at the interpreter's extreme words (the machinery of
test_gpu_quotient_operands.py), whole proofs, the permuted lookup columns, the witness check's report.

A program's stack depth is bounded by keygen (the LDS of the interpreters): the deepest circuit that fits proves like
any other, and one level more is refused by name."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import bound_circuits as BC  # noqa: E402
import limb_program_check as LC  # noqa: E402
import plonk_ref as PR  # noqa: E402
import witness_check_ref as W  # noqa: E402
from test_gpu_quotient_operands import INV32, MONT_INV, TAU, WORDS, by_kind, make_challenges, make_polys, to_field_ints  # noqa: E402
from test_limb_program import ops, run_length  # noqa: E402

pytestmark = pytest.mark.gpu
R = zu.R
REPR = 99
NAMES = list(BC.CIRCUITS)
POLYSETS = ["word_r_minus_1", "word_T_2p232_minus_1", "word_alt_even_limbs", "dealt0", "arbitrary0"]
CHALLENGES = ["tbg_rm1.y_rm1", "tbg_random.y_random", "tbg_one.y_one"]
GROUP_LIM = 169.0 * 30.0
UNSUPPORTED = -5
# a fixed column that holds this field element on every row is the constant polynomial whose coset values the limb
# interpreter loads as the word r - 1 (test_gpu_quotient_operands.py: the Montgomery word W / 32)
EXTREME_FIXED = WORDS["r_minus_1"] * INV32 % R * MONT_INV % R


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def h_program(pkg, pk):
    n = C.c_size_t(0)
    assert pkg.lib().amdzk_pk_h_program(pk.h, None, 0, C.byref(n)) == 0
    words = np.zeros(n.value, dtype=np.uint32)
    assert pkg.lib().amdzk_pk_h_program(pk.h, words.ctypes.data, n.value, C.byref(n)) == 0
    return [int(w) for w in words]


def terms_of(words):
    """{j: the instructions of term j} of a finalised program (the grouping reorders terms; WACC names each)."""
    out, cur = {}, []
    for w in words:
        op = LC.NAME[w >> 24]
        if op == "WACC":
            out[w & 0x7FFFFF] = cur
            cur = []
        elif op != "WFLUSH":
            cur.append(w)
    assert not cur
    return out


def fr_cols(oracle, cols, n):
    return np.stack([zu.ints_to_fr(oracle, col) for col in cols]) if cols else np.zeros((0, n, 4), np.uint64)


class Keys:
    """Per circuit, made once for the module: the oracle's key, and the device's keys in both coset modes, each with the
    h(X) program cut into the default six pieces and (AMDZK_H_PARTS=1 at keygen) in one piece — only in one piece does a
    group grow to its limit or hold two carries; only cut does a piece end inside a group. `extreme`: the same circuit
    with every fixed column (selectors too) the constant the interpreter loads as r - 1."""

    def __init__(self, ctx, pkg, plonk, oracle):
        self.ctx, self.pkg, self.plonk, self.oracle = ctx, pkg, plonk, oracle
        self.made, self.params, self.oracle_polys = {}, {}, {}

    def srs(self, k):
        if k not in self.params:
            g, gl = zu.test_srs(self.oracle, k, TAU)
            self.params[k] = self.pkg.kzg.ParamsKZG(self.ctx, k, g=g, g_lagrange=gl)
        return self.params[k]

    def keygen(self, c, flags=None, parts=None):
        before = os.environ.get("AMDZK_H_PARTS")
        if parts is not None:
            os.environ["AMDZK_H_PARTS"] = str(parts)
        try:
            return self.plonk.ProvingKey(self.ctx, self.srs(c.k), c.desc, fr_cols(self.oracle, c.fixed, c.n), c.assembly.mapping,
                                         zu.fr_from_int(REPR), flags=flags)
        finally:
            if parts is not None:
                if before is None:
                    del os.environ["AMDZK_H_PARTS"]
                else:
                    os.environ["AMDZK_H_PARTS"] = before

    def get(self, name, extreme=False):
        if (name, extreme) not in self.made:
            c = BC.CIRCUITS[name](self.plonk, **({"extreme_fixed": EXTREME_FIXED} if extreme else {}))
            dev = {(parts, flags): self.keygen(c, flags, parts) for parts in (None, 1) for flags in (0, self.plonk.KEYGEN_FULL_COSETS)}
            opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
            self.made[(name, extreme)] = (c, dev, opk)
        return self.made[(name, extreme)]

    def polys(self, name, polyset):
        if (name, polyset) not in self.oracle_polys:
            c = self.get(name)[0]
            a = make_polys(c.desc, c.n, polyset)
            ints = to_field_ints(a)
            self.oracle_polys[(name, polyset)] = (a, by_kind(c.desc, [ints[i * c.n:(i + 1) * c.n] for i in range(a.shape[0])]))
        return self.oracle_polys[(name, polyset)]

    def free(self):
        for _, dev, _ in self.made.values():
            for pk in dev.values():
                pk.free()
        for p in self.params.values():
            p.free()


@pytest.fixture(scope="module")
def keys(ctx, pkg, plonk, oracle):
    k = Keys(ctx, pkg, plonk, oracle)
    yield k
    k.free()


# ------------------------------------------------------------------------------------ (1) the programs the device runs
def walked(pkg, pk):
    words = h_program(pkg, pk)
    LC.check(words)
    return words, dict(LC.check.margins), LC.check.pieces


@pytest.mark.parametrize("name", NAMES)
def test_every_gate_compiles_to_the_instructions_derived_by_hand(pkg, plonk, keys, name):
    c, dev, _ = keys.get(name)
    for (parts, flags), pk in dev.items():
        words, _, pieces = walked(pkg, pk)
        assert pieces == 1 if parts == 1 else 1 <= pieces <= 6
        terms = terms_of(words)
        assert len(terms) >= len(c.gate_names)
        for g, (gate, want) in enumerate(zip(c.gate_names, c.gate_expect)):  # the gates are the first terms
            assert run_length(ops(terms[g])) == want, "%s, gate %d (%s), %r pieces" % (name, g, gate, parts)
    assert h_program(pkg, dev[(None, 0)]) == h_program(pkg, dev[(None, plonk.KEYGEN_FULL_COSETS)])  # the mode is not the program's


def test_margins_sit_on_the_thresholds_of_the_pass(pkg, plonk, keys):
    """Reached from below, by programs the tests below run on the device: a product of 152 (160 reduces), a negated sum of
    8 (9 reduces), a value of 8 sinking (above 8 reduces), a sum of 40 (above 40 reduces), five un-carried terms (the
    sixth carries), a group flushed within one term of its limit, and the h(X) program in pieces that end inside a group."""
    words, m, _ = walked(pkg, keys.get("thresholds")[1][(None, 0)])
    assert 152.0 <= m["product"] < 160.0 and 8.0 <= m["neg_big"] < 9.0 and m["sink"] == 8.0 and m["sum"] == 40.0
    assert 1.0 < m["neg"] < 2.0  # a reduced value, negated with the small constant
    hist = set(ops(words))
    # a lookup term subtracts one product from another, and a product's bound is exactly 2: SUB_BIG at its lower end
    words, m, _ = walked(pkg, keys.get("lookups7")[1][(1, 0)])
    hist |= set(ops(words))
    assert m["sub_big"] == 2.0 and m["sub"] == 0.0 and m["uncarried"] == 5
    group, run, carries = {}, 0, []
    for w in words:
        if LC.NAME[w >> 24] == "WACC":
            run += 1
            carries.append(bool(w & (1 << 23)))
        elif LC.NAME[w >> 24] == "WFLUSH":
            group[w & 7] = (run, sum(carries))
            run, carries = 0, []
    assert group[0][0] >= 13 and group[0][1] >= 2 and group[2][0] >= 13 and group[2][1] >= 2, group  # (terms, carries) of l_0 and l_active
    # 150 plain terms of bound 40 in one piece: the group is split at its limit
    words, m, pieces = walked(pkg, keys.get("many150")[1][(1, 0)])
    plain = [w & 0xFFFFFF for w in words if LC.NAME[w >> 24] == "WFLUSH" and w & 7 == 4]
    assert pieces == 1 and len(plain) == 2 and GROUP_LIM - 40.0 < m["wflush"] <= GROUP_LIM and m["uncarried"] == 5 and m["sum"] == 40.0
    # ... and in six pieces: a piece ends inside the plain group (the next piece's first flush is the same group's)
    words, m, pieces = walked(pkg, keys.get("many150")[1][(None, 0)])
    flushes = [w & 0xFFFFFF for w in words if LC.NAME[w >> 24] == "WFLUSH"]
    assert pieces == 6 and any(a & 7 == 4 and b == (4 | 16) for a, b in zip(flushes, flushes[1:])), flushes
    for name in ("branches", "long_sum", "rotations7"):
        hist |= set(ops(h_program(pkg, keys.get(name)[1][(None, 0)])))
    assert hist >= {"REDUCE", "SUB_BIG", "NEG_BIG", "NEG", "ADD", "MUL", "SQR", "PUSH_COL", "PUSH_CONST", "ADD_COL", "SUB_COL", "MUL_COL",
                    "ADD_CONST", "MUL_CONST", "PICK", "NIP", "WACC", "WFLUSH"}
    assert "MUL_HOT" not in hist and "ACC" not in hist


# ---------------------------------------------------------------------------------------------- (2) device against oracle
@pytest.mark.parametrize("chal", CHALLENGES)
@pytest.mark.parametrize("polyset", POLYSETS)
@pytest.mark.parametrize("name", NAMES)
def test_quotient_pieces_equal_the_oracle(keys, plonk, name, polyset, chal):
    """Both coset modes, the program whole and in pieces; at the word r - 1 also with every fixed column and selector the
    constant polynomial that makes the interpreter load r - 1 for it."""
    theta, beta, gamma, y = make_challenges(chal, POLYSETS.index(polyset))
    ch = [zu.fr_from_int(v) for v in (theta, beta, gamma, y)]
    a, polys = keys.polys(name, polyset)
    for extreme in ((False, True) if polyset == "word_r_minus_1" else (False,)):
        c, dev, opk = keys.get(name, extreme)
        num = PR.quotient_numerator(opk, polys, theta, beta, gamma, y)
        want = {0: PR.quotient_pieces_on_cosets(opk, polys, theta, beta, gamma, y, numerator=num),
                plonk.KEYGEN_FULL_COSETS: PR.quotient_pieces(opk, polys, theta, beta, gamma, y, numerator=num)}
        for (parts, flags), pk in dev.items():
            got = pk.quotient_eval(a, *ch)
            assert got.shape == (c.desc["cs_degree"] - 1, c.n, 4)
            assert [to_field_ints(p) for p in got] == want[flags], \
                "%s %s %s: pieces differ from the oracle's (flags %d, pieces %r, extreme fixed columns %r)" % (name, polyset, chal, flags, parts, extreme)


class Witness:
    def __init__(self, ctx, oracle, c):
        self.ctx, self.oracle, self.c = ctx, oracle, c
        self.d_adv = ctx.alloc(len(c.advice) * c.n * 32)
        self.inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]

    def upload(self, advice=None):
        self.d_adv.upload(fr_cols(self.oracle, self.c.advice if advice is None else advice, self.c.n))
        return self.d_adv


@pytest.mark.parametrize("name", NAMES)
def test_proofs_equal_the_oracle(ctx, plonk, oracle, keys, name):
    c, dev, opk = keys.get(name)
    wit = Witness(ctx, oracle, c)
    d_adv = wit.upload()
    want = PR.create_proof(opk, c.instances, c.advice, seed=41)
    assert PR.verify_proof(opk, c.instances, want)
    for (parts, flags), pk in dev.items():
        assert plonk.create_proof(ctx, pk, wit.inst, d_adv, seed=41) == want, "%s: flags %d, pieces %r" % (name, flags, parts)
    pk = dev[(None, 0)]
    if name == "branches":
        assert plonk.create_proof(ctx, pk, wit.inst, d_adv, seed=42, transcript=plonk.TRANSCRIPT_KECCAK256_EVM) == \
            PR.create_proof(opk, c.instances, c.advice, seed=42, transcript="evm")
    if name == "lookups7":
        assert plonk.create_proof(ctx, pk, wit.inst, d_adv, seed=43, transcript=plonk.MULTIOPEN_GWC) == \
            PR.create_proof(opk, c.instances, c.advice, seed=43, multiopen="gwc")
    wit.d_adv.free()


def test_compressed_lookup_columns_equal_their_definition(ctx, plonk, oracle, keys):
    """The Lagrange-domain interpreter's own output, where it happens: A' is the sorted compressed input and S' a
    permutation of the compressed table on the usable rows, theta-folded over one, two and three expressions of bounds up
    to 12, a negated and a scaled one among them."""
    c, dev, opk = keys.get("lookups7")
    wit = Witness(ctx, oracle, c)
    pk = dev[(None, 0)]
    proof = plonk.create_proof(ctx, pk, wit.inst, wit.upload(), seed=44)
    assert proof == PR.create_proof(opk, c.instances, c.advice, seed=44)
    polys = [zu.fr_array_to_ints(np.ascontiguousarray(p)) for p in pk.inspect(0)]
    theta = zu.fr_array_to_ints(np.ascontiguousarray(pk.inspect(1)))[0]
    A, I, L = c.desc["num_advice"], c.desc["num_instance"], len(c.desc["lookups"])
    assert L == 7
    lag = opk.domain.coeff_to_lagrange
    for li, lk in enumerate(c.desc["lookups"]):
        def compressed(exprs, row):
            acc = 0
            for e in exprs:
                acc = (acc * theta + BC.ev(e, row, c.fixed, c.advice, c.n)) % R
            return acc
        a_rows, s_rows = lag(polys[A + I + li])[:c.usable], lag(polys[A + I + L + li])[:c.usable]
        assert a_rows == sorted(compressed(lk["inputs"], row) for row in range(c.usable)), "lookup %d: A'" % li
        assert sorted(s_rows) == sorted(compressed(lk["tables"], row) for row in range(c.usable)), "lookup %d: S'" % li
    wit.d_adv.free()


@pytest.mark.parametrize("name", NAMES)
def test_witness_check_runs_the_same_gates(ctx, plonk, oracle, keys, name):
    """expr_check_kernel on the compiled gates: nothing to report on the satisfying witness; with one cell of every `out`
    column changed, the reference's report."""
    c, dev, _ = keys.get(name)
    wit = Witness(ctx, oracle, c)
    pk = dev[(None, 0)]
    report = lambda adv=None: [tuple(f) for f in plonk.check_witness(ctx, pk, wit.inst, wit.upload(adv)).failures]
    assert report() == [] == W.report(c)
    adv = [list(col) for col in c.advice]
    for i, col in enumerate(c.out_columns):
        row = c.gate_rows[(3 * i + 1) % len(c.gate_rows)]
        adv[col][row] = (adv[col][row] + 1 + i) % R
    want = W.report(c, advice=adv)
    assert sorted({e[1] for e in want if e[0] == W.GATE}) == list(range(len(c.desc["gates"]))), "every gate polynomial must fail"
    assert report(adv) == want
    assert report() == []
    wit.d_adv.free()


def test_challenges_as_operands(ctx, pkg, plonk, oracle, monkeypatch):
    """A phased key: the challenge takes every place a constant can in a fused instruction (its slot of the constant table
    is written per proof). Program as derived, proof bytes equal the harness's, witness check clean and, corrupted, the
    reference's."""
    from test_gpu_phased import Device, expected

    c = BC.phased_circuit(plonk)
    dev = Device(ctx, pkg, plonk, oracle, c)
    words = h_program(pkg, dev.pk)
    LC.check(words)
    terms = terms_of(words)
    for g, (gate, want) in enumerate(zip(c.gate_names, c.gate_expect)):
        assert run_length(ops(terms[g])) == want, "gate %d (%s)" % (g, gate)
    got = dev.prove(seed=51)
    ch = dev.challenges()
    assert got == expected(monkeypatch, dev, dev.opk(), 51, ch)
    chal = np.stack([zu.fr_from_int(v) for v in ch])
    adv = [list(col) for col in dev.adv[0]]
    d_adv = dev.d_adv[0]
    check = lambda a: [tuple(f) for f in plonk.check_witness(ctx, dev.pk, dev.inst[0], d_adv.upload(fr_cols(oracle, a, c.n)), challenges=chal).failures]
    assert check(adv) == [] == W.report(c, advice=adv, challenges=ch)
    for i in range(len(c.gate_names)):
        col = c.desc["num_advice"] - len(c.gate_names) + i
        adv[col][3 + i] = (adv[col][3 + i] + 1) % R
    want = W.report(c, advice=adv, challenges=ch)
    assert [e[1] for e in want if e[0] == W.GATE] == list(range(len(c.gate_names)))
    assert check(adv) == want
    dev.free()


# ------------------------------------------------------------------------------------------------------- (3) stack depth
def refusal(keys, c):
    with pytest.raises(keys.pkg.ffi.AmdzkError) as e:
        keys.keygen(c).free()
    assert e.value.code == UNSUPPORTED
    m = re.search(r"keygen: the (.+) program has stack depth (\d+) \((\d+) bytes of LDS\); depth (\d+) fits this device \((\d+) bytes per workgroup\)",
                  str(e.value))
    assert m, str(e.value)
    return m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5))


def prove_and_check(ctx, plonk, oracle, keys, c):
    """Proof bytes, quotient pieces at the word r - 1 in both modes, and the witness check, against the oracle."""
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    wit = Witness(ctx, oracle, c)
    a = make_polys(c.desc, c.n, "word_r_minus_1")
    ints = to_field_ints(a)
    polys = by_kind(c.desc, [ints[i * c.n:(i + 1) * c.n] for i in range(a.shape[0])])
    theta, beta, gamma, y = make_challenges("tbg_rm1.y_rm1", 0)
    num = PR.quotient_numerator(opk, polys, theta, beta, gamma, y)
    want = {0: PR.quotient_pieces_on_cosets(opk, polys, theta, beta, gamma, y, numerator=num),
            plonk.KEYGEN_FULL_COSETS: PR.quotient_pieces(opk, polys, theta, beta, gamma, y, numerator=num)}
    depth = None
    for flags in want:
        pk = keys.keygen(c, flags)
        depth = LC.check(h_program(keys.pkg, pk))[0]
        assert plonk.create_proof(ctx, pk, wit.inst, wit.upload(), seed=61) == PR.create_proof(opk, c.instances, c.advice, seed=61)
        assert [to_field_ints(p) for p in pk.quotient_eval(a, *[zu.fr_from_int(v) for v in (theta, beta, gamma, y)])] == want[flags]
        assert plonk.check_witness(ctx, pk, wit.inst, wit.upload()).ok and W.report(c) == []
        pk.free()
    wit.d_adv.free()
    return depth


def test_keygen_refuses_a_program_too_deep_for_the_lds_and_proves_the_deepest_that_fits(ctx, plonk, oracle, keys):
    """The limb interpreter keeps depth - 1 stack slots of 128 x 36 bytes behind 17 x 128 x 8 bytes of wide accumulator,
    the Lagrange-domain interpreters depth + 1 slots of 128 x 32 bytes. Every expression of a circuit lands in h(X) too,
    whose slots are the larger ones and whose lookup term holds two values below a compressed input: h(X) decides. A
    right-nested sum of `levels` products holds `levels` values at once (levels + 2 as a lookup input). The limit is the
    one the refusal reports for this device; the refused keygen launches nothing."""
    name, depth, need, fits, limit = refusal(keys, BC.deep_gate_circuit(plonk, 5, 64))
    assert (name, depth) == ("h(X)", 65) and need == 64 * 128 * 36 + 17 * 128 * 8 > limit >= 64 * 1024
    slots = (limit - 17 * 128 * 8) // (128 * 36)  # the launch asks for depth - 1 slots
    assert fits == slots + 1
    levels = slots  # the pass records depth = levels + 1
    print("LDS per workgroup %d bytes: h(X) programs of depth <= %d (%d stack slots), Lagrange-domain programs of depth <= %d"
          % (limit, fits, slots, limit // (128 * 32) - 1))
    assert (levels + 1) * 128 * 32 <= limit  # ... and the witness check's depth + 1 = levels + 1 slots fit as well
    assert prove_and_check(ctx, plonk, oracle, keys, BC.deep_gate_circuit(plonk, 5, levels)) == levels
    assert refusal(keys, BC.deep_gate_circuit(plonk, 5, levels + 1))[:2] == ("h(X)", levels + 2)
    # a lookup input: `levels - 2` products, the deepest the Lagrange-domain compression program can be given
    assert prove_and_check(ctx, plonk, oracle, keys, BC.deep_lookup_circuit(plonk, 5, levels - 2)) == levels
    assert refusal(keys, BC.deep_lookup_circuit(plonk, 5, levels - 1))[:2] == ("h(X)", levels + 2)
    # the ctx proves another circuit afterwards
    c, dev, opk = keys.get("branches")
    wit = Witness(ctx, oracle, c)
    assert plonk.create_proof(ctx, dev[(None, 0)], wit.inst, wit.upload(), seed=62) == PR.create_proof(opk, c.instances, c.advice, seed=62)
    wit.d_adv.free()


def test_a_key_from_sigma_meets_the_same_refusal_and_the_deepest_key_survives_its_file(ctx, plonk, oracle, keys):
    """amdzk_keygen_sigma and amdzk_pk_read build their programs in the same steps as amdzk_keygen: the file of the deepest
    key that fits reads back with the same program, and its sigma columns under a description one level deeper are refused."""
    _, _, _, fits, _ = refusal(keys, BC.deep_gate_circuit(plonk, 5, 64))
    c = BC.deep_gate_circuit(plonk, 5, fits - 1)
    pk = keys.keygen(c)
    sigma = pk.export(1)
    again = plonk.ProvingKey.read(ctx, keys.srs(c.k), pk.write())
    assert h_program(keys.pkg, again) == h_program(keys.pkg, pk)
    again.free()
    pk.free()
    deeper = BC.deep_gate_circuit(plonk, 5, fits)
    with pytest.raises(keys.pkg.ffi.AmdzkError) as e:
        plonk.ProvingKey.from_sigma(ctx, keys.srs(c.k), deeper.desc, fr_cols(oracle, deeper.fixed, deeper.n), sigma, zu.fr_from_int(REPR)).free()
    assert e.value.code == UNSUPPORTED and "the h(X) program has stack depth %d" % (fits + 1) in str(e.value)
