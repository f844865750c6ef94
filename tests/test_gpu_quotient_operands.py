"""GPU: amdzk_quotient_eval_dev — the coset transforms, the limb-resident h(X) interpreter (expr_eval_limbs_kernel) and
the recombination — on polynomials that are NOT a proof's: arbitrary ones, and constants chosen so that every word the
interpreter loads is an extreme of its 9 x 29-bit representation. The interpreter is lazily reduced; the host inserts the
weak reductions from bounds it tracks (finalize_limb_program) and adds up to six terms into un-carried 64-bit columns. A
proof's operands are evaluations on a coset, i.e. uniform field elements, for which a bound that is one bit too tight or
a column that overflows at the sixth term goes wrong with negligible probability. Everything is exact: the pieces must
equal, bit for bit, the oracle's for the key's mode (oracle/plonk_ref.py quotient_pieces for KEYGEN_FULL_COSETS,
quotient_pieces_on_cosets for the default; tests/test_oracle_quotient.py shows they differ on such inputs).

Which coefficient makes the interpreter load a chosen word W. A committed polynomial reaches the interpreter through
zk_coeff_to_cosets_r261 (poly.hip): per coset c one size-n transform whose first step multiplies input element m by the
table entry in_tab[c][m] (ntt.hip, F_IN_TABLE: xv = f29_mul(unpack(a_m), unpack(in_tab[m]))). zk_quotient_plan fills the
table with coset_table_kernel(g = g_c, scale = 32): entry m is fr29_const_to_r261(32 * g_c^m), the integer
(32 g_c^m) * 2^261 mod r. f29_mul is Montgomery multiplication in radix 2^261, so the product of the stored word a_m
(whatever field element it stands for) and that constant is the word a_m * 32 * g_c^m mod r. For a polynomial whose only
non-zero coefficient is the constant one, the transform's input is (32 a_0, 0, ..., 0) and every output row is 32 a_0
mod r, packed canonically by the last step (pack_out). The interpreter therefore loads W at every row and every rotation,
on every coset, exactly when coefficient 0 of the Montgomery-form input is the word W / 32 mod r. (As a field element
the polynomial is the constant W / 32 * 2^-256, which is what the oracle is given.)"""
import os
import random
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import plonk_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
R = zu.R
INV32 = pow(32, -1, R)
MONT_INV = pow(zu.MONT, -1, R)
LIMB = (1 << 29) - 1
T = R >> 232
# The words the interpreter is to load (all below r). The last two have limbs alternating between 0x1FFFFFFF and 0: ones in
# the odd limbs (limb 8 is then 0), and ones in the even limbs with limb 8, which r caps at T, brought down to T - 1.
WORDS = {
    "r_minus_1": R - 1,
    "T_2p232_minus_1": (T << 232) - 1,  # T * 2^232 - 1: the low eight limbs all ones
    "zero": 0,
    "one": 1,
    "half_r_minus_1": (R - 1) // 2,
    "half_r_plus_1": (R + 1) // 2,
    "two_p253": 1 << 253,
    "alt_odd_limbs": sum(LIMB << (29 * i) for i in (1, 3, 5, 7)),
    "alt_even_limbs": sum(LIMB << (29 * i) for i in (0, 2, 4, 6)) + ((T - 1) << 232),
}
assert all(0 <= w < R for w in WORDS.values())
CIRCUITS = ("lookup5", "rsa7", "hd9")
POLYSETS = ["arbitrary%d" % s for s in range(3)] + ["word_" + w for w in WORDS] + ["dealt%d" % s for s in range(3)]
# theta = beta = gamma from {random, r - 1, 1} crossed with y from {random, 0, 1, r - 1} (for y = 1 and y = r - 1 the per-term
# power constants of OP_WACC are +-1), and one case that draws theta, beta and gamma from the three independently
CHALLENGES = ["tbg_%s.y_%s" % (t, y) for t in ("random", "rm1", "one") for y in ("random", "zero", "one", "rm1")] + ["tbg_mixed.y_random"]


def make_circuit(plonk, name):
    if name == "lookup5":
        return circuits.lookup_circuit(plonk, 5)
    if name == "rsa7":
        return circuits.rsa_sha256_shape(plonk, k=7, num_advice=5, num_lookup_advice=2, lookup_bits=5, num_spread=2, spread_bits=3)
    return circuits.high_degree_circuit(plonk, 5, power=9)  # the generic combine kernel, the SQR and MUL chains


def poly_counts(desc):
    """Number of polynomials per kind, in the header's order: advice | instance | A' | S' | permutation products | lookup products."""
    L = len(desc["lookups"])
    nsets = -(-len(desc["permutation_columns"]) // (desc["cs_degree"] - 2))
    return [("advice", desc["num_advice"]), ("instance", desc["num_instance"]), ("la", L), ("ls", L), ("z", nsets), ("lz", L)]


def constant_poly_words(words, n):
    """(len(words), n, 4) Montgomery-form input: polynomial i is the constant that makes the interpreter load words[i]."""
    a = np.zeros((len(words), n, 4), np.uint64)
    for i, w in enumerate(words):
        a[i, 0] = zu.limbs(w * INV32 % R)
    return a


def deal_words(count, seed):
    rnd = random.Random(seed)
    pool = list(WORDS.values())
    return [rnd.choice(pool) for _ in range(count)]


def make_polys(desc, n, polyset):
    NP = sum(cnt for _, cnt in poly_counts(desc))
    kind, _, arg = polyset.partition("_")
    if kind.startswith("arbitrary"):
        return zu.random_fr(NP * n, seed=7000 + int(kind[-1])).reshape(NP, n, 4)
    if kind == "word":
        return constant_poly_words([WORDS[arg]] * NP, n)
    return constant_poly_words(deal_words(NP, 8000 + int(kind[-1])), n)


def make_challenges(name, seed):
    """theta, beta, gamma, y as field elements for a case name "tbg_<random|rm1|one|mixed>.y_<random|zero|one|rm1>"."""
    rnd = random.Random(9000 + seed)
    t, y = (part.split("_")[1] for part in name.split("."))
    fixed = {"rm1": R - 1, "one": 1, "zero": 0}
    draw = lambda: rnd.randrange(2, R - 1)
    if t == "mixed":
        tbg = [rnd.choice([R - 1, 1, draw()]) for _ in range(3)]
    else:
        tbg = [fixed[t] if t in fixed else draw() for _ in range(3)]
    return tbg[0], tbg[1], tbg[2], fixed[y] if y in fixed else draw()


def by_kind(desc, polys_int):
    out, at = {}, 0
    for kind, cnt in poly_counts(desc):
        out[kind] = polys_int[at:at + cnt]
        at += cnt
    assert at == len(polys_int)
    return out


def to_field_ints(a):
    """Montgomery words (any shape (..., 4)) -> field elements as Python ints; sparse rows are cheap."""
    flat = np.ascontiguousarray(a).reshape(-1, 4)
    out = [0] * flat.shape[0]
    for i in np.flatnonzero(flat.any(axis=1)):
        out[i] = zu.from_limbs(flat[i]) * MONT_INV % R
    return out


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


class Keys:
    """Per circuit: the oracle's key and the device's keys in both coset modes, made once for the module."""

    def __init__(self, ctx, pkg, plonk, oracle):
        self.ctx, self.pkg, self.plonk, self.oracle = ctx, pkg, plonk, oracle
        self.made, self.oracle_polys = {}, {}

    def get(self, name):
        if name not in self.made:
            c = make_circuit(self.plonk, name)
            g, gl = zu.test_srs(self.oracle, c.k, TAU)
            params = self.pkg.kzg.ParamsKZG(self.ctx, c.k, g=g, g_lagrange=gl)
            fixed = np.stack([zu.ints_to_fr(self.oracle, col) for col in c.fixed])
            dev = {flags: self.plonk.ProvingKey(self.ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(99), flags=flags)
                   for flags in (0, self.plonk.KEYGEN_FULL_COSETS)}
            opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=99)
            self.made[name] = (c, params, dev, opk)
        return self.made[name]

    def polys(self, name, polyset):
        """(device input, the oracle's view of it by kind), shared by the challenge cases of one polynomial set."""
        if (name, polyset) not in self.oracle_polys:
            c = self.get(name)[0]
            a = make_polys(c.desc, c.n, polyset)
            ints = to_field_ints(a)
            self.oracle_polys[(name, polyset)] = (a, by_kind(c.desc, [ints[i * c.n:(i + 1) * c.n] for i in range(a.shape[0])]))
        return self.oracle_polys[(name, polyset)]

    def free(self):
        for _, params, dev, _ in self.made.values():
            for pk in dev.values():
                pk.free()
            params.free()


@pytest.fixture(scope="module")
def keys(ctx, pkg, plonk, oracle):
    k = Keys(ctx, pkg, plonk, oracle)
    yield k
    k.free()


def test_the_constant_input_is_the_loaded_word_over_32():
    """The derivation of the module docstring in numbers: the word W / 32, times the table's 32 * g^0, is W again."""
    for w in WORDS.values():
        assert (w * INV32 % R) * 32 % R == w
    limbs29 = lambda v: [(v >> (29 * i)) & LIMB for i in range(9)]
    assert limbs29(WORDS["T_2p232_minus_1"])[:8] == [LIMB] * 8 and limbs29(WORDS["T_2p232_minus_1"])[8] == T - 1
    assert limbs29(WORDS["alt_odd_limbs"]) == [0, LIMB] * 4 + [0]
    assert limbs29(WORDS["alt_even_limbs"]) == [LIMB, 0] * 4 + [T - 1]


@pytest.mark.parametrize("chal", CHALLENGES)
@pytest.mark.parametrize("polyset", POLYSETS)
@pytest.mark.parametrize("name", CIRCUITS)
def test_quotient_pieces_equal_the_oracle_in_both_coset_modes(keys, plonk, name, polyset, chal):
    c, _, dev, opk = keys.get(name)
    a, polys = keys.polys(name, polyset)
    theta, beta, gamma, y = make_challenges(chal, POLYSETS.index(polyset))
    num = PR.quotient_numerator(opk, polys, theta, beta, gamma, y)
    want = {0: PR.quotient_pieces_on_cosets(opk, polys, theta, beta, gamma, y, numerator=num),
            plonk.KEYGEN_FULL_COSETS: PR.quotient_pieces(opk, polys, theta, beta, gamma, y, numerator=num)}
    ch = [zu.fr_from_int(v) for v in (theta, beta, gamma, y)]
    for flags, pk in dev.items():
        got = pk.quotient_eval(a, *ch)
        assert got.shape == (c.desc["cs_degree"] - 1, c.n, 4)
        got = [to_field_ints(p) for p in got]
        assert got == want[flags], "%s %s %s: pieces differ from the oracle's, mode flags = %d" % (name, polyset, chal, flags)


# ------------------------------------------------------------------------------------------- the benchmark's own program
class Metric:
    """The metric's constraint system (141 advice, 24 lookups, 118 permutation columns) at k = 10: the h(X) program with
    hot-column groups, six pieces and the every-sixth-term carry. A Python oracle of the whole quotient is too slow at
    this size; the defining property of the default mode is checked instead — on its cosets g_c * H the interpolant is
    not truncated, so h(x) (x^n - 1) equals the y-folded constraints exactly at every point x = g_c * omega^i."""
    ROWS_PER_COSET = 16

    def __init__(self, oracle, c, quotient_eval):
        """quotient_eval(polys (NP, n, 4), theta, beta, gamma, y as Montgomery words) -> pieces (cs_degree - 1, n, 4)."""
        self.oracle, self.c, self.quotient_eval = oracle, c, quotient_eval
        desc = c.desc
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        n = c.n
        self.d = d = PR.Domain(desc["cs_degree"], c.k)
        od = zu.OracleDomain(oracle, desc["cs_degree"], c.k)
        self.fixed_polys = [od.lagrange_to_coeff(col) for col in fixed]
        omega_pow = [1] * n
        for i in range(1, n):
            omega_pow[i] = omega_pow[i - 1] * d.omega % R
        delta_pow = [pow(PR.DELTA, i, R) for i in range(len(desc["permutation_columns"]))]
        self.sigma_polys = [od.lagrange_to_coeff(zu.ints_to_fr(oracle, [delta_pow[pi] * omega_pow[pj] % R for pi, pj in col]))
                            for col in c.assembly.mapping]
        # the sample: rows 0 and n - 1 and 14 more of every one of the cs_degree - 1 cosets
        self.nc = desc["cs_degree"] - 1
        rnd = random.Random(4242)
        self.points = []
        for cc in range(self.nc):
            rows = [0, n - 1] + rnd.sample(range(1, n - 1), self.ROWS_PER_COSET - 2)
            g = d.coset_point(cc)
            self.points += [(cc, i, g * omega_pow[i] % R) for i in rows]
        self.key_evals = {}
        bf = desc["blinding_factors"]
        self.basis = {}
        for _, _, x in self.points:
            lb = PR.lagrange_basis_at(d, n, [0, n - bf - 1] + list(range(n - bf, n)), x)
            l_last = lb[n - bf - 1]
            self.basis[x] = {"l0": lb[0], "l_last": l_last, "l_active": (1 - (l_last + sum(lb[i] for i in range(n - bf, n)))) % R}

    def eval_key_poly(self, kind, i, x):
        if (kind, i, x) not in self.key_evals:
            poly = (self.fixed_polys if kind == "fixed" else self.sigma_polys)[i]
            self.key_evals[(kind, i, x)] = zu.fr_to_int(self.oracle.eval_polynomial(poly, zu.fr_from_int(x)))
        return self.key_evals[(kind, i, x)]

    def check(self, words, theta, beta, gamma, y):
        """words: per committed polynomial, the word the interpreter is to load (the polynomial is that constant)."""
        desc, d, n = self.c.desc, self.d, self.c.n
        a = constant_poly_words(words, n)
        pieces = self.quotient_eval(a, *[zu.fr_from_int(v) for v in (theta, beta, gamma, y)])
        assert pieces.shape == (self.nc, n, 4)
        consts = by_kind(desc, [w * INV32 % R * MONT_INV % R for w in words])  # the constants as field elements
        nsets = len(consts["z"])
        checked = 0
        for cc, row, x in self.points:
            def get(kind, i, rot, x=x):
                if kind in ("fixed", "sigma"):
                    return self.eval_key_poly(kind, i, d.rotate_omega(x, rot))
                if kind in self.basis[x]:
                    return self.basis[x][kind]
                return consts[kind][i]  # a constant polynomial: the same value at every rotation
            acc = 0
            for v in PR.h_constraints(desc, d, get, beta, gamma, theta, x, nsets, len(desc["lookups"])):
                acc = (acc * y + v) % R
            xn = pow(x, n, R)
            xm = zu.fr_from_int(x)
            hx = 0
            for piece in reversed(pieces):
                hx = (hx * xn + zu.fr_to_int(self.oracle.eval_polynomial(piece, xm))) % R
            assert acc == hx * (xn - 1) % R, "h(x)(x^n - 1) != folded constraints on coset %d, row %d" % (cc, row)
            checked += 1
        assert checked == self.nc * self.ROWS_PER_COSET  # no point is skipped



@pytest.fixture(scope="module")
def metric(ctx, pkg, plonk, oracle):
    shape = dict(circuits.SHAPES["full"])
    shape.pop("composite")
    shape["k"] = 10
    c = circuits.full_aadhaar_shape(plonk, **shape)
    assert c.desc["num_advice"] == 141 and len(c.desc["lookups"]) == 24 and len(c.desc["permutation_columns"]) == 118
    params = pkg.kzg.ParamsKZG.setup(ctx, c.k, zu.fr_from_int(TAU))
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(99), flags=0)  # the default mode
    yield Metric(oracle, c, pk.quotient_eval)
    pk.free()
    params.free()


METRIC_CASES = [("word_" + w, "tbg_random.y_random") for w in WORDS] + \
    [("dealt%d" % s, ch) for s in range(3) for ch in ("tbg_random.y_random", "tbg_random.y_one", "tbg_random.y_rm1", "tbg_rm1.y_random")]


@pytest.mark.parametrize("polyset,chal", METRIC_CASES)
def test_metric_shape_quotient_satisfies_its_definition_on_every_coset(metric, polyset, chal):
    NP = sum(cnt for _, cnt in poly_counts(metric.c.desc))
    kind, _, arg = polyset.partition("_")
    words = [WORDS[arg]] * NP if kind == "word" else deal_words(NP, 8100 + int(kind[-1]))
    metric.check(words, *make_challenges(chal, METRIC_CASES.index((polyset, chal))))
