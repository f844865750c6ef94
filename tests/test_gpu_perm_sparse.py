"""GPU: the permutation products formed from the cells that have copies (plonk_kernels.hip perm_frac_sparse / perm_fill, the
lists of keygen.hip build_perm_lists) — the oracle's proof bytes on both sides of the density rule m <= nsets * u / 2 and on
every route that reaches Prover::perm_products, and the product columns themselves, word for word, against the dense route.

`copies_circuit` below: b = a * a on every usable row, the free advice column c, and (with `wide`) an instance and a fixed
column, all in the permutation. Its constraint degree is 3, so every permutation column is a set of its own: three sets,
five with `wide`, chained through last_z. A copy src -> dst gives the destination cell the source's value and takes two
cells off the identity permutation; the expected list is counted from Assembly.mapping on the host (expected_cells)."""
import os
import sys

import numpy as np
import pytest

import circuits
import phased_circuits as PC
import test_gpu_batch as TB
import test_gpu_phased as TP
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
REPR = 99
_srs = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def copies_circuit(plonk, k, copies, wide=False, seed=1):
    """copies: (source column name, row, destination column name, row); sources 'a', 'b', 'c', destinations 'c' and, with
    `wide`, 'i' (instance) and 'f' (fixed) — the cells no gate constrains. Every destination cell is written once."""
    rnd = np.random.RandomState(seed)
    cs = plonk.ConstraintSystem()
    col = {"a": cs.advice_column(), "c": cs.advice_column(), "b": cs.advice_column()}
    if wide:
        col["i"], col["f"] = cs.instance_column(), cs.fixed_column()
    sel = cs.selector()
    for x in col.values():
        cs.enable_equality(x)

    def gate(meta):
        x = meta.query_advice(col["a"], 0)
        return [meta.query_selector(sel) * (meta.query_advice(col["b"], 0) - x * x)]

    cs.create_gate(gate)
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    for row in range(c.usable):
        x = int(rnd.randint(1, 1 << 62)) * int(rnd.randint(1, 1 << 62))
        c.fixed[sel.index][row] = 1
        c.advice[col["a"].index][row] = x
        c.advice[col["b"].index][row] = x * x % circuits.R
        c.advice[col["c"].index][row] = int(rnd.randint(1, 1 << 30))
    if wide:
        c.instances[col["i"].index] = [int(v) for v in rnd.randint(1, 1 << 30, size=c.usable)]
        c.fixed[col["f"].index][:c.usable] = [int(v) for v in rnd.randint(1, 1 << 30, size=c.usable)]
    seen = set()
    for s, r1, d, r2 in copies:
        assert d in ("c", "i", "f") and (d, r2) not in seen and s in ("a", "b", "c") and (s != "c" or ("c", r1) not in seen)
        seen.add((d, r2))
        v = c.value(col[s], r1)
        if d == "c":
            c.advice[col["c"].index][r2] = v
        elif d == "i":
            c.instances[col["i"].index][r2] = v
        else:
            c.fixed[col["f"].index][r2] = v
        c.copy(col[s], r1, col[d], r2)
    if not wide:
        c.instances = []
    circuits.check_satisfied(c)
    return c


def expected_cells(c):
    """(m, sparse) from the mapping: the (set, usable row) pairs where a column of the set is not mapped to itself"""
    S = len(c.cs.permutation_columns)
    chunk = c.desc["cs_degree"] - 2
    nsets = (S + chunk - 1) // chunk
    mp = np.array(c.assembly.mapping, dtype=np.int64).reshape(S, c.n, 2)
    off = (mp[:, :, 0] != np.arange(S)[:, None]) | (mp[:, :, 1] != np.arange(c.n)[None, :])
    m = sum(int(off[s * chunk:(s + 1) * chunk, :c.usable].any(axis=0).sum()) for s in range(nsets))
    return m, 2 * m <= nsets * c.usable


class Dev:
    def __init__(self, ctx, pkg, plonk, oracle, c, flags=None):
        if c.k not in _srs:
            _srs[c.k] = zu.test_srs(oracle, c.k, TAU)
        g, gl = _srs[c.k]
        self.ctx, self.plonk, self.c = ctx, plonk, c
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        self.fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, self.fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=flags)
        adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
        self.d_adv = ctx.alloc(adv.nbytes).upload(adv)
        self.inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
        self.opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        self.keys = [self.pk]

    def prove(self, seed, pk=None, transcript=0):
        return self.plonk.create_proof(self.ctx, pk or self.pk, self.inst, self.d_adv, seed=seed, transcript=transcript)

    def want(self, seed, **kw):
        return PR.create_proof(self.opk, self.c.instances, self.c.advice, seed=seed, **kw)

    def free(self):
        self.d_adv.free()
        for pk in reversed(self.keys):
            pk.free()
        self.params.free()


def prove_and_compare(ctx, pkg, plonk, oracle, c, seed, sparse, flags=None):
    """The key lists what the mapping says and takes the expected branch; two proofs in a row are the oracle's bytes."""
    m, sp = expected_cells(c)
    assert sp == sparse, "the circuit is on the other side of the density rule: m = %d" % m
    d = Dev(ctx, pkg, plonk, oracle, c, flags)
    try:
        assert d.pk.perm_cells() == (m, sparse)
        want = d.want(seed)
        assert d.prove(seed) == want
        assert d.prove(seed) == want  # the compact arrays share the fraction columns with the row differences
        assert PR.verify_proof(d.opk, c.instances, want)
    finally:
        d.free()


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("serial", [False, True])
def test_no_copy_at_all(ctx, pkg, plonk, oracle, k, serial):
    """m = 0: every Z is 1 up to its blinding tail."""
    c = copies_circuit(plonk, k, [], seed=k)
    assert expected_cells(c) == (0, True)
    prove_and_compare(ctx, pkg, plonk, oracle, c, 60 + k, True, plonk.KEYGEN_SERIAL if serial else None)


@pytest.mark.parametrize("k", [5, 6])
def test_copy_on_every_usable_row_stays_dense(ctx, pkg, plonk, oracle, k):
    c = copies_circuit(plonk, k, [("a", r, "c", r) for r in range((1 << k) - 6)], seed=k)
    assert expected_cells(c) == (2 * c.usable, False)
    prove_and_compare(ctx, pkg, plonk, oracle, c, 61 + k, False)


@pytest.mark.parametrize("k", [5, 7])
@pytest.mark.parametrize("over", [False, True])
def test_either_side_of_the_density_rule(ctx, pkg, plonk, oracle, k, over):
    """Three sets of u rows, two listed cells per copy: j copies are sparse up to 2 j <= 3 u / 2."""
    u = (1 << k) - 6
    j = (3 * u) // 4 + (1 if over else 0)
    c = copies_circuit(plonk, k, [("a", r, "c", u - 1 - r) for r in range(j)], seed=k)
    assert c.usable == u and expected_cells(c) == (2 * j, not over)
    prove_and_compare(ctx, pkg, plonk, oracle, c, 62 + k, not over, plonk.KEYGEN_SERIAL if k == 7 else None)


@pytest.mark.parametrize("k", [5, 6])
def test_copies_at_the_first_and_the_last_usable_row(ctx, pkg, plonk, oracle, k):
    u = (1 << k) - 6
    c = copies_circuit(plonk, k, [("a", 0, "c", u - 1), ("b", u - 1, "c", 0)], seed=k)
    assert expected_cells(c) == (4, True)
    prove_and_compare(ctx, pkg, plonk, oracle, c, 63 + k, True)


def wide_circuit(plonk, k, seed=3):
    """Five sets, copies in every one of them, instance and fixed cells among them, the first and last usable rows too."""
    u = (1 << k) - 6
    cp = [("a", 1, "i", 0), ("b", 2, "f", u - 1), ("c", 4, "i", u - 1), ("a", u - 1, "f", 0), ("b", 0, "c", 9), ("a", 3, "c", 3), ("b", 7, "i", 5),
          ("a", 1, "f", 6)]
    c = copies_circuit(plonk, k, cp, wide=True, seed=seed)
    assert len(c.cs.permutation_columns) == 5 and c.desc["cs_degree"] == 3
    return c


@pytest.mark.parametrize("k", [5, 7])
def test_five_chained_sets_with_instance_and_fixed_cells(ctx, pkg, plonk, oracle, k):
    c = wide_circuit(plonk, k)
    assert expected_cells(c)[1]
    prove_and_compare(ctx, pkg, plonk, oracle, c, 64 + k, True)


def test_both_transcripts_and_both_multiopens(ctx, pkg, plonk, oracle):
    d = Dev(ctx, pkg, plonk, oracle, wide_circuit(plonk, 5))
    try:
        assert d.pk.perm_cells()[1]
        for kind, name in ((plonk.TRANSCRIPT_BLAKE2B, "blake2b"), (plonk.TRANSCRIPT_KECCAK256_EVM, "evm")):
            for bit, mo in ((0, "shplonk"), (plonk.MULTIOPEN_GWC, "gwc")):
                assert d.prove(17, transcript=kind | bit) == d.want(17, transcript=name, multiopen=mo), (name, mo)
    finally:
        d.free()


def test_keys_that_were_read_or_built_from_sigma_and_a_clone(ctx, pkg, plonk, oracle):
    """amdzk_pk_read and amdzk_keygen_sigma derive the same lists (the file does not hold them); a clone shares them."""
    c = wide_circuit(plonk, 6)
    d = Dev(ctx, pkg, plonk, oracle, c)
    try:
        cells = d.pk.perm_cells()
        assert cells == expected_cells(c) and cells[1]
        want = d.want(23)
        blob = d.pk.write()
        d.keys.append(plonk.ProvingKey.read(ctx, d.params, blob, flags=0))
        d.keys.append(plonk.ProvingKey.from_sigma(ctx, d.params, c.desc, d.fixed, d.pk.export(1), zu.fr_from_int(REPR), flags=0))
        d.keys.append(d.keys[1].clone_workspace())
        d.keys.append(d.pk.clone_workspace())
        for i, pk in enumerate(d.keys[1:]):
            assert pk.perm_cells() == cells, i
            assert d.prove(23, pk=pk) == want, i
        assert d.keys[1].write() == blob
    finally:
        d.free()


@pytest.mark.parametrize("k,wide", [(6, True), (5, False)])
def test_two_proofs_through_the_batch_and_multi(ctx, pkg, plonk, oracle, k, wide):
    """amdzk_create_proof_batch (k = 6) and create_proof_multi with N = 2, each workspace with its own pointer table."""
    u = (1 << k) - 6
    c = wide_circuit(plonk, k) if wide else copies_circuit(plonk, k, [("a", r, "c", r + 1) for r in range(0, u - 1, 3)], seed=9)
    wit = [(c.advice, c.instances), (c.advice, c.instances)]
    B = TB.Batch(ctx, pkg, plonk, oracle, c, wit)
    try:
        assert B.pks[1].perm_cells() == expected_cells(c) and expected_cells(c)[1]
        opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=TB.REPR)
        got = B.batch([7, 8])
        for b, s in enumerate((7, 8)):
            assert got[b] == PR.create_proof(opk, c.instances, c.advice, seed=s), "proof %d" % b
        multi = plonk.create_proof_multi(ctx, B.pks, B.inst, B.d_adv, seed=9)
        assert multi == PR.create_proof_multi(opk, [c.instances] * 2, [c.advice] * 2, seed=9)
    finally:
        B.free()


@pytest.mark.parametrize("k", [5, 6])
def test_two_phase_key(ctx, pkg, plonk, oracle, monkeypatch, k):
    c = PC.rlc_circuit(plonk, k, seed=k)
    m, sparse = expected_cells(c)
    assert sparse, "the phased fixture left the sparse side of the rule: m = %d" % m
    dev = TP.Device(ctx, pkg, plonk, oracle, c)
    try:
        assert dev.pk.perm_cells() == (m, True)
        got = dev.prove(seed=31)
        assert got == TP.expected(monkeypatch, dev, dev.opk(), 31, dev.challenges())
    finally:
        dev.free()


@pytest.mark.parametrize("k,wide,copies", [(5, False, 13), (7, True, 8), (8, False, 125), (11, False, 1500)])
def test_product_columns_word_for_word_against_the_dense_route(ctx, pkg, plonk, oracle, k, wide, copies):
    """Rows 0 ... u of every Z before blinding, from the workspace a proof left: the listed cells alone give the words the
    fraction program, the full inversion and the per-column scans give — and those are the protocol's running products.
    k = 11: 3,000 listed cells, so the inversion takes two workgroups and the running product over the list two blocks."""
    u = (1 << k) - 6
    c = wide_circuit(plonk, k) if wide else copies_circuit(plonk, k, [("a", r, "c", (7 * r + 2) % u) for r in range(copies)], seed=k)
    m, sparse = expected_cells(c)
    assert sparse and m == (15 if wide else 2 * copies)
    d = Dev(ctx, pkg, plonk, oracle, c)
    try:
        assert d.prove(5) == d.want(5)
        beta, gamma = d.pk.inspect(1)[1], d.pk.inspect(1)[2]
        dense = d.pk.perm_products(beta, gamma, route=0)
        assert np.array_equal(d.pk.perm_products(beta, gamma, route=1), dense)
        assert np.array_equal(d.pk.perm_products(beta, gamma), dense)
        # the protocol's own values: Z[s][0] = last_z of the set before, Z[i + 1] = Z[i] * num_i / den_i
        b, g = zu.fr_to_int(beta), zu.fr_to_int(gamma)
        R, S = circuits.R, len(c.cs.permutation_columns)
        omega = zu.fr_to_int(oracle.omega(k))
        delta = PR.DELTA
        z, cols = 1, c.cs.permutation_columns
        for s in range(S):  # cs_degree 3: one column per set
            for i in range(u + 1):
                assert zu.fr_to_int(dense[s][i]) == z, (s, i)
                if i == u:
                    break
                v = c.value(cols[s], i)
                ms, mr = c.assembly.mapping[s][i]
                num = (v + b * pow(delta, s, R) * pow(omega, i, R) + g) % R
                den = (v + b * pow(delta, int(ms), R) * pow(omega, int(mr), R) + g) % R
                z = z * num * pow(den, R - 2, R) % R
        assert d.prove(6) == d.want(6)  # the entry point leaves the workspace fit for the next proof
    finally:
        d.free()


def test_dense_key_refuses_the_sparse_route(ctx, pkg, plonk, oracle):
    c = copies_circuit(plonk, 5, [("a", r, "c", r) for r in range(26)], seed=2)
    d = Dev(ctx, pkg, plonk, oracle, c)
    try:
        assert d.pk.perm_cells() == (52, False)
        assert d.prove(4) == d.want(4)
        ch = d.pk.inspect(1)
        with pytest.raises(pkg.AmdzkError, match="keeps no list"):
            d.pk.perm_products(ch[1], ch[2], route=1)
        assert np.array_equal(d.pk.perm_products(ch[1], ch[2]), d.pk.perm_products(ch[1], ch[2], route=0))
        assert d.prove(4) == d.want(4)
    finally:
        d.free()
