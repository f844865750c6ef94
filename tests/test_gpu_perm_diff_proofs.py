"""GPU: proofs whose permutation products are committed through their row differences (prover.hip, Prover::perm_commit) are
the oracle's bytes, at the two ends of how often a product column changes and on every route that reaches that phase:
the lanes and a serial key, two phases, create_proof_multi and the lock-step batch.

The circuits: tests/circuits.py random_circuit (the generator of tests/test_random_circuits.py) where a seed has the shape — no
permutation columns; permutation columns without a single copy, every Z constant up to its blinding tail — and `copy_circuit`
below for the shape no seed has: a copy on every usable row, so every Z changes on every row (the dense case)."""
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


def copy_circuit(plonk, k, every_row, seed=1):
    """b = a * a on every usable row; a, c and b are in the permutation. every_row: c[row] is a copy of a[row] on every usable
    row (each cell of a and c sits in a cycle); else there is no copy at all and c is free."""
    rnd = np.random.RandomState(seed)
    cs = plonk.ConstraintSystem()
    a, c_, b = cs.advice_column(), cs.advice_column(), cs.advice_column()
    sel = cs.selector()
    for col in (a, c_, b):
        cs.enable_equality(col)

    def gate(meta):
        x = meta.query_advice(a, 0)
        return [meta.query_selector(sel) * (meta.query_advice(b, 0) - x * x)]

    cs.create_gate(gate)
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    for row in range(c.usable):
        x = int(rnd.randint(1, 1 << 62)) * int(rnd.randint(1, 1 << 62))
        c.fixed[sel.index][row] = 1
        c.advice[a.index][row] = x
        c.advice[b.index][row] = x * x % circuits.R
        c.advice[c_.index][row] = x if every_row else int(rnd.randint(1, 1 << 30))
        if every_row:
            c.copy(a, row, c_, row)
    c.instances = []
    circuits.check_satisfied(c)
    return c


def generated(plonk, k, want):
    """the first seed whose random circuit has the wanted shape"""
    for seed in range(300):
        c = circuits.random_circuit(plonk, k, seed)
        if want(c):
            return c, seed
    raise AssertionError("the generator made no such circuit at k = %d" % k)


def prove_and_compare(ctx, pkg, plonk, oracle, c, seed, flags=None):
    if c.k not in _srs:
        _srs[c.k] = zu.test_srs(oracle, c.k, TAU)
    g, gl = _srs[c.k]
    params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=flags)
    adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    want = PR.create_proof(opk, c.instances, c.advice, seed=seed)
    try:
        assert plonk.create_proof(ctx, pk, inst, d_adv, seed=seed) == want
        assert plonk.create_proof(ctx, pk, inst, d_adv, seed=seed) == want  # the difference scratch is reused cleanly
        assert PR.verify_proof(opk, c.instances, want)
    finally:
        d_adv.free(); pk.free(); params.free()


@pytest.mark.parametrize("k", [5, 6, 7])
@pytest.mark.parametrize("serial", [False, True])
def test_copy_on_every_usable_row(ctx, pkg, plonk, oracle, k, serial):
    c = copy_circuit(plonk, k, every_row=True, seed=k)
    assert len(c.copies) == c.usable
    prove_and_compare(ctx, pkg, plonk, oracle, c, seed=40 + k, flags=plonk.KEYGEN_SERIAL if serial else None)


@pytest.mark.parametrize("k", [5, 6, 7])
def test_permutation_columns_without_any_copy(ctx, pkg, plonk, oracle, k):
    """Every Z is 1 on all usable rows: its differences are zero but for the blinding tail."""
    c, seed = generated(plonk, k, lambda c: len(c.cs.permutation_columns) >= 2 and not c.copies)
    prove_and_compare(ctx, pkg, plonk, oracle, c, seed=seed, flags=plonk.KEYGEN_SERIAL if k == 6 else None)
    prove_and_compare(ctx, pkg, plonk, oracle, copy_circuit(plonk, k, every_row=False, seed=k), seed=50 + k)


@pytest.mark.parametrize("k", [5, 6, 7])
def test_no_permutation_columns(ctx, pkg, plonk, oracle, k):
    """No Z at all: no prefix-sum basis is built (the MSM over it is still refused afterwards) and nothing else changes."""
    c, seed = generated(plonk, k, lambda c: not c.cs.permutation_columns)
    prove_and_compare(ctx, pkg, plonk, oracle, c, seed=seed)


@pytest.mark.parametrize("k", [5, 7])
def test_two_phase_circuit(ctx, pkg, plonk, oracle, monkeypatch, k):
    c = PC.rlc_circuit(plonk, k, seed=k)
    assert c.cs.permutation_columns
    dev = TP.Device(ctx, pkg, plonk, oracle, c)
    try:
        got = dev.prove(seed=31)
        assert got == TP.expected(monkeypatch, dev, dev.opk(), 31, dev.challenges())
    finally:
        dev.free()


@pytest.mark.parametrize("k", [5, 6])
def test_two_proofs_through_the_batch_and_multi(ctx, pkg, plonk, oracle, k):
    """Two workspaces of the dense circuit: amdzk_create_proof_batch (the gang's commitment step now has two submissions,
    the lookup products' and the differences') gives each proof the oracle's bytes, and create_proof_multi over the same two
    instances the oracle's multi-instance proof."""
    c = copy_circuit(plonk, k, every_row=True, seed=10 + k)
    wit = [(c.advice, c.instances), (c.advice, c.instances)]
    B = TB.Batch(ctx, pkg, plonk, oracle, c, wit)
    try:
        got = B.batch([7, 8])
        opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=TB.REPR)
        for b, s in enumerate((7, 8)):
            assert got[b] == PR.create_proof(opk, c.instances, c.advice, seed=s), "proof %d" % b
        multi = plonk.create_proof_multi(ctx, B.pks, B.inst, B.d_adv, seed=9)
        assert multi == PR.create_proof_multi(opk, [c.instances] * 2, [c.advice] * 2, seed=9)
    finally:
        B.free()
