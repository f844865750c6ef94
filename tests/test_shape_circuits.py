"""CPU: the circuits of tests/shape_circuits.py — the extreme shapes of a constraint system — are what their names say, hold
a satisfying witness, and are proved by both oracle provers to the same bytes, which the oracle verifier accepts under
(blake2b, shplonk) and (evm, gwc) and rejects with one byte or one public input changed. The two refusal shapes are
refused where the issue of a prover is: the identity commitment of a zero h(X) piece, and a domain with no usable row.
tests/test_gpu_shape_circuits.py compares the device with these same bytes."""
import os
import sys

import pytest

import shape_circuits as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import witness_check_ref as W  # noqa: E402

TAU, REPR, SEED = S.TAU, S.REPR, S.SEED


@pytest.fixture(scope="module")
def plonk():
    import __graft_entry__ as g
    return g.load_package().plonk


# name -> k, A, F, I, permutation columns, lookups (pairs of each), gate polynomials, degree, usable rows, permutation sets
COUNTS = {
    "square_min_rows":    dict(k=3, A=2, F=1, I=1, S=3, L=[], G=1, degree=3, usable=2, sets=3),
    "perm_only-k3":       dict(k=3, A=2, F=0, I=0, S=2, L=[], G=0, degree=3, usable=2, sets=2),
    "perm_only-k4":       dict(k=4, A=2, F=0, I=0, S=2, L=[], G=0, degree=3, usable=10, sets=2),
    "perm_ten_sets":      dict(k=4, A=9, F=0, I=1, S=10, L=[], G=0, degree=3, usable=10, sets=10),
    "lookup_only-k3":     dict(k=3, A=1, F=1, I=0, S=0, L=[1], G=0, degree=4, usable=2, sets=0),
    "lookup_only-k4":     dict(k=4, A=1, F=1, I=0, S=0, L=[1], G=0, degree=4, usable=10, sets=0),
    "lookups_eight":      dict(k=4, A=8, F=8, I=0, S=0, L=[1] * 8, G=0, degree=4, usable=10, sets=0),
    "lookup_six_wide":    dict(k=4, A=6, F=6, I=0, S=0, L=[6], G=0, degree=4, usable=10, sets=0),
    "no_advice":          dict(k=4, A=0, F=2, I=1, S=0, L=[], G=1, degree=3, usable=10, sets=0),
    "far_rotation-11":    dict(k=5, A=2, F=2, I=0, S=2, L=[1], G=1, degree=4, usable=26, sets=1),
    "far_rotation-31":    dict(k=5, A=2, F=2, I=0, S=2, L=[1], G=1, degree=4, usable=26, sets=1),
    "far_rotation-33":    dict(k=5, A=2, F=2, I=0, S=2, L=[1], G=1, degree=4, usable=26, sets=1),
    "unused_columns":     dict(k=4, A=3, F=2, I=2, S=3, L=[], G=1, degree=3, usable=10, sets=3),
    "tables_interleaved": dict(k=4, A=5, F=2, I=0, S=0, L=[1, 1, 1], G=0, degree=5, usable=10, sets=0),
}
# every (column, rotation) the shape's constraints read, by column kind
ROTATIONS = {
    "square_min_rows":    dict(advice=[(0, 0), (1, 0)], fixed=[(0, 0)], instance=[(0, 0)]),
    "perm_only-k3":       dict(advice=[(0, 0), (1, 0)], fixed=[], instance=[]),
    "perm_only-k4":       dict(advice=[(0, 0), (1, 0)], fixed=[], instance=[]),
    "perm_ten_sets":      dict(advice=[(j, 0) for j in range(9)], fixed=[], instance=[(0, 0)]),
    "lookup_only-k3":     dict(advice=[(0, 0)], fixed=[(0, 0)], instance=[]),
    "lookup_only-k4":     dict(advice=[(0, 0)], fixed=[(0, 0)], instance=[]),
    "lookups_eight":      dict(advice=[(j, 0) for j in range(8)], fixed=[(j, 0) for j in range(8)], instance=[]),
    "lookup_six_wide":    dict(advice=[(j, 0) for j in range(6)], fixed=[(j, 0) for j in range(6)], instance=[]),
    "no_advice":          dict(advice=[], fixed=[(0, 0), (1, 0)], instance=[(0, 0), (0, 1)]),
    "far_rotation-11":    dict(advice=[(0, 0), (1, 0), (0, 11), (0, -11)], fixed=[(0, 0), (1, 0)], instance=[]),
    "far_rotation-31":    dict(advice=[(0, 0), (1, 0), (0, 31), (0, -31)], fixed=[(0, 0), (1, 0)], instance=[]),
    "far_rotation-33":    dict(advice=[(0, 0), (1, 0), (0, 33), (0, -33)], fixed=[(0, 0), (1, 0)], instance=[]),
    "unused_columns":     dict(advice=[(0, 0), (1, 0)], fixed=[(0, 0)], instance=[(0, 0)]),
    "tables_interleaved": dict(advice=[(0, 0), (1, 0), (2, 0), (3, 1), (4, -1)], fixed=[(0, 0), (1, 0)], instance=[]),
}


def test_the_tables_name_every_shape():
    assert set(COUNTS) == set(ROTATIONS) == set(S.SHAPES) and len(S.SHAPES) == 14
    assert set(S.REFUSALS) == {"nothing_constrained", "too_few_rows"}


@pytest.mark.parametrize("name", S.NAMES)
def test_the_shape_is_what_its_name_says(plonk, name):
    c, want = S.shape(plonk, name), COUNTS[name]
    d = c.desc
    chunk = d["cs_degree"] - 2
    got = dict(k=d["k"], A=d["num_advice"], F=d["num_fixed"], I=d["num_instance"], S=len(d["permutation_columns"]),
               L=[len(lk["inputs"]) for lk in d["lookups"]], G=len(d["gates"]), degree=d["cs_degree"], usable=c.usable,
               sets=(len(d["permutation_columns"]) + chunk - 1) // chunk)
    assert got == want
    assert all(len(lk["inputs"]) == len(lk["tables"]) for lk in d["lookups"])
    assert d["blinding_factors"] == 5 and c.n == 1 << want["k"] and c.usable == c.n - 6
    rot = ROTATIONS[name]
    assert (d["advice_queries"], d["fixed_queries"], d["instance_queries"]) == (rot["advice"], rot["fixed"], rot["instance"])
    assert len(c.advice) == want["A"] and len(c.fixed) == want["F"] and len(c.instances) == want["I"]
    kinds = S.SHAPES[name][1]
    assert ("gate" in kinds) == (want["G"] > 0) and ("lookup" in kinds) == bool(want["L"])
    assert ("copy" in kinds) == any(tuple(c.assembly.mapping[i][j]) != (i, j) for i in range(want["S"]) for j in range(c.n))


def test_the_shapes_hold_what_the_counts_cannot_show(plonk):
    n = 32
    for r in (11, 31, 33):
        c = S.shape(plonk, "far_rotation-%d" % r)
        on = [row for row in range(c.usable) if (row + r) % n < c.usable and (row - r) % n < c.usable]
        assert on and [row for row in range(n) if c.fixed[0][row]] == on == c.gate_rows
    assert 31 % n == (-1) % n and 33 % n == 1 % n  # the points of the built-in rotations -1 (lookups) and +1 (products)
    c = S.shape(plonk, "unused_columns")
    queried = {col for col, _ in c.desc["advice_queries"]}
    assert queried == {0, 1} and all(c.advice[2][row] for row in range(c.usable))
    assert {col for col, _ in c.desc["fixed_queries"]} == {0} and all(c.fixed[1][row] for row in range(c.usable))
    assert {col for col, _ in c.desc["instance_queries"]} == {0} and len(c.instances[1]) == c.usable and all(c.instances[1])
    c = S.shape(plonk, "tables_interleaved")
    tables = [lk["tables"][0][0] for lk in c.desc["lookups"]]
    assert tables == ["advice", "fixed", "advice"]
    assert c.desc["lookups"][2]["tables"][0] == ("advice", 4, -1) and S._queries(c.desc["lookups"][2]["inputs"][0], "advice", []) == [(3, 1)]
    c = S.shape(plonk, "perm_ten_sets")
    rows = {row for i in range(10) for row in range(c.n) if tuple(c.assembly.mapping[i][row]) != (i, row)}
    assert {0, c.usable - 1} <= rows and tuple(c.assembly.mapping[9][0]) != (9, 0) and len(c.instances[0]) == 1
    for k in (3, 4):
        c = S.shape(plonk, "perm_only-k%d" % k)
        assert {row for i in range(2) for row in range(c.n) if tuple(c.assembly.mapping[i][row]) != (i, row)} == {0, c.usable - 1}
    c = S.shape(plonk, "no_advice")
    assert c.advice == [] and len(c.instances[0]) == c.usable


@pytest.mark.parametrize("name", S.NAMES)
def test_the_witness_satisfies_and_one_corrupted_cell_per_kind_does_not(plonk, name):
    c = S.shape(plonk, name)
    assert S.check_satisfied(c)
    assert W.report(c) == []
    for seed in (1, 2) if c._witness_fn else ():
        adv, inst = c.witness(seed)
        assert W.report(c, advice=adv, instances=inst) == [] and adv != c.advice
    for way in sorted(S.SHAPES[name][1]):
        adv, inst, rep = S.corrupt(c, way)
        assert any(e[0] == S.KIND[way] for e in rep)
        with pytest.raises(AssertionError):
            S.check_satisfied(c, advice=adv, instances=inst)


@pytest.mark.parametrize("name", S.NAMES)
def test_the_oracle_provers_agree_and_the_verifier_accepts(plonk, name):
    import plonk_fast as PF

    c, opk = S.shape(plonk, name), S.oracle_key(plonk, name)
    fpk = PF.FastKey(c.desc, c.fixed, c.assembly.mapping, TAU, REPR)
    assert fpk.fixed_commitments == opk.fixed_commitments and fpk.permutation_commitments == opk.permutation_commitments
    assert len(opk.fixed_commitments) == COUNTS[name]["F"] and len(opk.permutation_commitments) == COUNTS[name]["S"]
    for tr in ("blake2b", "evm"):  # the C++-backed prover opens with SHPLONK alone
        assert PF.create_proof(fpk, c.instances, c.advice, seed=SEED, transcript=tr) == S.oracle_proof(plonk, name, tr, "shplonk")
    bad = S.wrong_instances(c)
    assert (bad is None) == (not any(c.instances))
    for tr, mo in S.KINDS:
        proof = S.oracle_proof(plonk, name, tr, mo)
        assert PR.verify_proof(opk, c.instances, proof, transcript=tr, multiopen=mo)
        with pytest.raises(AssertionError):
            PR.verify_proof(opk, c.instances, S.flipped(proof), transcript=tr, multiopen=mo)
        if bad is not None:
            with pytest.raises(AssertionError):
                PR.verify_proof(opk, bad, proof, transcript=tr, multiopen=mo)


@pytest.mark.parametrize("name", ["perm_ten_sets", "unused_columns"])
def test_the_oracle_proves_two_instances_under_gwc(plonk, name):
    c, opk = S.shape(plonk, name), S.oracle_key(plonk, name)
    wit = [(c.advice, c.instances), c.witness(1)]
    for tr in ("blake2b", "evm"):
        proof = PR.create_proof_multi(opk, [i for _, i in wit], [a for a, _ in wit], seed=SEED, transcript=tr, multiopen="gwc")
        assert PR.verify_proof_multi(opk, [i for _, i in wit], proof, transcript=tr, multiopen="gwc")
        with pytest.raises(AssertionError):
            PR.verify_proof_multi(opk, [i for _, i in wit][::-1], proof, transcript=tr, multiopen="gwc")


def test_nothing_constrained_is_refused_for_its_identity_commitment(plonk):
    import plonk_fast as PF

    c = S.shape(plonk, "nothing_constrained")
    assert S.check_satisfied(c) and W.report(c) == []
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    with pytest.raises(AssertionError, match="cannot write points at infinity"):
        PR.create_proof(opk, c.instances, c.advice, seed=SEED)
    with pytest.raises(AssertionError, match="cannot write points at infinity"):
        PF.create_proof(PF.FastKey(c.desc, c.fixed, c.assembly.mapping, TAU, REPR), c.instances, c.advice, seed=SEED)


def test_too_few_rows_is_refused_at_keygen(plonk):
    c = S.shape(plonk, "too_few_rows")
    assert c.n == 4 and c.usable < 0
    with pytest.raises(AssertionError, match="not enough rows"):
        PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)


@pytest.mark.parametrize("name", S.NAMES)
def test_key_files_with_empty_sections_pass_the_host_checks(plonk, name):
    """The proving-key and verifying-key files of the oracle's key, from the independent encoders: the library's host-only
    parsers accept them and report the shape's counts — with no fixed column, no permutation column or no advice column
    the files have zero-length sections — and the description they rebuild is the circuit's."""
    import pk_blob
    import vk_blob
    import zkutil as zu
    import pyref as P

    c, opk, want = S.shape(plonk, name), S.oracle_key(plonk, name), COUNTS[name]
    blob = pk_blob.encode(plonk, zu.Oracle(), c.desc, opk, REPR)
    shape = dict(k=want["k"], num_fixed=want["F"], num_advice=want["A"], num_perm_columns=want["S"], num_challenges=0)
    assert plonk.blob_info(blob) == shape == pk_blob.shape(c.desc)
    assert len(blob) == len(pk_blob.header(plonk, c.desc)) + 32 + (want["F"] + want["S"]) * (64 + 32 * c.n) + 64
    assert plonk.blob_desc(blob) == c.desc
    with pytest.raises(plonk._ffi.AmdzkError, match="pk_read: digest mismatch"):
        plonk.blob_info(S.flipped(blob))
    vfile = vk_blob.encode(plonk, c.desc, opk.fixed_commitments, opk.permutation_commitments, REPR, P.G1_GEN)
    assert plonk.vk_blob_info(vfile) == dict(shape, has_g2=False) == vk_blob.shape(c.desc, False)
    assert plonk.blob_desc(vfile) == plonk.blob_desc(blob)
