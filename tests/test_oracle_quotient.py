"""CPU: the oracle's two quotient functions (oracle/plonk_ref.py). quotient_pieces is the loop create_proof_multi used
to carry inline — upstream's evaluate_h on the whole extended domain, divide_by_vanishing_poly, extended_to_coeff —
and quotient_pieces_on_cosets is the device's default mode stated from its definition: the
interpolant of N(x) / (x^n - 1) over the first cs_degree - 1 cosets of the size-n subgroup. For a satisfying witness
both are the pieces the oracle prover commits to; for arbitrary polynomials they differ (so a GPU test that compares a
key's mode with the matching function can tell the modes apart); when cs_degree - 1 cosets are the whole extended
domain they are the same function."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
SMALL = dict(k=7, num_advice=5, num_lookup_advice=2, lookup_bits=5, num_spread=2, spread_bits=3)


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def random_polys(desc, n, seed):
    """One circuit's polynomials by kind, uniform random coefficients: nothing is satisfied."""
    rng = P.SplitMix64(seed)
    L = len(desc["lookups"])
    chunk = desc["cs_degree"] - 2
    nsets = -(-len(desc["permutation_columns"]) // chunk)
    count = {"advice": desc["num_advice"], "instance": desc["num_instance"], "z": nsets, "lz": L, "la": L, "ls": L}
    return {kind: [[rng.fr() for _ in range(n)] for _ in range(count[kind])] for kind in PR.QUOTIENT_KINDS}


@pytest.mark.parametrize("name", ["lookup5", "rsa7"])
def test_both_functions_give_the_committed_pieces_for_a_satisfying_witness(plonk, name):
    c = circuits.lookup_circuit(plonk, 5) if name == "lookup5" else circuits.rsa_sha256_shape(plonk, **SMALL)
    circuits.check_satisfied(c)
    pk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=7)
    trace = []
    proof = PR.create_proof(pk, c.instances, c.advice, seed=13, trace=trace)
    assert PR.verify_proof(pk, c.instances, proof)
    tr = {t[0]: t[1:] for t in trace}
    (polys,), (theta,), (beta, gamma), (y,) = tr["quotient_polys"][0], tr["theta"], tr["beta_gamma"], tr["y"]
    committed = [t[1] for t in trace if t[0] == "h_piece"]
    # rsa7: degree 4, three of four cosets; lookup5: degree 5, the four cosets are the whole extended domain
    assert len(committed) == c.desc["cs_degree"] - 1 == (3 if name == "rsa7" else 4) and pk.domain.extended_k - pk.k == 2
    num = PR.quotient_numerator(pk, polys, theta, beta, gamma, y)
    full = PR.quotient_pieces(pk, polys, theta, beta, gamma, y, numerator=num)
    cosets = PR.quotient_pieces_on_cosets(pk, polys, theta, beta, gamma, y, numerator=num)
    assert [PR.commit_tau(p, TAU) for p in full] == committed
    assert cosets == full
    assert PR.quotient_pieces_on_cosets(pk, polys, theta, beta, gamma, y) == cosets  # and without a shared numerator


def test_the_two_functions_differ_on_arbitrary_polynomials(plonk):
    """Random polynomials satisfy nothing: X^n - 1 does not divide the numerator, upstream's pieces are a truncation of
    a polynomial of degree up to the extended domain's size, the coset mode's are an interpolant on three cosets. Both
    are well defined and they are not the same — and the coset mode's h really is N / (X^n - 1) on its cosets."""
    c = circuits.rsa_sha256_shape(plonk, **SMALL)
    pk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=7)
    d, n = pk.domain, pk.n
    polys = random_polys(c.desc, n, seed=5)
    theta, beta, gamma, y = (P.SplitMix64(77 + i).fr() for i in range(4))
    num = PR.quotient_numerator(pk, polys, theta, beta, gamma, y)
    full = PR.quotient_pieces(pk, polys, theta, beta, gamma, y, numerator=num)
    cosets = PR.quotient_pieces_on_cosets(pk, polys, theta, beta, gamma, y, numerator=num)
    assert len(full) == len(cosets) == 3 and all(len(p) == n for p in full + cosets)
    assert all(a != b for a, b in zip(full, cosets))
    m = 1 << (d.extended_k - d.k)
    h = [v for piece in cosets for v in piece]
    for cc in range(3):
        for i in (0, 1, n // 2, n - 1):
            x = d.coset_point(cc + m * i)
            assert P.eval_polynomial(h, x) * (pow(x, n, PR.R) - 1) % PR.R == num[cc + m * i]
    # on the coset the default mode leaves out, only upstream's (untruncated) quotient could agree: the interpolant does not
    x = d.coset_point(3)
    assert P.eval_polynomial(h, x) * (pow(x, n, PR.R) - 1) % PR.R != num[3]


def test_the_two_functions_coincide_when_the_cosets_are_the_whole_extended_domain(plonk):
    c = circuits.high_degree_circuit(plonk, 5, power=4)
    pk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=7)
    assert c.desc["cs_degree"] - 1 == 4 == 1 << (pk.domain.extended_k - pk.k)
    for seed in (1, 2):
        polys = random_polys(c.desc, pk.n, seed)
        theta, beta, gamma, y = (P.SplitMix64(100 * seed + i).fr() for i in range(4))
        num = PR.quotient_numerator(pk, polys, theta, beta, gamma, y)
        assert PR.quotient_pieces_on_cosets(pk, polys, theta, beta, gamma, y, numerator=num) == \
            PR.quotient_pieces(pk, polys, theta, beta, gamma, y, numerator=num)
