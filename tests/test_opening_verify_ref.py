"""CPU: tests/opening_verify_ref.py — the reference of amdzk_multiopen_verify — held to the oracle's own provers: for the
openings plonk_ref.shplonk_prove / gwc_prove write over tests/multiopen_cases.py's query shapes, tau * L == R with the tau
of the test SRS; for a wrong evaluation, a wrong commitment, swapped read points and another tau it is not. Duplicate
queries and a second index for one point value change nothing."""
import pytest

import multiopen_cases as MC
import opening_verify_ref as OV
import plonk_ref as PR
import pyref as P

TAU, R = MC.TAU, OV.R
CASES = [("one", "shplonk"), ("one", "gwc"), ("shared", "shplonk"), ("shared", "gwc"), ("17 sets", "shplonk"), ("17 sets", "gwc"),
         ("17 points", "shplonk"), ("17 points", "gwc"), ("top 10", "shplonk"), ("top 10", "gwc")]


@pytest.mark.parametrize("name,scheme", CASES)
def test_reference_accepts_the_oracles_openings_and_nothing_else(name, scheme):
    case = MC.make_case(name)
    coms, evals, proof = OV.opening_of(case, scheme, TAU)
    T = PR.Blake2bRead(proof)
    ch, pts = OV.read(scheme, T, case.point_vals, case.queries)
    assert T.pos == len(proof) and len(pts) == OV.n_read(scheme, case.point_vals, case.queries)
    lr = OV.pair(scheme, coms, case.point_vals, case.queries, evals, ch, pts)
    assert OV.holds(lr, TAU) and not OV.holds(lr, TAU + 1)
    wrong_eval = list(evals)
    wrong_eval[0] = (wrong_eval[0] + 1) % R  # query 0 is the first of its (commitment, point) pair: both schemes read it
    assert not OV.holds(OV.pair(scheme, coms, case.point_vals, case.queries, wrong_eval, ch, pts), TAU)
    wrong_com = list(coms)
    wrong_com[case.queries[0][0]] = P.g1_add(wrong_com[case.queries[0][0]], P.G1_GEN)
    assert not OV.holds(OV.pair(scheme, wrong_com, case.point_vals, case.queries, evals, ch, pts), TAU)
    if len(pts) > 1:
        assert (pts[0] != pts[1]) == (name != "one")  # one polynomial at one point: h2 = h1 (l(X) = (X - u) h(X), z_0 = 1)
    if len(pts) > 1 and pts[0] != pts[1]:
        assert not OV.holds(OV.pair(scheme, coms, case.point_vals, case.queries, evals, ch, [pts[1], pts[0]] + pts[2:]), TAU)


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_an_identity_commitment_and_renamed_points_are_handled(scheme):
    case = MC.make_case("shared")
    case.polys[2] = [0] * case.n  # commits to the identity
    coms, evals, proof = OV.opening_of(case, scheme, TAU)
    assert coms[2] is None
    ch, pts = OV.read(scheme, PR.Blake2bRead(proof), case.point_vals, case.queries)
    lr = OV.pair(scheme, coms, case.point_vals, case.queries, evals, ch, pts)
    assert OV.holds(lr, TAU)
    # point index 5 carries the value of index 1: naming either is the same opening
    renamed = [(c, 1 if z == 5 else z) for c, z in case.queries]
    assert OV.pair(scheme, coms, case.point_vals, renamed, evals, ch, pts) == lr
