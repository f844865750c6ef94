"""CPU: the reference of the witness check (tests/witness_check_ref.py) against workloads.check_satisfied — both accept
the satisfied fixtures, and on hand-corrupted ones the reference's first entry is the failure check_satisfied stops at
(its walk is gates by index, then lookups, then copies, rows ascending: the report's order)."""
import re

import pytest

import circuits
import witness_check_ref as W


@pytest.fixture(scope="module")
def plonk(pkg):
    return pkg.plonk


def fixtures(plonk):
    return [circuits.square_circuit(plonk, 4), circuits.high_degree_circuit(plonk), circuits.lookup_circuit(plonk, 5, seed=2),
            circuits.lookup_circuit(plonk, 5, seed=2, tables="pair_first")] + [circuits.random_circuit(plonk, 6, seed=s) for s in range(6)]


def test_satisfied_fixtures_give_an_empty_report(plonk):
    for c in fixtures(plonk):
        assert circuits.check_satisfied(c)
        assert W.report(c) == []


def first_failure_of_check_satisfied(c):
    try:
        circuits.check_satisfied(c)
    except AssertionError as e:
        m = re.match(r"(gate|lookup) (\d+) fails at row (\d+)|copy constraint fails at col (\d+) row (\d+)", str(e))
        assert m, str(e)
        if m.group(1):
            return (W.GATE if m.group(1) == "gate" else W.LOOKUP, int(m.group(2)), int(m.group(3)))
        return (W.COPY, int(m.group(4)), int(m.group(5)))
    return None


def test_hand_corrupted_fixtures_agree_with_check_satisfied(plonk):
    R = circuits.R
    # a mul gate's output: polynomial 0 of the lookup circuit, at the corrupted row only
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    c.advice[2][0] = (c.advice[2][0] + 1) % R
    rep = W.report(c)
    assert rep[0] == (W.GATE, 0, 0, 1) and first_failure_of_check_satisfied(c) == rep[0][:3]
    # a range-lookup input outside the table, on the first row whose range selector is on
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    q_rng = c.desc["lookups"][0]["inputs"][0][1]  # the input is q_rng * a
    assert q_rng[0] == "fixed"
    row = next(r for r in range(1, c.usable) if c.fixed[q_rng[1]][r] == 1)
    c.advice[0][row] = 1000
    rep = W.report(c)
    assert (W.LOOKUP, 0, row, 1) in rep and first_failure_of_check_satisfied(c) == rep[0][:3]
    # a copied cell: both ends of the two-cycle are reported, one row each
    c = circuits.high_degree_circuit(plonk)
    c.advice[0][5] = (c.advice[0][5] + 1) % R
    rep = W.report(c)
    assert (W.COPY, 0, 2, 2) in rep and rep[0][0] == W.GATE and first_failure_of_check_satisfied(c) == rep[0][:3]
    # the square circuit's only gate, and nothing else
    c = circuits.square_circuit(plonk, 4)
    c.advice[1][0] = 26
    assert W.report(c) == [(W.GATE, 0, 0, 1)] and first_failure_of_check_satisfied(c) == (W.GATE, 0, 0)


def test_rows_behind_the_usable_ones(plonk):
    """A gate violated only at rows >= u is not reported; a copy constraint is checked on all n rows."""
    c = circuits.square_circuit(plonk, 4)
    c.fixed[0][c.usable] = 1
    c.advice[1][c.usable] = 3
    assert W.Walk(c).gate_fails_at(0, c.usable) and W.report(c) == []
    c.fixed[0][c.usable - 1] = 1
    c.advice[1][c.usable - 1] = 3
    assert W.report(c) == [(W.GATE, 0, c.usable - 1, 1)]
