"""CPU: the gadget circuit of tests/witness_circuits.py against the reference interpreter alone — the witness that
tests/witness_ref.py computes from the program satisfies the circuit the same calls laid out (gates, the 8-bit lookup,
every copy), for edge inputs too, and a hint that is off by one does not."""
import pytest

import circuits
import witness_circuits as WCi
import witness_ref as WR

CASES = [(0, 0), (1, 1), ((1 << 64) - 1, WCi.M - 1), (WCi.M, 12345), (WCi.M - 1, WCi.M - 1), (0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF), (1 << 32, (1 << 32) - 1)]


@pytest.fixture(scope="module")
def gadget(pkg):
    return WCi.MulModGadget(pkg.plonk, pkg.witness.WitnessProgram)


def test_every_advice_cell_is_a_node(gadget):
    cells = {(c, r) for _, c, r in gadget.p.cells}
    assert len(cells) == len(gadget.p.cells) == 2 * gadget.c.n
    assert gadget.p.plan(4)["levels"] > 10


@pytest.mark.parametrize("x,y", CASES)
def test_reference_witness_satisfies_the_circuit(gadget, x, y):
    values = WR.evaluate(gadget.p, gadget.inputs(x, y))
    adv, inst = gadget.witness(values)
    assert inst == [[x * y % WCi.M, x]]
    circuits.check_satisfied(gadget.c, advice=adv, instances=inst)


@pytest.mark.parametrize("err", [1, -1])
def test_a_hint_off_by_one_breaks_it(gadget, err):
    x, y = CASES[5]
    adv, inst = gadget.witness(WR.evaluate(gadget.p, gadget.inputs(x, y, hint_error=err)))
    with pytest.raises(AssertionError):
        circuits.check_satisfied(gadget.c, advice=adv, instances=inst)
