"""CPU: the wide accumulator of fp29_model.py (reference B of csrc/fp29.cuh f29_wide_*) at the length lincomb_kernel and
poly_eval_kernel drive it to — 255 and 256 unreduced products in 17 un-carried columns with a carry pass every sixth
term — on the operands tests/test_gpu_plonk_operands.py sends to the device. fp29_model.class_wide stops at 18 terms.

What this pins is the reference, not the device: with every documented precondition an assertion and every accumulator
checked against its width, the model accepts these sums, returns the right residue, and hands f29_reduce_weak a value it
accepts. A device result that differs on the same operands is therefore the kernel's fault."""
import fp29_model as M
import pytest

FR, R = M.FR, M.R
T = R >> 232  # the top limb of r
RM1 = M.digits(R - 1)
T232M1 = M.digits((T << 232) - 1)  # low eight limbs all ones, top limb T - 1: the largest such value below r
HOT = [M.MASK] * 8 + [FR.P[8]]  # low eight limbs all ones under r's own top limb: above r, below 2r (a product's range)
TWO_P_M1 = M.digits(2 * R - 1)  # the bound of a power-table entry (f29_mul returns values below 2p), normalised
EXTREME = {"rm1": RM1, "t232m1": T232M1, "hot": HOT}
# a coefficient / point / root word w enters the kernels as 32 w mod r (fr29_const_to_r261): the word whose image has all
# low limbs set
W_ALL_ONES = ((T << 232) - 1) * pow(32, -1, R) % R


def test_the_operands_are_what_their_names_say():
    assert T232M1 == [M.MASK] * 8 + [T - 1] and M.val(T232M1) < R < M.val(HOT) < 2 * R and FR.P[8] == T
    assert W_ALL_ONES < R and 32 * W_ALL_ONES % R == (T << 232) - 1
    assert M.digits(32 * W_ALL_ONES % R) == T232M1
    assert all(x < 1 << 29 for x in TWO_P_M1) and M.val(TWO_P_M1) == 2 * R - 1


def _sum_and_reduce(a, b, nterms):
    r, total = M.wide_sum(FR, [(a, b)], nterms)
    assert total == nterms * M.val(a) * M.val(b)
    assert all(x < 1 << 29 for x in r[:8]) and M.val(r) % R == M.mont_redc(FR, total)
    assert M.val(r) < total // M.RADIX + R + 1  # the reduction's own bound: T / 2^261 + p
    w = M.f29_reduce_weak(FR, r)
    assert all(x < 1 << 29 for x in w[:8]) and M.val(w) % R == M.mont_redc(FR, total) and M.val(w) < 2 * R  # f29_pack_canonical's range
    return M.val(r)


@pytest.mark.parametrize("nterms", [255, 256])
@pytest.mark.parametrize("b", sorted(EXTREME))
@pytest.mark.parametrize("a", sorted(EXTREME))
def test_wide_sum_of_256_extreme_products(a, b, nterms):
    """Every ordered pair of the three extreme operands, 255 and 256 times: accepted, right residue, and the result (below
    2.6 p for canonical operands, lincomb_kernel's figure; below 4.1 p with both in a product's range) goes through
    f29_reduce_weak."""
    v = _sum_and_reduce(EXTREME[a], EXTREME[b], nterms)
    canonical = "hot" not in (a, b)
    assert v * 10 < (26 if canonical else 41) * R


@pytest.mark.parametrize("nterms", [255, 256])
@pytest.mark.parametrize("a", sorted(EXTREME))
def test_wide_sum_with_a_power_table_entry_at_its_bound(a, nterms):
    """poly_eval_kernel: the second operand is an entry of the power table, any value below 2p. 256 terms of (data, 2p - 1)
    stay below 256 * 2 / 169.3 + 1 < 4.1 p (the kernel's comment)."""
    v = _sum_and_reduce(EXTREME[a], TWO_P_M1, nterms)
    assert v * 10 < 41 * R


@pytest.mark.parametrize("name,a", [("t232m1", T232M1), ("hot", HOT)])
def test_the_carry_group_has_room_up_to_eight(monkeypatch, name, a):
    """The kernels carry after every sixth term (fp29_model.WIDE_GROUP). On the all-ones operand a group of seven and of
    eight still fits the 64-bit columns; nine does not: the margin the group of six has."""
    assert M.WIDE_GROUP == 6
    for group in (7, 8):
        monkeypatch.setattr(M, "WIDE_GROUP", group)
        _sum_and_reduce(a, a, 256)
    monkeypatch.setattr(M, "WIDE_GROUP", 9)
    with pytest.raises(M.OverflowError_, match="64-bit accumulator overflow"):
        M.wide_sum(FR, [(a, a)], 256)
