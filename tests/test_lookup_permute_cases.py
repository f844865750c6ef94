"""CPU: the cases of tests/lookup_permute_cases.py are what their names claim, and the two judges the GPU test relies on
— the oracle's permute_expression_pair and the definition written out in check_definition — agree on every one of them.
A device result is compared with the reference exactly; this file is why that reference can be trusted on these inputs."""
import pytest

import lookup_permute_cases as LC

R = LC.R
TAIL = 6  # rows beyond `usable` in the columns handed to the judges


def every_key():
    return [v for keys in LC.KEY_SETS.values() for v in keys]


def test_ladder_pairs_are_ordered_by_limb_j_alone():
    assert len(LC.LADDER_PAIRS) == 28 and len(LC.KEY_SETS["limb_ladder"]) == 56 + 14
    for i, j, lo, hi in LC.LADDER_PAIRS:
        assert i < j and lo < hi
        assert [LC.limb(lo, m) for m in range(8)] == [2 if m == i else 1 if m == j else 0 for m in range(8)]
        assert [LC.limb(hi, m) for m in range(8)] == [1 if m == i else 2 if m == j else 0 for m in range(8)]
        # limb i says the opposite: whoever ranks it above limb j, or reads the limbs from the bottom, misorders the pair
        assert LC.limb(lo, i) > LC.limb(hi, i) and LC.limb(lo, j) < LC.limb(hi, j)
    for i in range(1, 8):
        below, at = LC.LADDER_CARRIES[2 * (i - 1)], LC.LADDER_CARRIES[2 * (i - 1) + 1]
        assert at == 1 << (32 * i) and below == at - 1
        assert all(LC.limb(below, m) == 0xFFFFFFFF for m in range(i)) and LC.limb(at, i) == 1 and LC.limb(below, i) == 0


def test_sign_pairs_are_misordered_by_a_signed_limb_compare():
    assert [i for i, _, _ in LC.SIGN_PAIRS] == list(range(7))
    for i, lo, hi in LC.SIGN_PAIRS:
        assert lo < hi and hi - lo == 1 << (32 * i)
        assert LC.limb(lo, i) == 0x7FFFFFFF and LC.limb(hi, i) == 0x80000000
        assert all(LC.limb(lo, m) == LC.limb(hi, m) == 1 for m in range(8) if m != i)
        assert LC.signed_limb_less(hi, lo) and not LC.signed_limb_less(lo, hi)
    # the model is the unsigned order wherever no limb has its top bit set
    for _, _, lo, hi in LC.LADDER_PAIRS:
        assert LC.signed_limb_less(lo, hi) and not LC.signed_limb_less(hi, lo)


def test_keys_are_canonical_and_the_pads_are_foreign():
    keys = every_key()
    assert all(0 <= v < R for v in keys) and len(set(keys)) == len(keys)
    assert LC.KEY_SETS["edges"] == [0, 1, R - 1, R - 2, (R >> 232 << 232) - 1, 1 << 253]
    fillers = [LC.filler(t) for t in range(1 << 14)]
    assert len(set(fillers)) == len(fillers) and not set(fillers) & set(keys) and max(fillers) < R
    assert LC.TABLE_PAD < R and LC.INPUT_PAD == R - 1
    for n in LC.SIZES:
        for u in LC.default_usable(n):
            for name, inp, tab in LC.cases(u):
                assert LC.TABLE_PAD not in inp and LC.TABLE_PAD not in tab, (n, name)


@pytest.mark.parametrize("n", LC.SIZES)
def test_every_case_is_well_formed(n):
    for u in LC.default_usable(n):
        assert 0 < u <= n
        seen = set()
        for name, inp, tab in LC.cases(u):
            assert len(inp) == u and len(tab) == u and inp == sorted(inp), (n, name)
            assert all(0 <= v < R for v in inp + tab), (n, name)
            assert set(inp) <= set(tab), (n, name)  # a lookup asks for the values, not for their multiplicity
            seen.add(name)
        # every key of every key set is in some chunk, every 0-1 split is there
        for kname, keys in LC.KEY_SETS.items():
            got = [v for name, inp, _ in LC.cases(u) if name.startswith(kname + "[") for v in inp if v in keys]
            assert sorted(got) == sorted(keys), (n, kname)
        assert {"zero_one[%d]" % s for s in (0, 1, u // 2, u - 1, u)} <= seen
        assert set(LC.MULTISETS) <= seen


def test_the_multisets_are_the_existing_ones():
    for u in (58, 122, 1018):  # tests/test_gpu_plonk_ops.py runs them at these
        assert LC.MULTISETS["all_equal"](u) == ([5] * u, [5] + list(range(100, 100 + u - 1)))
        assert LC.MULTISETS["many_leftovers"](u) == ([3, 3, 3, 9, 9, 1] * (u // 6) + [1] * (u % 6), [1, 3, 9] + list(range(1000, 1000 + u - 3)))
        assert LC.MULTISETS["table_with_repeats"](u) == ([i % 3 for i in range(u)], [0, 1, 2] + [0] * (u - 3))


@pytest.mark.parametrize("u", [1, 2, 3, 7, 58, 250, 4090])
def test_orders_are_permutations_with_the_shape_their_name_says(u):
    for name, order in LC.ORDERS.items():
        assert sorted(order(u)) == list(range(u)), name
    assert LC.ORDERS["ascending"](u) == sorted(LC.ORDERS["ascending"](u))
    assert LC.ORDERS["descending"](u) == sorted(LC.ORDERS["descending"](u), reverse=True)
    pipe = LC.ORDERS["organ_pipe"](u)
    top = pipe.index(u - 1)
    assert pipe[:top + 1] == sorted(pipe[:top + 1]) and pipe[top:] == sorted(pipe[top:], reverse=True)
    bits = max(1, (u - 1).bit_length())
    assert LC.ORDERS["bit_reversed"](1 << bits) == [int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)]
    if u > 7:
        assert LC.ORDERS["shuffle"](u) not in (LC.ORDERS["ascending"](u), LC.ORDERS["descending"](u))


def judge_both(inp, tab, u, where):
    a, s = LC.reference(inp + [LC.INPUT_PAD] * TAIL, tab + [LC.TABLE_PAD] * TAIL, u)
    assert len(a) == u and len(s) == u, where
    assert LC.check_definition(inp + [LC.INPUT_PAD] * TAIL, tab + [LC.TABLE_PAD] * TAIL, u, a, s) is None, where
    return a, s


@pytest.mark.parametrize("n", LC.SIZES)
def test_reference_and_definition_agree_on_every_case(n):
    for u in LC.default_usable(n):
        for name, inp, tab in LC.cases(u):
            a, s = judge_both(inp, tab, u, (n, u, name))
            # the input's order does not enter: one shuffled column per case
            assert LC.reference(LC.ordered(inp, "shuffle"), tab, u) == (a, s), (n, u, name)


@pytest.mark.parametrize("u", [0, 1, 2, 63, 64, 4095, 4096, 4097, 8191, 8192])
def test_reference_and_definition_agree_at_the_usable_row_counts(u):
    if u == 0:
        assert LC.reference([LC.INPUT_PAD] * TAIL, [LC.TABLE_PAD] * TAIL, 0) == ([], [])
        assert LC.check_definition([LC.INPUT_PAD] * TAIL, [LC.TABLE_PAD] * TAIL, 0, [], []) is None
        return
    for name in ("all_equal", "many_leftovers"):
        _, inp, tab = LC.multiset_case(name, u)
        judge_both(inp, tab, u, (u, name))


def test_the_definition_refuses_what_is_not_the_permuted_pair():
    u = 12
    _, inp, tab = LC.multiset_case("many_leftovers", u)
    a, s = LC.reference(inp, tab, u)
    assert LC.check_definition(inp, tab, u, a, s) is None
    assert "sorted" in LC.check_definition(inp, tab, u, a[::-1], s)
    assert "permutation" in LC.check_definition(inp, tab, u, a, s[:-1] + [s[0]])
    rep = [r for r in range(1, u) if a[r] == a[r - 1]]
    first = [r for r in range(u) if r not in rep]
    swapped = list(s)
    swapped[rep[0]], swapped[rep[-1]] = swapped[rep[-1]], swapped[rep[0]]
    assert swapped != s and "ascending" in LC.check_definition(inp, tab, u, a, swapped)
    moved = list(s)
    moved[first[1]], moved[rep[0]] = moved[rep[0]], moved[first[1]]
    assert "starts a run" in LC.check_definition(inp, tab, u, a, moved)
    with pytest.raises(AssertionError):
        LC.reference([4] + inp[1:], tab, u)  # 4 is not in the table


def test_launch_plan_is_the_closed_form():
    """n = 2048 * 2^m: 1 + m launches of the LDS kernel, m (m + 1) / 2 of the global one; one LDS launch up to a tile."""
    for n in LC.SIZES + [1024, 8192, 1 << 18]:
        plan = LC.launch_plan(n, n - 1, 3)
        m = max(0, (n // LC.SORT_TILE).bit_length() - 1)
        assert plan.get("sort_bitonic_lds") == 1 + m and plan.get("sort_bitonic_global", 0) == m * (m + 1) // 2, n
        assert (plan["lookup_mark"], plan["lookup_flag_scan"], plan["lookup_compact"], plan["lookup_assign"]) == (1, 2, 1, 1)
    assert LC.launch_plan(64, 0, 1) == {} and LC.launch_plan(64, 58, 0) == {}
