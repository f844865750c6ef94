"""CPU: tests/poseidon_ref.py — the reference of the Poseidon tests — against closed forms it cannot share a mistake with."""
import pytest

import poseidon_cases as PC
import poseidon_ref as PR

R = PR.R


@pytest.mark.parametrize("t,r_f,r_p", [(2, 2, 0), (3, 2, 1), (5, 8, 57), (8, 4, 3)])
def test_identity_matrix_and_zero_constants_leave_powers(t, r_f, r_p):
    """M = identity, no constants: an element is only ever raised to the fifth power — element 0 in every round, the
    others in the full rounds."""
    s = PR.Spec(t, 1, r_f, r_p, [[0] * t for _ in range(r_f + r_p)], [[int(i == j) for j in range(t)] for i in range(t)])
    for state in PC.states(t, 7):
        got = PR.permute(s, state)
        assert got[0] == pow(state[0], 5 ** (r_f + r_p), R)
        assert got[1:] == [pow(x, 5 ** r_f, R) for x in state[1:]]


@pytest.mark.parametrize("t", [2, 3, 8])
def test_two_full_rounds_expanded_by_hand(t):
    s = PC.spec(t, 1, 2, 0)
    for x in PC.states(t, 6):
        a = [(x[i] + s.rc[0][i]) ** 5 for i in range(t)]
        b = [sum(s.mds[i][j] * a[j] for j in range(t)) for i in range(t)]
        c = [(b[i] + s.rc[1][i]) ** 5 for i in range(t)]
        want = [sum(s.mds[i][j] * c[j] for j in range(t)) % R for i in range(t)]  # exact integers, reduced once
        assert PR.permute(s, x) == want


def test_a_partial_round_takes_the_s_box_on_element_0_only():
    t = 3
    s = PC.spec(t, 2, 2, 1)
    x = PC.states(t, 5)[4]
    a = [pow(x[i] + s.rc[0][i], 5, R) for i in range(t)]
    b = [sum(s.mds[i][j] * a[j] for j in range(t)) % R for i in range(t)]
    c = [(b[i] + s.rc[1][i]) % R for i in range(t)]
    c[0] = pow(c[0], 5, R)
    d = [sum(s.mds[i][j] * c[j] for j in range(t)) % R for i in range(t)]
    e = [pow(d[i] + s.rc[2][i], 5, R) for i in range(t)]
    assert PR.permute(s, x) == [sum(s.mds[i][j] * e[j] for j in range(t)) % R for i in range(t)]


@pytest.mark.parametrize("t,rate", [(2, 1), (5, 4), (5, 2), (8, 7)])
def test_sponge_permutation_count_and_padding(t, rate):
    s = PC.spec(t, rate, 2, 1, init=(t == 5))
    for length in (0, 1, rate - 1, rate, rate + 1, 2 * rate, 37):
        data = PC.inputs(length, "ref")
        seen = []

        def spy(spec, state):
            seen.append(list(state))
            return PR.permute(spec, state)

        digest = PR.sponge(s, data, permute_fn=spy)
        assert len(seen) == length // rate + 1
        # what went into the last permutation: the state before it plus the left-over followed by ONE, nothing beyond
        before = PR.permute(s, seen[-2]) if len(seen) > 1 else s.initial_state()
        m = length % rate
        tail = data[length - m:] + [1] if m else [1]
        want = list(before)
        for i, v in enumerate(tail):
            want[1 + i] = (want[1 + i] + v) % R
        assert seen[-1] == want and len(tail) == m + 1 <= rate
        assert digest == PR.permute(s, seen[-1])[1]
    assert PR.Spec(3, 2, 2, 0, [[0] * 3] * 2, [[0] * 3] * 3).initial_state() == [1 << 64, 0, 0]
