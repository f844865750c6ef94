"""CPU: the identity behind AMDZK_BASIS_G_LAGRANGE_PREFIX, on integers and on the pure-Python curve (oracle/pyref.py), n = 8.

    sum_i Z[i] L_i = sum_i D[i] S_i,   S_i = L_0 + ... + L_i,   D[i] = Z[i] - Z[i+1] for i < n-1,   D[n-1] = Z[n-1]

(Abel summation: sum_i D[i] S_i = sum_j L_j sum_{i >= j} D[i], and the inner sum telescopes to Z[j].) The device commits the
permutation products this way: D is zero wherever Z does not change."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402

N = 8


def differences(z, mod):
    n = len(z)
    d = [(z[i] - z[i + 1]) % mod for i in range(n - 1)]
    d.append(z[n - 1] % mod)  # D[n-1] = Z[n-1]: nothing follows the last row
    return d


def prefix(xs, add, zero):
    out, acc = [], zero
    for x in xs:
        acc = add(acc, x)
        out.append(acc)
    return out


COLUMNS = {
    "random": [0x1234567 * (i + 3) ** 5 % P.R for i in range(N)],
    "all_equal": [77] * N,
    "one_jump_at_row_0": [5] + [9] * (N - 1),
    "jumps_at_n-2_and_n-1": [4] * (N - 1) + [P.R - 1],
    "zeros": [0, 0, 3, 3, 0, 0, 0, 8],
    "all_zero": [0] * N,
    "blinded_tail": [1, 1, 1, 6, 6] + [P.R - 2, 12345, 1 << 200],
}


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_identity_on_integers(name):
    """The 'basis' is a list of integers mod a prime: the identity is plain algebra, for any basis."""
    z = COLUMNS[name]
    basis = [(31 * i * i + 7 * i + 1) % P.R for i in range(N)]
    s = prefix(basis, lambda a, b: (a + b) % P.R, 0)
    d = differences(z, P.R)
    assert d[N - 1] == z[N - 1] % P.R
    assert sum(a * b for a, b in zip(z, basis)) % P.R == sum(a * b for a, b in zip(d, s)) % P.R
    # a constant run of Z gives zero differences inside it
    assert all(d[i] == 0 for i in range(N - 1) if z[i] == z[i + 1])


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_identity_on_curve_points(name):
    z = COLUMNS[name]
    gen = (1, 2)
    basis = [P.g1_mul(gen, 1000003 * (i + 1) ** 3 + 11) for i in range(N)]
    s = prefix(basis, P.g1_add, None)
    d = differences(z, P.R)
    assert P.msm_naive(z, basis) == P.msm_naive(d, s)


def test_prefix_sums_of_a_lagrange_basis_end_in_the_generator_multiple():
    """sum_i L_i(X) = 1: the last prefix sum of g_lagrange is g[0] — the constant polynomial 1 commits to the same point in
    either basis. Here with L_i(tau) G for the domain of size 8."""
    tau, w = 0xABCDEF, P.omega(3)
    tn1, ninv = (pow(tau, N, P.R) - 1) % P.R, pow(N, -1, P.R)
    lag = [pow(w, i, P.R) * tn1 % P.R * ninv % P.R * pow((tau - pow(w, i, P.R)) % P.R, -1, P.R) % P.R for i in range(N)]
    assert sum(lag) % P.R == 1
    gl = [P.g1_mul((1, 2), v) for v in lag]
    s = prefix(gl, P.g1_add, None)
    assert s[0] == gl[0] and s[N - 1] == (1, 2)
