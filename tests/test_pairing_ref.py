"""CPU: self-checks of tests/pairing_ref.py, the integer reference the pairing unit is pinned against: the published
constants, non-degeneracy, order, bilinearity. Nine pairings in all (the reference caches per process)."""
import pairing_ref as X

A, B = 0x1F2E3D4C5B6A79881726354453627180, 0x0123456789ABCDEFFEDCBA9876543210F


def P(k):
    return X.g1_mul(X.G1_GEN, k)


def Qk(k):
    return X.g2_mul(X.G2_GEN, k)


def test_the_g2_generator_is_on_the_twist_and_has_order_r():
    assert X.g2_on_curve(X.G2_GEN)
    assert X.g2_mul(X.G2_GEN, X.R) is None and X.g2_mul(X.G2_GEN, X.R - 1) == X.g2_neg(X.G2_GEN)
    assert X.g1_mul(X.G1_GEN, X.R) is None


def test_the_hard_part_decomposition_the_device_chain_uses_is_the_exact_exponent():
    u, p = X.U, X.P
    l0, l1, l2 = -36 * u**3 - 30 * u**2 - 18 * u - 2, -36 * u**3 - 18 * u**2 - 12 * u + 1, 6 * u**2 + 1
    assert l0 + l1 * p + l2 * p**2 + p**3 == (p**4 - p**2 + 1) // X.R
    assert (p**12 - 1) // X.R == (p**6 - 1) * (p**2 + 1) * ((p**4 - p**2 + 1) // X.R)
    assert X.ATE == 0x19D797039BE763BA8


def test_the_pairing_of_the_generators_is_not_one_and_has_order_r():
    e = X.pairing(X.G1_GEN, X.G2_GEN)
    assert e != X.F12_ONE
    assert X.f12_pow(e, X.R) == X.F12_ONE


def test_bilinearity_for_one_random_pair_of_scalars():
    e = X.pairing(X.G1_GEN, X.G2_GEN)
    assert X.pairing(P(A), Qk(B)) == X.f12_pow(e, A * B % X.R)


def test_additivity_in_each_argument():
    e = X.pairing(X.G1_GEN, X.G2_GEN)
    ea, eb = X.pairing(P(A), X.G2_GEN), X.pairing(X.G1_GEN, Qk(B))
    assert X.pairing(X.g1_add(P(A), X.G1_GEN), X.G2_GEN) == X.f12_mul(ea, e)
    assert X.pairing(X.G1_GEN, X.g2_add(Qk(B), X.G2_GEN)) == X.f12_mul(eb, e)


def test_negation_inverts():
    e = X.pairing(X.G1_GEN, X.G2_GEN)
    assert X.f12_mul(X.pairing(X.g1_neg(X.G1_GEN), X.G2_GEN), e) == X.F12_ONE
    # and a product of Miller values under one final exponentiation is the product of the pairings
    assert X.pairing_product([(X.G1_GEN, X.G2_GEN), (None, X.G2_GEN), (X.g1_neg(X.G1_GEN), X.G2_GEN)]) == X.F12_ONE


def test_tower_order_of_the_polynomial_basis():
    # u = w^6 - 9: the element u w (c1.c0 = (0, 1)) is w^7 - 9 w
    a = [0] * 12
    a[7], a[1] = 1, -9 % X.P
    t = X.f12_to_tower(tuple(a))
    assert t == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    assert X.f12_to_tower(X.F12_ONE) == [1] + [0] * 11
