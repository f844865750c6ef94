"""CPU: the references of tests/srs_unit_ref.py against the oracle's own restatements, and the COVERAGE CONDITIONS of
tests/test_gpu_srs_unit.py — that its chosen inputs take the device through the degenerate additions they are chosen for —
asserted from the simulators, so they hold whether or not a GPU is there."""
import numpy as np
import pytest

import srs_unit_ref as S
import zkutil as zu

import plonk_ref as PR  # srs_unit_ref put oracle/ on the path
import pyref as P

Q, R = S.Q, S.R


# ------------------------------------------------------------------------------------------------ number facts
def test_number_facts():
    assert Q.bit_length() == 254 and Q % 4 == 3
    assert pow(3, (Q - 1) // 2, Q) == Q - 1  # 3 is a non-residue: x = 0 has no point
    for x in (4, 10):
        assert pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == Q - 1, x  # off the curve
    for x in (2, 3):  # ... and the smallest x above 1 that no point has is 4
        assert S.g1_y_from_x(x, 0) is not None
    for x in (1, Q - 1):
        assert pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == 1, x  # on the curve
    assert S.g1_y_from_x(1, 0) == 2 and S.g1_y_from_x(1, 1) == Q - 2
    assert (Q + 1) % Q == 1 and Q + 1 < 1 << 254  # x = q + 1 is the generator's x, not canonical, bit 254 clear


# ------------------------------------------------------------------------------------------------ the codec
def test_decompress_inverts_compress_on_random_points():
    rng = P.SplitMix64(5)
    for _ in range(24):
        p = P.g1_mul(P.G1_GEN, rng.fr())
        for pt in (p, P.g1_neg(p)):
            assert S.g1_decompress(PR.g1_compress(pt)) == ("point", pt)
    assert S.g1_decompress(PR.g1_compress(None)) == ("identity", None)


def test_codec_classes():
    for name, b in S.ACCEPTED_ENCODINGS:
        kind, pt = S.g1_decompress(b)
        assert kind == ("identity" if name == "identity" else "point"), name
        assert PR.g1_compress(pt) == b, name
        if pt is not None:
            assert P.g1_on_curve(pt) and (pt[1] & 1) == b[31] >> 7, name
    reasons = {name: S.g1_decompress(b) for name, b in S.REFUSED_ENCODINGS}
    assert all(kind == "refused" for kind, _ in reasons.values()), reasons
    assert {n for n, (_, why) in reasons.items() if why == "x >= q"} == {"x_eq_q", "x_eq_q_plus_1", "x_1_bit_254", "all_ff"}
    assert len(S.REFUSED_ENCODINGS) == 9 and len({b for _, b in S.REFUSED_ENCODINGS}) == 9


def test_edge_points():
    pts = dict(S.edge_points())
    assert all(P.g1_on_curve(p) for p in pts.values())
    assert pts["gen"] == (1, 2) and pts["neg_gen"] == (1, Q - 2)
    assert pts["x_qm1_even"][0] == pts["x_qm1_odd"][0] == Q - 1 and pts["x_qm1_even"][1] & 1 == 0 and pts["x_qm1_odd"][1] & 1 == 1
    assert pts["x_bit_253"][0] >> 253 == 1
    assert 1 < pts["x_small_even"][0] < 1 << 32 and pts["x_small_even"][1] & 1 == 0 and pts["x_small_odd"][1] & 1 == 1
    for name, p in pts.items():
        assert S.g1_decompress(PR.g1_compress(p)) == ("point", p), name


# ------------------------------------------------------------------------------------------------ the group FFT
@pytest.mark.parametrize("k", [0, 1, 2, 3, 6, 10])
def test_ecfft_sim_is_best_fft_bit_reversed(k):
    n = 1 << k
    rng = P.SplitMix64(40 + k)
    a = [rng.fr() for _ in range(n)]
    state, out, kinds = S.ecfft_sim(a, k)
    want = P.best_fft(a, pow(P.omega(k), -1, R) if k else 1, k)
    assert [state[S.brev(i, k)] for i in range(n)] == want
    assert out == [x * pow(n, -1, R) % R for x in want]
    assert len(kinds) == k and all(len(row) == n // 2 for row in kinds)


def test_ecfft_sim_against_points_k3():
    """On points: the simulator's output times G is pyref.g_to_lagrange of the a_i G, with an identity, a repeated point and
    an opposite pair in the input; and its classes name them."""
    rng = P.SplitMix64(3)
    a = [rng.fr() for _ in range(8)]
    a[2], a[5], a[7] = 0, a[1], R - a[3]  # round 0 pairs (1, 5) and (3, 7), and (2, 6)
    _, out, kinds = S.ecfft_sim(a, 3)
    assert kinds[0] == ["gen", "eq", "u0", "neg"]
    got = P.g_to_lagrange([P.g1_mul(P.G1_GEN, x) for x in a], 3)
    assert got == [P.g1_mul(P.G1_GEN, x) for x in out]


def test_ecfft_round0_inverts():
    k = 6
    rng = P.SplitMix64(9)
    t = [rng.fr() for _ in range(1 << k)]
    a = S.ecfft_invert_round0(t, k)
    b = list(a)
    half = 1 << (k - 1)
    w = pow(P.omega(k), -1, R)
    for j in range(half):
        u, v = b[j], b[j + half]
        b[j], b[j + half] = (u + v) % R, (u - v) * pow(w, j, R) % R
    assert b == t


def ecfft_degenerate_counts(k=10):
    a = S.ecfft_degenerate_input(k)
    _, out, kinds = S.ecfft_sim(a, k)
    return a, out, kinds


def test_ecfft_degenerate_input_coverage():
    """k = 10: threads 256.. of a round are its blocks 1 and up. Round 1 there holds at least 40 of every kind; rounds 2 and 3
    meet the identities round 1 made. Round 0, the inverted one, is general except where the chosen state holds a zero (a zero
    sum is an opposite pair, a zero difference an equal pair)."""
    a, out, kinds = ecfft_degenerate_counts(10)
    assert S.butterfly_counts(kinds[0])["gen"] >= 128
    c1 = S.butterfly_counts(kinds[1], first_thread=256)
    assert sum(c1.values()) == 256 and all(c1[kind] >= 40 for kind in S.BUTTERFLY_KINDS), c1
    for s in (2, 3):
        c = S.butterfly_counts(kinds[s], first_thread=256)
        assert all(c[kind] >= 1 for kind in ("u0", "v0", "u0v0")), (s, c)
    assert sum(1 for x in out if x == 0) < 8  # the output is no trivial one


# ------------------------------------------------------------------------------------------------ the prefix scan
def test_prefix_level_sizes():
    assert [S.prefix_level_sizes(1 << k) for k in (4, 5, 8, 9, 10, 13)] == [
        [16], [32, 2], [256, 16], [512, 32, 2], [1024, 64, 4], [8192, 512, 32, 2]]


@pytest.mark.parametrize("n", [1, 15, 16, 17, 100, 256, 300])
def test_prefix_sim_is_a_prefix_sum(n):
    rng = P.SplitMix64(n)
    a = [rng.fr() if i % 5 else 0 for i in range(n)]
    prefix, steps, info = S.prefix_sim(a)
    acc, want = 0, []
    for x in a:
        acc = (acc + x) % R
        want.append(acc)
    assert prefix == want
    sizes = info["sizes"]
    # two additions per entry of a level that has one above it, one per entry of the top level
    assert len(steps) == sum(2 * m for m in sizes[:-1]) + sizes[-1]


def test_prefix_sim_on_points():
    """One small case on points: the simulator's prefix times G is the running sum of the a_i G, degenerate steps included."""
    a = S.prefix_degenerate_scalars(5)
    prefix, _, _ = S.prefix_sim(a)
    acc = None
    for x, s in zip(a, prefix):
        acc = P.g1_add(acc, P.g1_mul(P.G1_GEN, x))
        assert acc == P.g1_mul(P.G1_GEN, s)


FOUR = ("into_identity", "adding_identity", "doubling", "cancelling")


@pytest.mark.parametrize("k", [5, 9, 10, 13])
def test_prefix_degenerate_scalars_coverage(k):
    """What test_gpu_srs_unit's prefix-sum test relies on. Every level with a full chunk meets all four degenerate steps in its
    total pass and in its apply pass. The one chunk at the top has 4 entries at k = 10 and meets all four too; with 2 entries
    (k = 5, 9, 13) it has one step behind its first, which cannot be four things: the three k take a kind each (k = 5: adding the
    identity first, then into the identity; k = 9: doubling; k = 13: cancelling), so the three tops together meet all four."""
    a = S.prefix_degenerate_scalars(k)
    assert len(a) == 1 << k
    prefix, steps, info = S.prefix_sim(a)
    sizes = info["sizes"]
    assert sizes == {5: [32, 2], 9: [512, 32, 2], 10: [1024, 64, 4], 13: [8192, 512, 32, 2]}[k]
    cov = S.prefix_coverage(steps, info)
    top = len(sizes) - 1
    assert set(cov) == {(l, "total") for l in range(top)} | {(l, "apply") for l in range(top + 1)}
    for (level, pas), c in cov.items():
        if level < top:
            assert all(c[kind] >= 1 for kind in FOUR) and c["general"] >= 1, (level, pas, c)
    ctop = cov[(top, "apply")]
    if sizes[-1] == 4:
        assert all(ctop[kind] == 1 for kind in FOUR), ctop
    else:
        want = {"zero_first": ("adding_identity", "into_identity"), "double": ("doubling",), "cancel": ("cancelling",)}[S.TOP_OF_2[k]]
        assert all(ctop[kind] == 1 for kind in want), ctop
    # an apply pass that starts from a carry (not from the identity) doubles and cancels against it
    from_carry = [(l, kind) for l, pas, t, i, first, kind in steps if pas == "apply" and first and t and info["carries"][l][t - 1]]
    for l in range(top):
        if any(info["carries"][l]):
            assert (l, "doubling") in from_carry, l
    assert any(x == 0 for lv in info["totals"] for x in lv)  # a chunk total is the identity
    assert any(c == 0 for l in range(top) for c in info["carries"][l])  # a carry is the identity
    assert [(l, t, lo, hi) for l, t, lo, hi in info["ragged"]] == [(top, 0, 0, sizes[-1])]  # the ragged chunk: the top one
    rows = S.prefix_rows_to_read(steps, info)
    assert len(rows) <= 64 and {0, 15, 16, (1 << k) - 1} <= set(rows)
    assert any(prefix[r] == 0 for r in rows)  # an S_i that is the identity is read


def test_tops_of_two_cover_all_four_kinds():
    kinds = set()
    for k in (5, 9, 13):
        _, steps, info = S.prefix_sim(S.prefix_degenerate_scalars(k))
        top = len(info["sizes"]) - 1
        kinds |= {kind for kind, cnt in S.prefix_coverage(steps, info)[(top, "apply")].items() if cnt}
    assert set(FOUR) <= kinds


def test_oracle_points_of_edge_scalars(oracle):
    """The oracle's g1_mul_many / srs_powers at the scalars the GPU tests lean on: 0 gives the identity as (0, 0), and a trapdoor
    of 0 gives g = [G, identity, ...] and every L_i = 1/n."""
    G = oracle.generator()
    pts = oracle.g1_mul_many(G, zu.ints_to_fr(oracle, [0, 1, R - 1, 1 << 253]))
    assert [zu.point_to_ints(p) for p in pts] == [None, (1, 2), (1, Q - 2), P.g1_mul(P.G1_GEN, 1 << 253)]
    g, gl = zu.test_srs(oracle, 3, 0)
    assert zu.point_to_ints(g[0]) == (1, 2) and not g[1:].any()
    assert all(zu.point_to_ints(p) == P.g1_mul(P.G1_GEN, pow(8, -1, R)) for p in gl)
