"""GPU: the pairing unit — amdzk_g2_setup, amdzk_g2_prepare, amdzk_pairing_products — against tests/pairing_ref.py: GT limb
for limb for m = 1, 2, 3 with identity entries in every position and for batches across the wave boundary and the
lanes-per-block threshold, and for calls of more than one chunk of 16384 Miller lanes (m = 16 and m = 3, values on both
sides of the boundary); is_one on pairs that cancel and pairs that do not; s * G2; refusals that leave the ctx usable."""
import ctypes as C

import numpy as np
import pytest

import pairing_ref as X

pytestmark = pytest.mark.gpu

A1, A2, A3 = 0x9E3779B97F4A7C15F39CC0605CEDC834, 0x2545F4914F6CDD1D, X.R - 5
B1, B2 = 0x1082276BF3A27251F86C6A11D0C18E95, X.R - 2
QS = [X.G2_GEN, X.g2_mul(X.G2_GEN, B1), X.g2_mul(X.G2_GEN, B2)]


def P(k):
    return None if k is None else X.g1_mul(X.G1_GEN, k)


def words(vals, width):
    return np.array(vals, dtype=np.uint64).reshape(-1, width)


@pytest.fixture(scope="module")
def kzg(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.kzg", fromlist=["x"])


@pytest.fixture(scope="module")
def prepared(ctx, kzg):
    qs = [kzg.G2Prepared(ctx, words(X.g2_words(q), 16)) for q in QS]
    yield qs
    for q in qs:
        q.free()


def run(ctx, kzg, prepared, checks):
    """checks: per product a list of m G1 scalars (None = the identity). Returns (is_one, gt rows as lists of ints)."""
    m = len(checks[0])
    g1 = words([X.g1_words(P(k)) for row in checks for k in row], 8)
    one, gt = kzg.pairing_products(ctx, prepared[:m], g1)
    return [bool(v) for v in one], [[int(v) for v in row] for row in gt]


def want(row):
    return X.pairing_product([(P(k), QS[j]) for j, k in enumerate(row)])


@pytest.mark.parametrize("checks", [
    [[A1], [None]],                                        # m = 1, and the lone identity
    [[A1, None], [None, A2]],                              # m = 2: identity last / first
    [[None, A1, A2], [A1, None, A2], [A1, A2, None]],      # m = 3: identity first / middle / last
    [[1, 1]],                                              # n = 1
], ids=["m1", "m2", "m3", "n1"])
def test_gt_equals_the_reference_limb_for_limb(ctx, kzg, prepared, checks):
    one, gt = run(ctx, kzg, prepared, checks)
    for row, o, g in zip(checks, one, gt):
        w = want(row)
        assert g == X.gt_words(w), row
        assert o == (w == X.F12_ONE)


@pytest.mark.parametrize("n", [65, 2049])
def test_batches_across_the_wave_boundary_and_the_lanes_per_block_threshold(ctx, kzg, prepared, n):
    """Four distinct inputs; the distinct answers sit at 0, n - 2 and n - 1 (63 and 64 for n = 65: the wave boundary). 2049
    products are more than one lane per SIMD on every part, so blocks run several active lanes and the last block is partial."""
    ks = [A1] + [A2] * (n - 3) + [A3, 1]
    one, gt = run(ctx, kzg, prepared, [[k] for k in ks])
    ref = {k: X.gt_words(want([k])) for k in set(ks)}
    assert len({tuple(v) for v in ref.values()}) == 4
    for i, k in enumerate(ks):
        assert gt[i] == ref[k], i
    assert not any(one)


def _row16(a, b, c):
    """m = 16: the identity everywhere but at positions 0, 7 and 15."""
    row = [None] * 16
    row[0], row[7], row[15] = a, b, c
    return tuple(row)


# (m, n, the common row, {index: another row}, the index of the row that cancels). PAIRING_CHUNK_LANES = 16384 Miller lanes
# go into one pair of launches, so a call is cut into chunks of 16384 / m checks.
CHUNKED = {
    # 16400 lanes, chunks of 1024 + 1 checks; handle j is prepared point j % 3, so positions 0 and 15 pair with the same point
    # and row 1024, the first of the second chunk, is e(5 P, Q) e(-5 P, Q) = 1 (A3 = r - 5)
    "m16": (16, 1025, _row16(A1, A2, A3), {0: _row16(1, A2, A3), 517: _row16(A1, A2, 1), 1023: _row16(A1, 1, A3), 1024: _row16(5, None, A3)}, 1024),
    # chunks of 5461 + 1 checks: 16384 is no multiple of 3; row 5461 is e(2 P, Q) e(P, -2 Q) = 1 (B2 = r - 2)
    "m3": (3, 5462, (A1, A2, A3), {0: (1, A2, A3), 5460: (A1, 1, A3), 5461: (2, None, 1)}, 5461),
}


@pytest.mark.parametrize("want_gt", [True, False], ids=["gt", "is_one_only"])
@pytest.mark.parametrize("shape", sorted(CHUNKED))
def test_calls_of_more_than_one_chunk(ctx, kzg, prepared, shape, want_gt):
    """Values checked on both sides of a chunk boundary: the second chunk's G1 rows, GT rows and is_one bytes start where the
    first chunk's end, its lanes pick their lines by (lane % m) counted from the chunk's first lane, and its launches reuse
    the two register slabs. GT limb for limb for every row; is_one for the row that cancels, the first of the second chunk."""
    m, n, common, special, cancels = CHUNKED[shape]
    rows = [special.get(i, common) for i in range(n)]
    distinct = sorted(set(rows), key=str)
    ref = {row: X.pairing_product([(P(k), QS[j % 3]) for j, k in enumerate(row)]) for row in distinct}
    assert len(set(ref.values())) == len(distinct) == len(special) + 1 and ref[rows[cancels]] == X.F12_ONE
    point = {k: np.array(X.g1_words(P(k)), dtype=np.uint64) for row in distinct for k in row}
    g1 = np.stack([point[k] for row in rows for k in row])
    one, gt = kzg.pairing_products(ctx, [prepared[j % 3] for j in range(m)], g1, want_gt=want_gt)
    assert [i for i in range(n) if one[i]] == [cancels]
    if not want_gt:
        assert gt is None
        return
    expect = {row: np.array(X.gt_words(f), dtype=np.uint64) for row, f in ref.items()}
    wrong = [i for i in range(n) if not np.array_equal(gt[i], expect[rows[i]])]
    assert not wrong, "GT differs from the reference in rows %s ... (%d rows)" % (wrong[:8], len(wrong))


@pytest.mark.parametrize("a", [1, X.R - 1])
def test_is_one_on_pairs_that_cancel_and_pairs_that_do_not(ctx, kzg, a):
    """e(aP, Q) e(-P, aQ) = 1; with a + 1 in the first place it is e(P, Q) != 1."""
    qs = [kzg.G2Prepared(ctx, words(X.g2_words(q), 16)) for q in (X.G2_GEN, X.g2_mul(X.G2_GEN, a))]
    try:
        g1 = words(X.g1_words(P(a)) + X.g1_words(P(X.R - 1)) + X.g1_words(P((a + 1) % X.R)) + X.g1_words(P(X.R - 1)), 8)
        one, gt = kzg.pairing_products(ctx, qs, g1)
        assert list(one) == [True, False]
        assert [int(v) for v in gt[0]] == X.gt_words(X.F12_ONE)
    finally:
        for q in qs:
            q.free()


def test_all_identity_g1_entries_give_one(ctx, kzg, prepared):
    one, gt = kzg.pairing_products(ctx, prepared[:2], np.zeros((4, 8), np.uint64))
    assert list(one) == [True, True] and [int(v) for v in gt[1]] == X.gt_words(X.F12_ONE)
    one, gt = kzg.pairing_products(ctx, prepared[:2], np.zeros((2, 8), np.uint64), want_gt=False)
    assert list(one) == [True] and gt is None


def test_g2_setup_is_the_references_scalar_multiple(ctx, kzg):
    import zkutil as zu
    for s in (1, 2, X.R - 1, 0x2B1C0D9E8F7A6B5C4D3E2F1A0B9C8D7E6F5A4B3C2D1E0F9A8B7C6D5E4F3A2B1 % X.R):
        g2, s_g2 = kzg.g2_setup(ctx, zu.fr_from_int(s))
        assert [int(v) for v in g2] == X.g2_words(X.G2_GEN)
        assert [int(v) for v in s_g2] == X.g2_words(X.g2_mul(X.G2_GEN, s)), hex(s)


def test_refusals_leave_the_ctx_usable(ctx, pkg, kzg, prepared):
    L = ctx.L
    good = words(X.g2_words(X.G2_GEN), 16).reshape(16)
    g1 = words(X.g1_words(P(1)) + X.g1_words(P(X.R - 1)), 8)
    handles = (C.c_void_p * 2)(prepared[0].h, prepared[0].h)

    def still_works():
        one = np.zeros(1, np.uint8)
        assert L.amdzk_pairing_products(ctx.h, handles, 2, g1.ctypes.data, 1, one.ctypes.data, None) == 0 and one[0] == 1  # e(P, Q) e(-P, Q)

    def refused(rc, prefix):
        assert rc == -2 and L.amdzk_last_error(ctx.h).decode().startswith(prefix), (rc, L.amdzk_last_error(ctx.h))
        still_works()

    out = C.c_void_p()
    off_twist = good.copy()
    off_twist[8:12] = good[0:4]                      # y.c0 := x.c0
    big = good.copy()
    big[4:8] = np.array([(X.P >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)  # x.c1 := q itself
    refused(L.amdzk_g2_prepare(ctx.h, None, C.byref(out)), "g2_prepare:")
    refused(L.amdzk_g2_prepare(ctx.h, good.ctypes.data, None), "g2_prepare:")
    for bad in (big, off_twist, np.zeros(16, np.uint64)):
        refused(L.amdzk_g2_prepare(ctx.h, bad.ctypes.data, C.byref(out)), "g2_prepare:")
        assert not out.value
    many = (C.c_void_p * 17)(*[prepared[0].h] * 17)
    g17 = np.zeros((17, 8), np.uint64)
    one = np.zeros(1, np.uint8)
    for rc in (L.amdzk_pairing_products(ctx.h, None, 2, g1.ctypes.data, 1, one.ctypes.data, None),
               L.amdzk_pairing_products(ctx.h, handles, 2, None, 1, one.ctypes.data, None),
               L.amdzk_pairing_products(ctx.h, handles, 0, g1.ctypes.data, 1, one.ctypes.data, None),
               L.amdzk_pairing_products(ctx.h, handles, 2, g1.ctypes.data, 0, one.ctypes.data, None),
               L.amdzk_pairing_products(ctx.h, (C.c_void_p * 2)(prepared[0].h, None), 2, g1.ctypes.data, 1, one.ctypes.data, None),
               L.amdzk_pairing_products(ctx.h, many, 17, g17.ctypes.data, 1, one.ctypes.data, None)):
        refused(rc, "pairing_products:")
    assert L.amdzk_pairing_products(ctx.h, many, 16, g17.ctypes.data, 1, one.ctypes.data, None) == 0 and one[0] == 1  # the cap itself runs
    with pytest.raises(pkg.ffi.AmdzkError, match="g2_prepare:"):
        kzg.G2Prepared(ctx, np.zeros(16, np.uint64))
