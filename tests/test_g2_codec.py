"""CPU: amdzk_g2_compress / amdzk_g2_decompress / amdzk_g2_check (csrc/g2codec.hpp) through ctypes, with no device, against a
Python-integer encoder written from the format's description: halo2curves 0.3.1's G2Compressed is x.c0 | x.c1, canonical
little-endian, bit 7 of byte 63 = the parity of the canonical y.c0, 64 zero bytes = the identity (the convention is recalled,
not pinned by a fixture: DESIGN.md §4). Points come from tests/pairing_ref.py."""
import random

import numpy as np
import pytest

import pairing_ref as X

Q, R = X.P, X.R


# ------------------------------------------------------------------ the reference, Python integers only
def ref_encode(pt):
    if pt is None:
        return bytes(64)
    (x0, x1), (y0, _y1) = pt
    b = bytearray(x0.to_bytes(32, "little") + x1.to_bytes(32, "little"))
    b[63] |= (y0 & 1) << 7
    return bytes(b)


def twist_rhs(x):
    return X.f2_add(X.f2_mul(X.f2_mul(x, x), x), X.B2)


def is_residue(a):
    return a == (0, 0) or X.f2_pow(a, (Q * Q - 1) // 2) == (1, 0)


def words(pt):
    return np.array(X.g2_words(pt), dtype=np.uint64)


def raw_words(x0, x1, y0, y1):
    """16 words from four 256-bit integers taken as they are (no reduction, no Montgomery form): for coordinates >= q."""
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in (x0, x1, y0, y1) for i in range(4)], dtype=np.uint64)


def small_x_candidates():
    """x = (a, b) for small a, b in a fixed order, each with whether x^3 + 3/xi is a square (Euler's criterion)."""
    for a in range(1, 40):
        for b in range(0, 3):
            yield (a, b), is_residue(twist_rhs((a, b)))


@pytest.fixture(scope="module")
def kzg(pkg):
    return pkg.kzg


@pytest.fixture(scope="module")
def g2_points():
    rng = random.Random(0x62636F646563)
    pts = [X.G2_GEN, X.g2_neg(X.G2_GEN)] + [X.g2_mul(X.G2_GEN, rng.randrange(1, R)) for _ in range(50)]
    assert {p[1][0] & 1 for p in pts[2:]} == {0, 1}, "both parities of y.c0 must occur among the random points"
    return pts


@pytest.fixture(scope="module")
def off_group_points(kzg):
    """Ten points of the twist from small residue x values. The twist's cofactor is about 2^254, so they lie outside G2:
    Python decides ([r]Q != O), and none is kept for which it says otherwise."""
    out = []
    for x, res in small_x_candidates():
        if not res:
            continue
        q = X.g2_from_words(kzg.g2_from_bytes(ref_encode((x, (0, 0)))))
        assert q[0] == x and X.g2_on_curve(q)
        if X.g2_mul(q, R) is not None:
            out.append(q)
        if len(out) == 10:
            break
    assert len(out) >= 8
    return out


# ------------------------------------------------------------------ compress
def test_generator_encodes_as_its_x_with_no_flag(kzg):
    assert X.G2_GEN[1][0] & 1 == 0
    b = kzg.g2_to_bytes(words(X.G2_GEN))
    assert b == X.G2_GEN[0][0].to_bytes(32, "little") + X.G2_GEN[0][1].to_bytes(32, "little") == ref_encode(X.G2_GEN)
    n = kzg.g2_to_bytes(words(X.g2_neg(X.G2_GEN)))
    assert n[:63] == b[:63] and n[63] == b[63] | 0x80 and n == ref_encode(X.g2_neg(X.G2_GEN))


def test_compress_matches_the_reference_byte_for_byte(kzg, g2_points):
    for p in g2_points:
        assert kzg.g2_to_bytes(words(p)) == ref_encode(p)


def test_identity_is_64_zero_bytes_both_ways(kzg):
    assert kzg.g2_to_bytes(np.zeros(16, np.uint64)) == bytes(64)
    assert not kzg.g2_from_bytes(bytes(64)).any()


# ------------------------------------------------------------------ decompress
def test_decompress_inverts_compress_and_the_sign_bit_negates(kzg, g2_points):
    for p in g2_points:
        b = ref_encode(p)
        assert np.array_equal(kzg.g2_from_bytes(b), words(p))
        flipped = b[:63] + bytes([b[63] ^ 0x80])
        assert np.array_equal(kzg.g2_from_bytes(flipped), words(X.g2_neg(p)))


def refused(kzg, pkg, fn, arg, prefix):
    with pytest.raises(pkg.AmdzkError) as e:
        fn(arg)
    assert e.value.code == -2 and prefix in str(e.value), str(e.value)
    return str(e.value)


def test_decompress_refuses_x_not_below_q(kzg, pkg):
    gx0, gx1 = X.G2_GEN[0]
    for b in (Q.to_bytes(32, "little") + gx1.to_bytes(32, "little"),      # x.c0 = q
              gx0.to_bytes(32, "little") + Q.to_bytes(32, "little"),      # x.c1 = q
              (Q + 5).to_bytes(32, "little") + gx1.to_bytes(32, "little"),
              gx0.to_bytes(32, "little") + ((1 << 256) - 1 - (1 << 255)).to_bytes(32, "little")):
        refused(kzg, pkg, kzg.g2_from_bytes, b, "g2_decompress: x is not below the modulus")
    b = bytearray(ref_encode(X.G2_GEN))
    b[63] |= 0x40  # bit 6 is always clear in a valid encoding: x.c1 < q < 2^254
    refused(kzg, pkg, kzg.g2_from_bytes, bytes(b), "g2_decompress: x is not below the modulus")


def test_decompress_refuses_zero_x_with_the_sign_bit(kzg, pkg):
    refused(kzg, pkg, kzg.g2_from_bytes, bytes(63) + b"\x80", "g2_decompress: x = 0")


def test_decompress_refuses_non_residues(kzg, pkg):
    bad = [x for x, res in small_x_candidates() if not res][:20]
    assert len(bad) == 20
    for x in bad:
        for sign in (0, 0x80):
            b = bytearray(ref_encode((x, (0, 0))))
            b[63] |= sign
            refused(kzg, pkg, kzg.g2_from_bytes, bytes(b), "g2_decompress: x^3 + 3/xi is not a square")


def test_decompress_and_compress_refuse_a_wrong_length_or_null(kzg, pkg):
    refused(kzg, pkg, kzg.g2_from_bytes, bytes(63), "g2_decompress:")
    L = pkg.lib()
    import ctypes as C
    msg = C.create_string_buffer(64)
    assert L.amdzk_g2_compress(None, None, msg, 64) == -2 and msg.value.startswith(b"g2_compress:")
    assert L.amdzk_g2_decompress(None, None, msg, 64) == -2 and msg.value.startswith(b"g2_decompress:")
    assert L.amdzk_g2_decompress(None, None, None, 0) == -2
    st = C.c_int(0)
    assert L.amdzk_g2_check(None, C.byref(st)) == -2


def test_compress_refuses_what_g2_prepare_refuses_except_the_identity(kzg, pkg):
    (x0, x1), (y0, y1) = X.G2_GEN
    refused(kzg, pkg, kzg.g2_to_bytes, raw_words(Q, x1, y0, y1), "g2_compress: a coordinate is not below the modulus")
    refused(kzg, pkg, kzg.g2_to_bytes, raw_words(x0, x1, y0, Q + 1), "g2_compress: a coordinate is not below the modulus")
    refused(kzg, pkg, kzg.g2_to_bytes, words(((x0, x1), ((y0 + 1) % Q, y1))), "g2_compress: the point is not on the twist")


# ------------------------------------------------------------------ membership
def test_check_accepts_points_of_g2(kzg, g2_points):
    for p in g2_points:
        assert kzg.g2_check(words(p)) == kzg.G2_IN_GROUP == 0


def test_check_statuses_of_bad_points(kzg):
    (x0, x1), (y0, y1) = X.G2_GEN
    assert kzg.g2_check(np.zeros(16, np.uint64)) == kzg.G2_IDENTITY == 3
    for w in (raw_words(Q, x1, y0, y1), raw_words(x0, Q, y0, y1), raw_words(x0, x1, Q, y1), raw_words(x0, x1, y0, (1 << 256) - 1)):
        assert kzg.g2_check(w) == kzg.G2_COORD_TOO_LARGE == 1
    assert kzg.g2_check(words(((x0, x1), ((y0 + 1) % Q, y1)))) == kzg.G2_OFF_TWIST == 2
    assert kzg.g2_check(words(((x0, x1), (y0, (y1 + 1) % Q)))) == 2


def test_check_rejects_twist_points_outside_the_subgroup(kzg, off_group_points):
    for q in off_group_points:
        assert X.g2_on_curve(q) and X.g2_mul(q, R) is not None
        assert kzg.g2_check(words(q)) == kzg.G2_OUTSIDE_SUBGROUP == 4
        # such a point still has an encoding: the codec answers for the twist, g2_check for the subgroup
        assert np.array_equal(kzg.g2_from_bytes(kzg.g2_to_bytes(words(q))), words(q))
