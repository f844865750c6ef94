"""GPU: the SRS unit (csrc/srs.hip) at edge encodings, trapdoors and degenerate points — the G1 codec behind ParamsKZG::{write,
read}, ParamsKZG::setup, g_to_lagrange / downsize and the prefix-sum basis, each against Python integers and the oracle.
Every comparison is exact (bytes, words, affine integers). The inputs are points a_i G with chosen a_i, and the claims that
they take the kernels through doublings, cancellations and identities at the threads named are asserted on scalars in
tests/test_srs_unit_ref.py (srs_unit_ref's simulators); the tests here repeat the assertion they depend on before they run.
This is also where bn254.cuh's radix-2^32 point formulas (x_add, x_add_affine, x_dbl, x_dbl_affine, x_to_affine,
fq_sqrt_checked, g1_y_from_x, is_canonical) run as device code: the other tests of those functions are host builds."""
import ctypes as C

import numpy as np
import pytest

import circuits
import srs_unit_ref as S
import zkutil as zu

import plonk_ref as PR  # srs_unit_ref put oracle/ on the path
import pyref as P

pytestmark = pytest.mark.gpu
Q, R = S.Q, S.R
TAU = 0x1234567890ABCDEF1234567
CODEC_K = 9  # 512 points: two blocks of g1_compress_kernel per basis, four of g1_decompress_kernel over both
_cache = {}


def points_of(oracle, scalars):
    """a_i G, (len, 8) uint64; a_i = 0 gives (0, 0)."""
    return oracle.g1_mul_many(oracle.generator(), zu.ints_to_fr(oracle, [a % R for a in scalars]))


def random_points(oracle, n, seed):
    return oracle.g1_mul_many(oracle.generator(), zu.random_fr(n, seed=seed))


def honest(oracle, k):
    if ("srs", k) not in _cache:
        _cache[("srs", k)] = zu.test_srs(oracle, k, TAU)
    return _cache[("srs", k)]


def blob_of(k, g_enc, gl_enc, tail=bytes(128)):
    return k.to_bytes(4, "little") + b"".join(g_enc) + b"".join(gl_enc) + tail


def point_words(kind, pt):
    return zu.point_from_ints(pt if kind == "point" else None)


# ------------------------------------------------------------------------------------------------ compression
def codec_bases(oracle):
    """Two bases of 512 points: random multiples of G with the named points among them — the identity at 0, 255, 256 (both
    sides of the block boundary) and 511, the edge points of srs_unit_ref behind index 1 in g and behind 257 in g_lagrange."""
    if "codec" not in _cache:
        n = 1 << CODEC_K
        edge = [zu.point_from_ints(p) for _, p in S.edge_points()]
        out = []
        for seed, at in ((71, 1), (72, 257)):
            b = random_points(oracle, n, seed)
            for i, e in enumerate(edge):
                b[at + i] = e
            b[[0, 255, 256, n - 1]] = 0
            out.append(b)
        _cache["codec"] = tuple(out)
    return _cache["codec"]


def test_compress_every_point(ctx, pkg, oracle):
    n = 1 << CODEC_K
    g, gl = codec_bases(oracle)
    ys = [zu.point_to_ints(p)[1] & 1 for p in g if p.any()]
    assert 0 < sum(ys) < len(ys)  # odd and even y
    params = pkg.kzg.ParamsKZG(ctx, CODEC_K, g=g, g_lagrange=gl)
    g2, s_g2 = bytes(range(100, 164)), bytes(range(7, 71))
    blob = params.write(g2, s_g2)
    assert len(blob) == 4 + 64 * n + 128 and blob[:4] == CODEC_K.to_bytes(4, "little") and blob[4 + 64 * n:] == g2 + s_g2
    for b, base in enumerate((g, gl)):
        for i in range(n):
            o = 4 + 32 * (b * n + i)
            assert blob[o:o + 32] == PR.g1_compress(zu.point_to_ints(base[i])), (b, i)
    # read(write(p)) = p for every point, word for word
    back, g2b, sg2b = pkg.kzg.ParamsKZG.read(ctx, blob)
    assert (g2b, sg2b) == (g2, s_g2)
    assert np.array_equal(back.get_g(), g) and np.array_equal(back.get_g_lagrange(), gl)
    assert back.write(g2, s_g2) == blob
    back.free(); params.free()


# ------------------------------------------------------------------------------------------------ decompression
# where a class is put: once in the first block of a basis, once in a later one
FIRST, LATER = 3, 256 + 64


def valid_encodings(oracle):
    """512 + 512 encodings ParamsKZG::read accepts: random points (other ones in either basis), and every accepted class at
    FIRST.. and at LATER.. of both bases."""
    if "valid" not in _cache:
        n = 1 << CODEC_K
        enc = []
        for seed in (81, 82):
            e = [PR.g1_compress(zu.point_to_ints(p)) for p in random_points(oracle, n, seed)]
            for at in (FIRST, LATER):
                for i, (_, b) in enumerate(S.ACCEPTED_ENCODINGS):
                    e[at + i] = b
            enc.append(e)
        _cache["valid"] = tuple(enc)
    return _cache["valid"]


def decoded(encodings):
    out = np.zeros((len(encodings), 8), np.uint64)
    for i, b in enumerate(encodings):
        kind, pt = S.g1_decompress(b)
        assert kind != "refused"
        out[i] = point_words(kind, pt)
    return out


def test_decompress_accepted_classes(ctx, pkg, oracle):
    g_enc, gl_enc = valid_encodings(oracle)
    params, _, _ = pkg.kzg.ParamsKZG.read(ctx, blob_of(CODEC_K, g_enc, gl_enc))
    for name, enc, got in (("g", g_enc, params.get_g()), ("g_lagrange", gl_enc, params.get_g_lagrange())):
        assert np.array_equal(got, decoded(enc)), name
        for i, b in enumerate(enc):  # the canonical y's parity is the sign bit; the identity is (0, 0)
            pt = zu.point_to_ints(got[i])
            if any(b):
                assert pt is not None and pt[0] == int.from_bytes(b, "little") & ((1 << 255) - 1) and pt[1] & 1 == b[31] >> 7, (name, i)
                assert P.g1_on_curve(pt), (name, i)
            else:
                assert pt is None and i in (FIRST, LATER), (name, i)
    assert params.write() == blob_of(CODEC_K, g_enc, gl_enc)
    params.free()


@pytest.mark.parametrize("name,bad", S.REFUSED_ENCODINGS, ids=[n for n, _ in S.REFUSED_ENCODINGS])
def test_decompress_refuses(ctx, pkg, oracle, name, bad):
    """One refused encoding alone in an otherwise valid file, in the first and in a later block of either basis: refused as an
    invalid point encoding, no handle comes back, and the ctx reads the valid file next."""
    assert S.g1_decompress(bad)[0] == "refused"
    g_enc, gl_enc = valid_encodings(oracle)
    good = blob_of(CODEC_K, g_enc, gl_enc)
    want_g = decoded(g_enc[:4])
    for basis in (0, 1):
        for at in (FIRST + 9, LATER + 9, (1 << CODEC_K) - 1):
            enc = [list(g_enc), list(gl_enc)]
            enc[basis][at] = bad
            blob = blob_of(CODEC_K, *enc)
            h = C.c_void_p()
            raw = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
            rc = ctx.L.amdzk_srs_read(ctx.h, raw, len(blob), C.byref(h), None, None)
            assert rc == -2 and not h.value, (basis, at, rc)
            assert "invalid point encoding" in ctx.L.amdzk_last_error(ctx.h).decode(), (basis, at)
            with pytest.raises(pkg.AmdzkError, match="invalid point encoding"):
                pkg.kzg.ParamsKZG.read(ctx, blob)
            ok, _, _ = pkg.kzg.ParamsKZG.read(ctx, good)
            assert np.array_equal(ok.get_g()[:4], want_g), (basis, at)
            ok.free()


# ------------------------------------------------------------------------------------------------ setup
def trapdoors(k):
    """0: g = [G, identity, ...], every L_i = 1/n. 2^253: one bit, the top one of a scalar below r. r - 2: near r. The primitive
    2^(k+1)-th root of unity: s^n = -1, the farthest from the refused s^n = 1."""
    return [("zero", 0), ("two", 2), ("top_bit", 1 << 253), ("r_minus_2", R - 2), ("root_2n", P.omega(k + 1))]


# powers_kernel gives a thread 64 elements and a block 64 threads: k = 0, 1, 5 ragged; 6 one full thread; 7 two threads; 12 exactly
# one block; 13 two blocks. fixed_base_mul_kernel and the launches around batch_invert have 256 threads: k = 9 is two blocks of them.
SETUP_CASES = [(k, name) for k in (0, 1, 5, 6, 7, 9) for name, _ in trapdoors(0)] + [(k, name) for k in (12, 13) for name in ("r_minus_2", "top_bit")]


@pytest.mark.parametrize("k,name", SETUP_CASES, ids=["k%d_%s" % c for c in SETUP_CASES])
def test_setup_matches_oracle(ctx, pkg, oracle, k, name):
    s = dict(trapdoors(k))[name]
    n = 1 << k
    if name == "root_2n":
        assert pow(s, n, R) == R - 1
    params = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(s), want_host_copy=True)
    g, gl = zu.test_srs(oracle, k, s)
    assert np.array_equal(params._g, g), "g"
    assert np.array_equal(params._gl, gl), "g_lagrange"
    if name == "zero":
        assert zu.point_to_ints(g[0]) == (1, 2) and not g[1:].any()
    assert np.array_equal(params.get_g(), g) and np.array_equal(params.get_g_lagrange(), gl)  # what stays on the device
    params.free()


def setup_rc(ctx, k, words):
    s = np.array(words, dtype=np.uint64)
    h = C.c_void_p()
    rc = ctx.L.amdzk_srs_setup(ctx.h, k, s.ctypes.data_as(C.c_void_p), C.byref(h), None, None)
    return rc, h, ctx.L.amdzk_last_error(ctx.h).decode()


def test_setup_refuses_what_has_no_meaning(ctx, pkg, oracle):
    """s >= r as words, and s^n = 1 (s a point of the domain: the Lagrange basis would come out all identities). AMDZK_E_INVALID
    with the cause named, no handle, and the next setup on the ctx is right."""
    def then_usable(k):
        p = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(TAU), want_host_copy=True)
        g, gl = honest(oracle, k)
        assert np.array_equal(p._g, g) and np.array_equal(p._gl, gl)
        p.free()

    w5 = P.omega(5)
    in_domain = {0: [("one", 1)], 5: [("one", 1), ("r_minus_1", R - 1), ("omega^3", pow(w5, 3, R))]}
    for k in (0, 5):
        for name, words in (("r", zu.limbs(R)), ("r_plus_1", zu.limbs(R + 1)), ("all_ones", [2 ** 64 - 1] * 4)):
            rc, h, msg = setup_rc(ctx, k, words)
            assert rc == -2 and not h.value and "s >= r" in msg, (k, name, rc, msg)
            then_usable(k)
        for name, s in in_domain[k]:
            assert pow(s, 1 << k, R) == 1
            rc, h, msg = setup_rc(ctx, k, zu.fr_from_int(s))
            assert rc == -2 and not h.value and "s^n = 1" in msg, (k, name, rc, msg)
            with pytest.raises(pkg.AmdzkError, match="s\\^n = 1"):
                pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(s))
            then_usable(k)
    rc, h, msg = setup_rc(ctx, 5, zu.limbs(R - 1))  # the largest words that are a field element: accepted
    assert rc == 0 and h.value
    ctx.L.amdzk_srs_free(ctx.h, h)


# ------------------------------------------------------------------------------------------------ g_to_lagrange, k = 10
def test_g_to_lagrange_degenerate_butterflies_in_every_block(ctx, pkg, oracle):
    """The input of srs_unit_ref.ecfft_degenerate_input: in round 1, threads 256.. (blocks 1 and up, twiddle index pos << 1)
    add equal points, opposite points and identities, at least 40 butterflies of each kind, and rounds 2 and 3 meet the
    identities that makes. Reference: ifft(a) G."""
    k = 10
    a = S.ecfft_degenerate_input(k)
    _, out, kinds = S.ecfft_sim(a, k)
    c1 = S.butterfly_counts(kinds[1], first_thread=256)
    assert all(c1[kind] >= 40 for kind in S.BUTTERFLY_KINDS), c1
    for s in (2, 3):
        c = S.butterfly_counts(kinds[s], first_thread=256)
        assert all(c[kind] >= 1 for kind in ("u0", "v0", "u0v0")), (s, c)
    got = pkg.arithmetic.g_to_lagrange(ctx, points_of(oracle, a), k)
    assert np.array_equal(got, points_of(oracle, out))


def test_g_to_lagrange_all_equal_and_all_identity(ctx, pkg, oracle):
    """Every butterfly of every round adds two equal points (or two identities): one output is finite, c G at index 0, the
    other 1023 reach x_to_affine as the identity. And the all-identity input."""
    k, c = 10, 0x1F2E3D4C5B6A79880123456789ABCDEF
    n = 1 << k
    _, out, kinds = S.ecfft_sim([c] * n, k)
    assert out == [c] + [0] * (n - 1) and all(set(row) <= {"eq", "u0v0"} for row in kinds)
    p = points_of(oracle, [c])
    got = pkg.arithmetic.g_to_lagrange(ctx, np.tile(p, (n, 1)), k)
    assert np.array_equal(got[0], p[0]) and not got[1:].any()
    assert not pkg.arithmetic.g_to_lagrange(ctx, np.zeros((n, 8), np.uint64), k).any()


# ------------------------------------------------------------------------------------------------ downsize
def test_downsize_to_the_same_k_to_0_and_without_g(ctx, pkg, oracle):
    k = 6
    g, gl = honest(oracle, k)
    params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
    params.downsize(k)  # new_k = k: the FFT of the whole g gives back g_lagrange
    assert params.k == k and np.array_equal(params.get_g(), g) and np.array_equal(params.get_g_lagrange(), gl)
    params.downsize(0)  # n = 1: L_0 = 1, g_lagrange = [g[0]]
    assert params.n == 1 and np.array_equal(params.get_g(), g[:1]) and np.array_equal(params.get_g_lagrange(), g[:1])
    params.free()
    only_gl = pkg.kzg.ParamsKZG(ctx, k, g_lagrange=gl)
    h = C.c_void_p()
    rc = ctx.L.amdzk_srs_downsize(ctx.h, only_gl.h, 3, C.byref(h))
    assert rc == -2 and not h.value and "no monomial basis" in ctx.L.amdzk_last_error(ctx.h).decode()
    assert np.array_equal(only_gl.get_g_lagrange(), gl)  # untouched, and the ctx goes on
    only_gl.free()


# ------------------------------------------------------------------------------------------------ prefix sums
def key_with_permutation(ctx, plonk, oracle, params, k):
    c = circuits.square_circuit(plonk, k)  # three equality-enabled columns: keygen builds the prefix-sum basis
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    return plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(5))


FOUR = ("into_identity", "adding_identity", "doubling", "cancelling")


@pytest.mark.parametrize("k", [5, 9, 10, 13])
def test_prefix_sums_over_a_chosen_basis(ctx, pkg, oracle, k):
    """g_lagrange[i] = a_i G with the a_i of srs_unit_ref.prefix_degenerate_scalars: every level of the scan (32 -> 2, 512 -> 32
    -> 2, 1024 -> 64 -> 4, 8192 -> 512 -> 32 -> 2) doubles, cancels, adds the identity and adds into the identity, in the chunk
    totals and on the way down, a chunk total and a carry are the identity, and the top chunk is ragged. S is read back through
    MSMs over the prefix basis: unit vectors at the chunk edges of every level and at the degenerate steps, and one random
    column, which weighs every S_i."""
    n = 1 << k
    a = S.prefix_degenerate_scalars(k)
    prefix, steps, info = S.prefix_sim(a)
    cov = S.prefix_coverage(steps, info)
    top = len(info["sizes"]) - 1
    assert all(c[kind] >= 1 for (level, _), c in cov.items() if level < top for kind in FOUR)
    assert info["ragged"] == [(top, 0, 0, info["sizes"][-1])]
    rows = S.prefix_rows_to_read(steps, info)
    plonk = __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])
    A, PFX = pkg.arithmetic, pkg.kzg.BASIS_G_LAGRANGE_PREFIX
    g = oracle.srs_powers(zu.fr_from_int(TAU), n)  # an honest g
    params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=points_of(oracle, a))
    pk = key_with_permutation(ctx, plonk, oracle, params, k)
    one = zu.fr_from_int(1)
    units = []
    for r in rows:
        e = np.zeros((n, 4), np.uint64)
        e[r] = one
        units.append(e)
    got = zu.jac_to_affine_host(oracle, A.best_multiexp_batch(ctx, params.h, PFX, units)).reshape(-1, 8)
    want = points_of(oracle, [prefix[r] for r in rows])
    for j, r in enumerate(rows):
        assert np.array_equal(got[j], want[j]), ("S_%d" % r, prefix[r] == 0)
    d = zu.fr_array_to_ints(zu.random_fr(n, seed=900 + k))
    got = zu.jac_to_affine_host(oracle, A.best_multiexp(ctx, params.h, PFX, zu.fr_array_from_ints(d)))
    assert np.array_equal(got, points_of(oracle, [sum(x * s for x, s in zip(d, prefix)) % R])[0])
    pk.free(); params.free()
