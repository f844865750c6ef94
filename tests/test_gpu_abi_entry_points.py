"""GPU parity of C ABI entry points that bench.py and a fork call but no other test does: the representation changes on
resident data (amdzk_fr_from_raw_dev / amdzk_fr_to_repr_dev — bench.py converts every witness through the first, on the
grid-stride path), the host-column batch transform (amdzk_ntt_fr_batch) and the MSM over resident columns that are not
packed (amdzk_msm_g1_dev with col_stride > len). Exact arithmetic: every comparison is equality with the oracle."""
import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu

T232 = (zu.R >> 232 << 232) - 1  # T * 2^232 - 1, T = r >> 232: the largest value below r whose low 232 bits are all ones
EDGES = [0, 1, zu.R - 1, 1 << 253, T232]


def raw_words(xs):
    """Canonical integers below r as (len, 4) uint64 little-endian words (what Fr::from_raw takes)."""
    return np.array([zu.limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


def raw_column(n, seed):
    """n canonical values: the edge values first (as far as n reaches), then 253-bit random words (all below r)."""
    a = zu.random_fr(n, seed) if n else np.zeros((0, 4), np.uint64)
    m = min(n, len(EDGES))
    a[:m] = raw_words(EDGES[:m])
    if n > 300:  # and the edges again across the block boundary at 256 and at the very end
        a[254:254 + len(EDGES)] = raw_words(EDGES)
        a[n - len(EDGES):] = raw_words(EDGES)
    return a


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, (1 << 20) + 3])
def test_fr_from_raw_and_to_repr_on_resident_data(ctx, pkg, oracle, n):
    """n = 2^20 + 3 is more than 4096 blocks of 256: the kernel's grid-stride loop, the path the benchmark's witness
    upload takes. from_raw equals the oracle's (and x * 2^256 mod r in Python integers where that is cheap), to_repr of
    it is x again, and to_repr alone equals x * 2^-256 mod r; the elements behind the n-th stay untouched."""
    ar = pkg.arithmetic
    raw = raw_column(n, seed=4000 + n)
    guard = zu.random_fr(2, seed=9)
    buf = ctx.alloc((n + 2) * 32).upload(np.concatenate([raw, guard]))
    ar.fr_from_raw_dev(ctx, buf, n)
    mont = buf.download((n + 2, 4))
    assert np.array_equal(mont[n:], guard)
    assert np.array_equal(mont[:n], oracle.fr_from_raw(raw) if n else raw)
    some = list(range(min(n, 300))) + list(range(max(0, n - 8), n))
    assert [zu.from_limbs(mont[i]) for i in some] == [zu.from_limbs(raw[i]) * zu.MONT % zu.R for i in some]
    ar.fr_to_repr_dev(ctx, buf, n)
    back = buf.download((n + 2, 4))
    assert np.array_equal(back[:n], raw) and np.array_equal(back[n:], guard)
    # to_repr on its own: the words read as Montgomery form
    ar.fr_to_repr_dev(ctx, buf, n)
    canon = buf.download((n + 2, 4))
    assert np.array_equal(canon[:n], oracle.fr_to_raw(raw) if n else raw) and np.array_equal(canon[n:], guard)
    inv = pow(zu.MONT, -1, zu.R)
    assert [zu.from_limbs(canon[i]) for i in some] == [zu.from_limbs(raw[i]) * inv % zu.R for i in some]
    buf.free()
    if n == 0:  # a null pointer with no elements is a no-op, with elements an error
        ar.fr_from_raw_dev(ctx, None, 0)
        ar.fr_to_repr_dev(ctx, None, 0)
        assert ctx.L.amdzk_fr_from_raw_dev(ctx.h, None, 1) != 0 and ctx.L.amdzk_fr_to_repr_dev(ctx.h, None, 1) != 0


@pytest.mark.parametrize("k", [4, 11])
@pytest.mark.parametrize("scale", [False, True])
def test_ntt_batch_of_host_columns(ctx, pkg, oracle, k, scale):
    """Three host columns in one submission (k = 4: one step; k = 11: two), with and without NTT_SCALE_NINV: each column
    is the oracle's transform (times 2^-k in the oracle's field arithmetic when scaled)."""
    ar = pkg.arithmetic
    n = 1 << k
    w = oracle.omega(k)
    cols = [zu.random_fr(n, seed=500 + k), np.tile(np.array(zu.limbs(zu.R - 1), dtype=np.uint64), (n, 1)), zu.skewed_fr(n, 510 + k, oracle)]
    got = ar.best_fft_batch(ctx, [c.copy() for c in cols], w, k, flags=ar.NTT_SCALE_NINV if scale else 0)
    ninv = np.tile(zu.fr_from_int(pow(n, -1, zu.R)), (n, 1))
    for c in range(3):
        want = oracle.best_fft(cols[c].copy(), w, k)
        assert np.array_equal(got[c], oracle.fr_mul(want, ninv) if scale else want), c


@pytest.fixture(scope="module")
def srs13(oracle):
    return oracle.srs_powers(zu.fr_from_int(0xC0FFEE), 1 << 13)


@pytest.mark.parametrize("ragged", [0, 123])
def test_msm_over_resident_columns_with_a_stride(ctx, pkg, oracle, srs13, ragged):
    """amdzk_msm_g1_dev as bench.py's BASELINE config 5 drives it, with what no test gave it: columns that are not packed
    (col_stride = len + 37, random junk between them), a full and a ragged length at k = 12, both bases. Each column
    equals the oracle's best_multiexp over bases[..len], and the scalar buffer comes back unchanged."""
    k, ncols = 12, 3
    n = 1 << k
    length, stride = n - ragged, n - ragged + 37
    g, gl = srs13[:n].copy(), srs13[n:].copy()
    params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
    host = zu.random_fr(ncols * stride, seed=71 + ragged).reshape(ncols, stride, 4)  # the junk: whatever the columns leave
    cols = [zu.random_fr(length, seed=80 + ragged), zu.skewed_fr(length, 81 + ragged, oracle), zu.random_fr(length, seed=82 + ragged)]
    cols[2][::5] = np.array(zu.limbs(zu.R - 1), dtype=np.uint64)
    for c in range(ncols):
        host[c, :length] = cols[c]
    buf = ctx.alloc(host.nbytes).upload(host)
    for basis, bases in ((0, g), (1, gl)):
        got = pkg.arithmetic.best_multiexp_dev(ctx, params.h, basis, buf, ncols, length, col_stride=stride)
        for c in range(ncols):
            assert np.array_equal(zu.jac_to_affine_host(oracle, got[c]), oracle.best_multiexp(cols[c], bases[:length])), (basis, c)
        assert np.array_equal(buf.download(host.shape), host), "the scalars are read, not written"
    buf.free()
    params.free()
