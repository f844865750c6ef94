"""GPU: the prefix-sum basis of an amdzk_srs (AMDZK_BASIS_G_LAGRANGE_PREFIX): S_i = g_lagrange[0] + ... + g_lagrange[i], built on the
device the first time a proving key with permutation columns is made on the parameters, and the identity the prover relies on,

    MSM(Z, g_lagrange) = MSM(D, S),   D[i] = Z[i] - Z[i+1] (i < n-1),   D[n-1] = Z[n-1]

as normalised points, against the device's own g_lagrange MSM AND the oracle's Pippenger. The EC prefix scan works in chunks
of 16 points, level over level: k = 4 is one chunk (no level above it), k = 8 sixteen chunks whose totals are one chunk,
k = 12 two levels of totals (256, then 16)."""
import numpy as np
import pytest

import circuits
import zkutil as zu

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
KS = [4, 8, 12]
_srs = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def srs(oracle, k):
    if k not in _srs:
        _srs[k] = zu.test_srs(oracle, k, TAU)
    return _srs[k]


def key_with_permutation(ctx, plonk, oracle, params, k):
    c = circuits.square_circuit(plonk, k)  # three equality-enabled columns
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    return plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(5))


def differences(z):
    n = len(z)
    return [(z[i] - z[i + 1]) % zu.R for i in range(n - 1)] + [z[n - 1] % zu.R]  # D[n-1] = Z[n-1]


def jump_column(n, rows, seed):
    """Constant between jumps: Z[i] != Z[i+1] exactly for i in rows (i < n-1); n-1 in rows: Z[n-1] != 0 (a jump to the
    nothing behind the last row), else Z[n-1] = 0."""
    rnd = np.random.RandomState(seed)
    z, cur = [0] * n, 0
    for i in range(n - 1, -1, -1):
        if i in rows:
            cur = (cur + 1 + int(rnd.randint(0, 1 << 62)) * int(rnd.randint(1, 1 << 62)) * int(rnd.randint(1, 1 << 62))) % zu.R
        z[i] = cur
    d = differences(z)
    assert [i for i in range(n) if d[i]] == sorted(rows)
    return z


def columns(n, k):
    rnd = np.random.RandomState(40 + k)
    uni = zu.fr_array_to_ints(zu.random_fr(n, seed=500 + k))
    with_zeros = [0 if rnd.rand() < 0.4 else v for v in zu.fr_array_to_ints(zu.random_fr(n, seed=600 + k))]
    with_zeros[0] = with_zeros[n - 1] = 0
    eight = {0, n - 2, n - 1} | {int(x) for x in rnd.choice(np.arange(1, n - 2), 5, replace=False)}
    return [("uniform", uni),
            ("one_jump_row_0", jump_column(n, {0}, 1)),
            ("two_jumps_rows_n-2_n-1", jump_column(n, {n - 2, n - 1}, 2)),
            ("eight_jumps", jump_column(n, eight, 3)),
            ("all_equal", [123456789] * n),
            ("zeros", with_zeros),
            ("all_zero", [0] * n)]


def unit(n, i):
    e = np.zeros((n, 4), np.uint64)
    e[i] = zu.fr_from_int(1)
    return e


@pytest.mark.parametrize("k", KS)
def test_differences_over_prefix_sums_equal_values_over_g_lagrange(ctx, pkg, plonk, oracle, k):
    n = 1 << k
    g, gl = srs(oracle, k)
    params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
    A, PFX = pkg.arithmetic, pkg.kzg.BASIS_G_LAGRANGE_PREFIX
    # refused, not a crash, while the parameters have no key — and usable afterwards
    with pytest.raises(pkg.AmdzkError, match="prefix-sum basis has not been built"):
        A.best_multiexp(ctx, params.h, PFX, zu.random_fr(n, seed=1))
    pk = key_with_permutation(ctx, plonk, oracle, params, k)
    cols = columns(n, k)
    assert len(cols) == 7
    for name, z in cols:  # one by one
        zf, df = zu.fr_array_from_ints(z), zu.fr_array_from_ints(differences(z))
        got = zu.jac_to_affine_host(oracle, A.best_multiexp(ctx, params.h, PFX, df))
        assert np.array_equal(got, zu.jac_to_affine_host(oracle, params.commit_lagrange(zf))), name
        assert np.array_equal(got, oracle.best_multiexp(zf, gl)), name
    # ... and the seven in one batch
    got = A.best_multiexp_batch(ctx, params.h, PFX, [zu.fr_array_from_ints(differences(z)) for _, z in cols])
    want = A.best_multiexp_batch(ctx, params.h, pkg.kzg.BASIS_G_LAGRANGE, [zu.fr_array_from_ints(z) for _, z in cols])
    for c, (name, z) in enumerate(cols):
        assert np.array_equal(zu.jac_to_affine_host(oracle, got[c]), zu.jac_to_affine_host(oracle, want[c])), name
    # device-resident differences too (the prover's entry point)
    d = np.stack([zu.fr_array_from_ints(differences(z)) for _, z in cols])
    buf = ctx.alloc(d.nbytes).upload(d)
    dev = A.best_multiexp_dev(ctx, params.h, PFX, buf, len(cols), n, col_stride=n)
    assert np.array_equal(dev, got)
    buf.free()
    pk.free(); params.free()


@pytest.mark.parametrize("k", KS)
def test_prefix_sums_themselves(ctx, pkg, plonk, oracle, k):
    """S_i read back as MSM(e_i, S): S_0 = L_0, S_{n-1} = g[0] (sum_i L_i = 1: the commitment of the constant polynomial 1
    over g), and S_i at the chunk edges of every level against the oracle's sum of g_lagrange[0..i]."""
    n = 1 << k
    g, gl = srs(oracle, k)
    params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
    pk = key_with_permutation(ctx, plonk, oracle, params, k)
    A, PFX = pkg.arithmetic, pkg.kzg.BASIS_G_LAGRANGE_PREFIX
    s = lambda i: zu.jac_to_affine_host(oracle, A.best_multiexp(ctx, params.h, PFX, unit(n, i)))
    assert np.array_equal(s(0), gl[0])
    one = unit(n, 0)  # the polynomial 1, coefficient form
    assert np.array_equal(s(n - 1), zu.jac_to_affine_host(oracle, params.commit(one)))
    assert np.array_equal(s(n - 1), g[0])
    ones = np.tile(zu.fr_from_int(1), (n, 1))
    for i in sorted({1, 14, 15, 16, 17, 31, 32, 255, 256, 257, 511, 512, 4079, 4080, n - 2, n - 1}):
        if i < n:
            assert np.array_equal(s(i), oracle.best_multiexp(ones[:i + 1], gl[:i + 1])), i
    pk.free(); params.free()


def prefix_builds(prof):
    return prof.get("srs_prefix_apply", (0, 0.0))[0]


def test_basis_is_built_once_per_srs(ctx, pkg, plonk, oracle):
    """Two keys on one SRS, made on two contexts: the scan's kernels are launched for ONE build (counted by the per-kernel
    profile of both contexts), and a key without permutation columns builds nothing."""
    k = 8
    g, gl = srs(oracle, k)
    per_build = 2  # k = 8: the 16 chunk totals are scanned by one launch, then the bottom level's
    ctx.prof_enable(True)
    ctx2 = pkg.Context(0)
    ctx2.prof_enable(True)
    try:
        # no permutation columns: no basis
        params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
        ctx.prof_reset()
        c = circuits.random_circuit(plonk, k, seed=no_perm_seed(plonk, k))
        pk0 = plonk.ProvingKey(ctx, params, c.desc, np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]), c.assembly.mapping, zu.fr_from_int(5))
        assert prefix_builds(ctx.prof_dump()) == 0
        with pytest.raises(pkg.AmdzkError, match="prefix-sum basis has not been built"):
            pkg.arithmetic.best_multiexp(ctx, params.h, pkg.kzg.BASIS_G_LAGRANGE_PREFIX, zu.random_fr(1 << k, seed=1))
        # one after the other
        pk1 = key_with_permutation(ctx, plonk, oracle, params, k)
        assert prefix_builds(ctx.prof_dump()) == per_build
        pk2 = key_with_permutation(ctx2, plonk, oracle, params, k)
        assert prefix_builds(ctx.prof_dump()) == per_build and prefix_builds(ctx2.prof_dump()) == 0
        z = zu.fr_array_to_ints(zu.random_fr(1 << k, seed=9))
        got = pkg.arithmetic.best_multiexp(ctx2, params.h, pkg.kzg.BASIS_G_LAGRANGE_PREFIX, zu.fr_array_from_ints(differences(z)))
        assert np.array_equal(zu.jac_to_affine_host(oracle, got), oracle.best_multiexp(zu.fr_array_from_ints(z), gl))
        for pk in (pk0, pk1, pk2):
            pk.free()
        params.free()
    finally:
        ctx.prof_enable(False)
        ctx2.close()


def no_perm_seed(plonk, k):
    for seed in range(200):
        if not circuits.random_circuit(plonk, k, seed).cs.permutation_columns:
            return seed
    raise AssertionError("the generator made no circuit without permutation columns")
