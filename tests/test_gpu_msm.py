"""GPU parity: amdzk_msm_g1* (HIP, gfx950) vs the oracle's best_multiexp restatement. Equality is on
the affine point (the reference's projective coordinates depend on rayon's thread count)."""
import json
import os

import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bn254_golden.json")))


@pytest.fixture(scope="module")
def srs14(oracle):
    return oracle.srs_powers(zu.fr_from_int(0xABCDEF12345), 1 << 14)


def check(ctx, pkg, oracle, params, bases, scalars, basis=0):
    got = pkg.arithmetic.best_multiexp(ctx, params.h, basis, scalars)
    want = oracle.best_multiexp(scalars, bases[: scalars.shape[0]])
    assert np.array_equal(zu.jac_to_affine_host(oracle, got), want)


def edge_column(n):
    return zu.fr_array_from_ints([[0, 1, zu.R - 1, 127, 128, 129, 255, 256, (1 << 253) % zu.R, (1 << 64) - 1][i % 10] for i in range(n)])


def test_msm_golden_vectors(ctx, pkg, oracle):
    srs = np.array([zu.point_from_ints((int(p[0], 16), int(p[1], 16))) for p in G["srs"]["g"]], dtype=np.uint64)
    params = pkg.kzg.ParamsKZG(ctx, 6, g=srs)
    for v in G["msm"]:
        s = zu.fr_array_from_ints([int(x, 16) for x in v["scalars"]])
        got = zu.point_to_ints(zu.jac_to_affine_host(oracle, params.commit(s)))
        want = None if v["result"] is None else (int(v["result"][0], 16), int(v["result"][1], 16))
        assert got == want, v["kind"]
    params.free()


@pytest.mark.parametrize("k", [1, 4, 8, 10, 11, 12, 13, 14])
def test_msm_uniform_matches_oracle(ctx, pkg, oracle, srs14, k):
    n = 1 << k
    params = pkg.kzg.ParamsKZG(ctx, k, g=srs14[:n].copy())
    check(ctx, pkg, oracle, params, srs14, zu.random_fr(n, seed=300 + k))
    params.free()


@pytest.mark.parametrize("k", [15, 17, 18])
def test_msm_prover_sizes_match_oracle(ctx, pkg, oracle, k):
    """Every window width the prover selects for the BASELINE configurations (c = 13 at k = 15, 17 and 18: msm.hip
    pick_window_bits) checked directly against the oracle's Pippenger: uniform scalars, a witness-like
    skewed column, and a short (ragged) column, in one batched call over the Lagrange basis."""
    n = 1 << k
    g = oracle.srs_powers(zu.fr_from_int(0x5EED0000 + k), n)
    params = pkg.kzg.ParamsKZG(ctx, k, g_lagrange=g)
    cols = [zu.random_fr(n, seed=900 + k), zu.skewed_fr(n, 910 + k, oracle)]
    got = pkg.arithmetic.best_multiexp_batch(ctx, params.h, 1, cols)
    for c in range(2):
        assert np.array_equal(zu.jac_to_affine_host(oracle, got[c]), oracle.best_multiexp(cols[c], g))
    short = zu.random_fr(n - 12345, seed=920 + k)
    check(ctx, pkg, oracle, params, g, short, basis=1)
    params.free()


def test_msm_edge_cases(ctx, pkg, oracle, srs14):
    k = 10
    n = 1 << k
    params = pkg.kzg.ParamsKZG(ctx, k, g=srs14[:n].copy(), g_lagrange=srs14[n:2 * n].copy())
    one = zu.fr_from_int(1)
    zeros = np.zeros((n, 4), np.uint64)
    # all zero -> identity in normal form (0,1,0)
    got = params.commit(zeros)
    assert zu.point_to_ints(zu.jac_to_affine_host(oracle, got)) is None
    # empty and ragged lengths (bases[..len])
    for m in (0, 1, 2, 3, 31, 33, 1000):
        check(ctx, pkg, oracle, params, srs14, zu.random_fr(m, seed=m + 1) if m else np.zeros((0, 4), np.uint64))
    # all ones: every digit lands in one bucket (heavy-bucket path)
    check(ctx, pkg, oracle, params, srs14, np.tile(one, (n, 1)))
    # r-1 (= -1), 2^k-boundaries of the window digits, skewed witness-like column
    check(ctx, pkg, oracle, params, srs14, np.tile(zu.fr_from_int(zu.R - 1), (n, 1)))
    check(ctx, pkg, oracle, params, srs14, edge_column(n))
    check(ctx, pkg, oracle, params, srs14, zu.skewed_fr(n, 77, oracle))
    # second basis
    check(ctx, pkg, oracle, params, srs14[n:], zu.random_fr(n, seed=5), basis=1)
    params.free()


def test_msm_repeated_and_identity_bases(ctx, pkg, oracle):
    """Bases that collide (same point many times, P and -P, identity): exercises the doubling and
    cancellation branches of the mixed addition."""
    k = 8
    n = 1 << k
    gen = oracle.generator()
    neg = zu.point_from_ints((1, zu.Q - 2))
    bases = np.tile(gen, (n, 1))
    bases[1::3] = neg
    bases[2::7] = 0
    params = pkg.kzg.ParamsKZG(ctx, k, g=bases)
    for seed, s in ((1, zu.random_fr(n, seed=41)), (2, np.tile(zu.fr_from_int(1), (n, 1))), (3, zu.skewed_fr(n, 3, oracle))):
        check(ctx, pkg, oracle, params, bases, s)
    params.free()


def test_msm_batch_columns(ctx, pkg, oracle, srs14):
    k, ncols = 12, 7
    n = 1 << k
    params = pkg.kzg.ParamsKZG(ctx, k, g_lagrange=srs14[:n].copy())
    cols = [zu.skewed_fr(n, 50 + c, oracle) if c % 2 else zu.random_fr(n, seed=60 + c) for c in range(ncols)]
    cols[3] = np.zeros((n, 4), np.uint64)
    got = pkg.arithmetic.best_multiexp_batch(ctx, params.h, 1, cols)
    for c in range(ncols):
        assert np.array_equal(zu.jac_to_affine_host(oracle, got[c]), oracle.best_multiexp(cols[c], srs14[:n]))
    params.free()


def test_msm_linearity_large(ctx, pkg, oracle):
    """Size-independent property at a size the naive oracle cannot reach quickly: with bases
    g_i = t^i G (known t), MSM(s, g) = (sum s_i t^i) G = eval_polynomial(s, t) * G."""
    k = 16
    n = 1 << k
    tau = zu.fr_from_int(123456789)
    g = oracle.srs_powers(tau, n)
    params = pkg.kzg.ParamsKZG(ctx, k, g=g)
    s = zu.random_fr(n, seed=8)
    got = zu.jac_to_affine_host(oracle, params.commit(s))
    e = oracle.eval_polynomial(s, tau)
    want = oracle.g1_mul_many(oracle.generator(), e.reshape(1, 4))[0]
    assert np.array_equal(got, want)
    assert np.array_equal(got, oracle.best_multiexp(s, g))
    params.free()


def test_srs_setup_on_device_matches_oracle(ctx, pkg, oracle):
    """amdzk_srs_setup (ParamsKZG::setup with an explicit trapdoor) against the oracle's tau-powers and
    closed-form Lagrange bases; then commit_lagrange(p) == commit(lagrange_to_coeff(p))."""
    k, tau = 10, 0x1234567890ABCDEF1234567
    n = 1 << k
    params = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(tau), want_host_copy=True)
    g, gl = zu.test_srs(oracle, k, tau)
    assert np.array_equal(params._g, g)
    assert np.array_equal(params._gl, gl)
    p = zu.random_fr(n, seed=31)
    od = zu.OracleDomain(oracle, 3, k)
    a = zu.jac_to_affine_host(oracle, params.commit_lagrange(p))
    b = zu.jac_to_affine_host(oracle, params.commit(od.lagrange_to_coeff(p)))
    assert np.array_equal(a, b) and np.array_equal(a, oracle.best_multiexp(p, gl))
    params.free()


def test_g_to_lagrange_matches_oracle(ctx, pkg, oracle):
    """arithmetic::g_to_lagrange on the device (FFT over G1): against the pure-Python restatement on
    small domains, including points at infinity and repeated points, and against the closed-form
    Lagrange basis of a tau-powers SRS at k = 10."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import pyref as P

    tau = 0x1234567890ABCDEF1234567
    for k in (0, 1, 3, 5):
        g, _ = zu.test_srs(oracle, k, tau)
        if k == 3:
            g[2] = 0          # identity
            g[5] = g[4]       # u == v -> u - v = identity, u + v = doubling
            x6, y6 = zu.point_to_ints(g[6])
            g[7] = zu.point_from_ints((x6, (-y6) % P.Q))  # v == -u
        got = pkg.arithmetic.g_to_lagrange(ctx, g, k)
        want = P.g_to_lagrange([zu.point_to_ints(p) for p in g], k)
        assert [zu.point_to_ints(p) for p in got] == want, k
    g, gl = zu.test_srs(oracle, 10, tau)
    assert np.array_equal(pkg.arithmetic.g_to_lagrange(ctx, g, 10), gl)


def test_params_downsize(ctx, pkg, oracle):
    """ParamsKZG::downsize: g truncated, g_lagrange recomputed for the smaller domain (equal to a fresh
    setup at that k with the same trapdoor), commitments agree across bases, growing is refused."""
    tau = 0x1234567890ABCDEF1234567
    params = pkg.kzg.ParamsKZG.setup(ctx, 10, zu.fr_from_int(tau), want_host_copy=True)
    with pytest.raises(pkg.AmdzkError):
        params.downsize(11)
    params.downsize(7)
    g, gl = zu.test_srs(oracle, 7, tau)
    assert params.k == 7 and params.n == 128
    assert np.array_equal(params.get_g(), g) and np.array_equal(params.get_g_lagrange(), gl)
    assert np.array_equal(params._g, g) and np.array_equal(params._gl, gl)
    p = zu.random_fr(128, seed=5)
    od = zu.OracleDomain(oracle, 3, 7)
    a = zu.jac_to_affine_host(oracle, params.commit_lagrange(p))
    assert np.array_equal(a, zu.jac_to_affine_host(oracle, params.commit(od.lagrange_to_coeff(p))))
    assert np.array_equal(a, oracle.best_multiexp(p, gl))
    fresh = pkg.kzg.ParamsKZG.setup(ctx, 7, zu.fr_from_int(tau))
    assert fresh.write() == params.write()
    fresh.free(); params.free()


def test_msm_k22_full_size_tau_identity(ctx, pkg, oracle):
    """BASELINE config 5 size. With bases g_i = s^i G (device-built SRS), MSM(c, g) must equal
    eval_polynomial(c, s) * G — a size-independent identity checked at n = 2^22 against the oracle's
    Horner evaluation and one oracle scalar multiplication."""
    k = 22
    n = 1 << k
    s = zu.fr_from_int(7 ** 20)
    params = pkg.kzg.ParamsKZG.setup(ctx, k, s)
    for seed, kind in ((42, "uniform"), (43, "skewed")):
        c = zu.random_fr(n, seed=seed)
        if kind == "skewed":
            sel = zu.splitmix64(seed + 9, n) % np.uint64(4)
            c[sel < 2] = 0
        got = zu.jac_to_affine_host(oracle, params.commit(c))
        e = oracle.eval_polynomial(c, s)
        want = oracle.g1_mul_many(oracle.generator(), e.reshape(1, 4))[0]
        assert np.array_equal(got, want), kind
    params.free()


def test_params_write_read_roundtrip(ctx, pkg, oracle):
    """ParamsKZG::write / ::read: device compression matches the pure-Python encoder on every point,
    read(write(p)) commits identically, and a corrupted encoding is rejected."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import plonk_ref as PR

    k, tau = 8, 0x1234567890ABCDEF1234567
    n = 1 << k
    params = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(tau), want_host_copy=True)
    g2, s_g2 = bytes(range(64)), bytes(range(64, 128))
    blob = params.write(g2, s_g2)
    assert len(blob) == 4 + 2 * n * 32 + 128 and int.from_bytes(blob[:4], "little") == k
    for i in (0, 1, 17, n - 1):
        assert blob[4 + 32 * i:4 + 32 * (i + 1)] == PR.g1_compress(zu.point_to_ints(params._g[i]))
        assert blob[4 + 32 * (n + i):4 + 32 * (n + i + 1)] == PR.g1_compress(zu.point_to_ints(params._gl[i]))
    p2, g2b, sg2b = pkg.kzg.ParamsKZG.read(ctx, blob)
    assert (g2b, sg2b) == (g2, s_g2)
    c = zu.random_fr(n, seed=4)
    assert np.array_equal(p2.commit(c), params.commit(c)) and np.array_equal(p2.commit_lagrange(c), params.commit_lagrange(c))
    bad = bytearray(blob)
    bad[4 + 32 * 5] ^= 1  # x of g[5] -> almost surely not on the curve (or a different point: then commits differ)
    try:
        p3, _, _ = pkg.kzg.ParamsKZG.read(ctx, bytes(bad))
        assert not np.array_equal(p3.commit(c), params.commit(c))
        p3.free()
    except pkg.AmdzkError as e:
        assert "invalid point" in str(e)
    with pytest.raises(pkg.AmdzkError):
        pkg.kzg.ParamsKZG.read(ctx, blob[:100])
    p2.free(); params.free()


# ------------------------------------------------------------------------------------------------------------------------
# The window-table MSM at every instantiation of its counting sort and at the task geometries of the large batches, at the
# smallest sizes where those paths exist. AMDZK_MSM_C is read when the window table is built (so it is set before the
# ParamsKZG is made), AMDZK_MSM_T1 / _TL / _BIG_DIGITS at every call's geometry. Every comparison is equality of the affine
# point with the oracle's best_multiexp; the oracle's points do not depend on the switches and are computed once.
def windows(c):
    return (255 + c - 1) // c


def params_with_width(ctx, pkg, monkeypatch, c, k, **bases):
    """A ParamsKZG whose window tables are c bits wide. That the switch was read is counted, not assumed: building a table
    of W = ceil(255 / c) rows is W - 1 launches of table_next_kernel per basis, and W differs for every c in 8..16."""
    monkeypatch.setenv("AMDZK_MSM_C", str(c))
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        params = pkg.kzg.ParamsKZG(ctx, k, **bases)
        launches = ctx.prof_dump()["msm_table_next"][0]
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    assert launches == len(bases) * (windows(c) - 1), "the window tables were not built %d bits wide" % c
    return params


def scattered(ctx, cols):
    """The columns in separate allocations, not in address order and 16-byte (not 32-byte) aligned: (buffers, addresses)."""
    bufs, ptrs = [], []
    for j in reversed(range(len(cols))):
        b = ctx.alloc(cols[j].nbytes + 64)
        off = 16 * (1 + j % 3)
        ctx._chk(ctx.L.amdzk_dev_upload(ctx.h, b.ptr.value + off, cols[j].ctypes.data, cols[j].nbytes))
        bufs.append(b)
        ptrs.append(b.ptr.value + off)
    return bufs, ptrs[::-1]


def strided_and_pointer_forms(ctx, pkg, oracle, params, want, cols, lengths, bases_used=(0,)):
    """amdzk_msm_g1_dev on the packed columns against `want[basis, length][column]`, then amdzk_msm_g1_cols_dev
    (msm_digit_kernel<.., PTRS>) on the same columns in separate allocations: word-equal to the strided result."""
    A = pkg.arithmetic
    n = cols[0].shape[0]
    packed = ctx.alloc(len(cols) * n * 32).upload(np.stack(cols))
    bufs, ptrs = scattered(ctx, cols)
    try:
        for basis in bases_used:
            for length in lengths:
                got = A.best_multiexp_dev(ctx, params.h, basis, packed, len(cols), length, col_stride=n)
                for j in range(len(cols)):
                    assert np.array_equal(zu.jac_to_affine_host(oracle, got[j]), want[basis, length][j]), "basis %d len %d column %d" % (basis, length, j)
                assert np.array_equal(A.best_multiexp_cols_dev(ctx, params.h, basis, ptrs, length), got), "pointer table, basis %d len %d" % (basis, length)
    finally:
        packed.free()
        for b in bufs:
            b.free()


@pytest.fixture(scope="module")
def width_cases(oracle, srs14):
    """k = 10, both bases of one SRS: a uniform column, a skewed one, the edge column of test_msm_edge_cases, an all-zero one and
    a second uniform one, at the full length and at n - 37; the oracle's points for all of it."""
    n = 1 << 10
    bases = (srs14[:n].copy(), srs14[n:2 * n].copy())
    cols = [zu.random_fr(n, seed=1310), zu.skewed_fr(n, 1311, oracle), edge_column(n), np.zeros((n, 4), np.uint64), zu.random_fr(n, seed=1314)]
    cols = [np.ascontiguousarray(col, dtype=np.uint64) for col in cols]
    want = {(b, m): [oracle.best_multiexp(col[:m], bases[b][:m]) for col in cols] for b in (0, 1) for m in (n, n - 37)}
    return bases, cols, want


@pytest.mark.parametrize("c", range(8, 17))
def test_msm_every_window_width_of_the_table_form(ctx, pkg, oracle, monkeypatch, width_cases, c):
    """msm_digit_kernel<C, .., false, PTRS> and table_next_kernel at every C the dispatch has, 8..16 (the chooser never
    returns 9 or 14, returns 15 and 16 only from 2^19 points up, and the pointer-table form above 10 bits only in proofs of
    k >= 13): single columns, a three-column host batch with an all-zero column, five resident columns strided and through a
    pointer table, both bases, full and ragged length."""
    (g, gl), cols, want = width_cases
    n = 1 << 10
    params = params_with_width(ctx, pkg, monkeypatch, c, 10, g=g, g_lagrange=gl)
    try:
        for j in (0, 1, 2):
            got = pkg.arithmetic.best_multiexp(ctx, params.h, j % 2, cols[j])
            assert np.array_equal(zu.jac_to_affine_host(oracle, got), want[j % 2, n][j]), "column %d" % j
        got = pkg.arithmetic.best_multiexp(ctx, params.h, 1, cols[0][:n - 37])
        assert np.array_equal(zu.jac_to_affine_host(oracle, got), want[1, n - 37][0]), "ragged"
        got = pkg.arithmetic.best_multiexp_batch(ctx, params.h, 0, [cols[0], cols[3], cols[1]])
        for i, j in enumerate((0, 3, 1)):
            assert np.array_equal(zu.jac_to_affine_host(oracle, got[i]), want[0, n][j]), "three columns, column %d" % j
        assert not got[1][8:].any()  # the all-zero column: the identity, z = 0
        strided_and_pointer_forms(ctx, pkg, oracle, params, want, cols, (n, n - 37), bases_used=(0, 1))
    finally:
        params.free()


@pytest.fixture(scope="module")
def two_workgroup_cases(oracle, srs14):
    """k = 13: 8192 scalars are two workgroups of the 1024-thread counting sort (4096 scalars each) and four of the 256-thread
    one; 4096 + 3 leaves the second 1024-thread workgroup three scalars."""
    n = 1 << 13
    g = srs14[:n].copy()
    cols = [zu.random_fr(n, seed=1320), zu.skewed_fr(n, 1321, oracle), zu.random_fr(n, seed=1322)]
    cols = [np.ascontiguousarray(col, dtype=np.uint64) for col in cols]
    want = {(0, m): [oracle.best_multiexp(col[:m], g[:m]) for col in cols] for m in (n, 4096 + 3)}
    return g, cols, want


@pytest.mark.parametrize("big", [1, 0])
@pytest.mark.parametrize("c", [14, 15, 16])
def test_msm_wide_windows_with_both_counting_sorts(ctx, pkg, oracle, monkeypatch, two_workgroup_cases, c, big):
    """msm_digit_kernel<C, .., BIG, PTRS> for C = 14, 15, 16 with BIG on and off (both arms of the dispatch's ZK_CASE2), strided
    and pointer-table form, more than one workgroup per column and a nearly empty last one. The chooser turns BIG on only
    from 2^18 points up, and C = 14 never."""
    g, cols, want = two_workgroup_cases
    params = params_with_width(ctx, pkg, monkeypatch, c, 13, g=g)
    monkeypatch.setenv("AMDZK_MSM_BIG_DIGITS", str(big))
    try:
        strided_and_pointer_forms(ctx, pkg, oracle, params, want, cols, (1 << 13, 4096 + 3))
    finally:
        params.free()


@pytest.fixture(scope="module")
def task_size_cases(oracle, srs14):
    """k = 12 at c = 8: 32 windows into 128 buckets, about 1000 entries per bucket, so that even tasks of 64 leave several
    partial sums per bucket for the folds. Uniform, skewed, and all ones: one bucket holds the whole column."""
    n = 1 << 12
    g = srs14[:n].copy()
    cols = [zu.random_fr(n, seed=1330), zu.skewed_fr(n, 1331, oracle), np.tile(zu.fr_from_int(1), (n, 1))]
    return g, cols, [oracle.best_multiexp(col, g) for col in cols]


@pytest.mark.parametrize("t1,tl", [(8, 6), (12, 7), (32, 9), (64, 16)])
def test_msm_task_sizes_of_the_large_geometries(ctx, pkg, oracle, monkeypatch, task_size_cases, t1, tl):
    """The task sizes msm_geometry_cw picks only for real batches (level 1: T1 = 8, 12 from a million entries, 32 and 64 from
    2^19 points; folds: TL = 7 at 2^17 points, 9 at 2^18, up to 16), forced at a small shape: every T1 and every TL once."""
    g, cols, want = task_size_cases
    params = params_with_width(ctx, pkg, monkeypatch, 8, 12, g=g)
    monkeypatch.setenv("AMDZK_MSM_T1", str(t1))
    monkeypatch.setenv("AMDZK_MSM_TL", str(tl))
    try:
        got = pkg.arithmetic.best_multiexp_batch(ctx, params.h, 0, cols)
        for j in range(3):
            assert np.array_equal(zu.jac_to_affine_host(oracle, got[j]), want[j]), "column %d" % j
        got = pkg.arithmetic.best_multiexp(ctx, params.h, 0, cols[2])  # alone: another column count, another grid
        assert np.array_equal(zu.jac_to_affine_host(oracle, got), want[2])
    finally:
        params.free()


def test_msm_colliding_partial_sums(ctx, pkg, oracle):
    """Partial sums that meet as P + P, as P + (-P) and as the identity at every stage behind level 1 — the folds, the row and
    column sums, the suffix sums of msm_fold — built so that the order in which the counting sort's atomics place entries
    cannot matter. Bucket b holds the digits b + 1; b = r + 64 g is residue r of row group g. Window widths stay at the
    chooser's (8 at k = 8, 10 at k = 12): the bucket reduction is then one wavefront wide, which is where the quad-lane
    kernels run (test_alternative_kernels_give_the_same_points runs this test with them forced)."""
    gen = oracle.generator()
    neg = zu.point_from_ints((1, zu.Q - 2))
    one = zu.fr_from_int(1)

    def run(k, bases, scalars, identity=False):
        params = pkg.kzg.ParamsKZG(ctx, k, g=bases)
        try:
            check(ctx, pkg, oracle, params, bases, scalars)
            if identity:
                assert zu.point_to_ints(zu.jac_to_affine_host(oracle, params.commit(scalars))) is None
        finally:
            params.free()

    # every base P, every scalar 1, n = 4096: one bucket, every level-1 sum the same point in the same representation, so the
    # second addition of every fold task is a doubling
    n = 1 << 12
    run(12, np.tile(gen, (n, 1)), np.tile(one, (n, 1)))
    # two buckets that hold P each (the same representation), in one row group and then at one residue of two row groups: the row
    # sum, then the column sum, is P + P; with -P in the second it cancels; a third point keeps the result off the identity
    n = 1 << 8
    others = oracle.g1_mul_many(gen, zu.random_fr(n, seed=1340))
    for b1, b2 in ((3, 40), (5, 64 + 5)):
        for second in (gen, neg):
            bases = others.copy()
            bases[17], bases[200] = gen, second
            s = np.zeros((n, 4), np.uint64)
            s[17], s[200], s[99] = zu.fr_from_int(b1 + 1), zu.fr_from_int(b2 + 1), zu.fr_from_int(64 + 23)
            run(8, bases, s)
            s[99] = 0  # and nothing else in the column
            run(8, bases, s)
    # 3 P + 5 P - 8 P: three buckets of one row group whose weighted sum is the identity (the last addition of msm_fold cancels)
    bases = others.copy()
    bases[1], bases[2], bases[3] = gen, gen, neg
    s = np.zeros((n, 4), np.uint64)
    s[1], s[2], s[3] = zu.fr_from_int(3), zu.fr_from_int(5), zu.fr_from_int(8)
    run(8, bases, s, identity=True)
    # full-width scalars: x P + x (-P) + y P + y (-P) cancels in every window's bucket at level 1, the total is the identity
    s = np.zeros((n, 4), np.uint64)
    s[1], s[3], s[2] = zu.random_fr(1, seed=1341)[0], zu.random_fr(1, seed=1341)[0], zu.random_fr(1, seed=1342)[0]
    bases[4] = neg
    s[4] = s[2]
    run(8, bases, s, identity=True)
    # c = 10, 512 buckets in 8 row groups: three non-empty buckets in three row groups (equal points, then different ones), so
    # that the suffix sums of the row sums coincide over runs of lanes and meet as P + P in the shift-and-add rounds
    n = 1 << 12
    pts = oracle.g1_mul_many(gen, zu.random_fr(n, seed=1343))
    for same in (True, False):
        bases = pts.copy()
        if same:
            bases[10] = bases[2000] = bases[4000] = gen
        s = np.zeros((n, 4), np.uint64)
        s[10], s[2000], s[4000] = zu.fr_from_int(5 + 1), zu.fr_from_int(64 * 3 + 17 + 1), zu.fr_from_int(64 * 6 + 40 + 1)
        run(12, bases, s)


@pytest.mark.parametrize("env", [{"AMDZK_TAIL_QUAD": "1"}, {"AMDZK_TAIL_QUAD": "0", "AMDZK_TAIL_TREE": "1"}])
def test_alternative_kernels_give_the_same_points(env):
    """The kernel variants that only run in a proof's latency mode (the bucket reduction with quad-lane point additions, or
    with shuffle-tree row / column sums) must give the oracle's points too: the parity tests above — the two with colliding
    bases and colliding partial sums among them, where the quad formulas double and cancel — again, in a child process with
    the switch forced (the switches are read once per process). One child per setting, one timeout, nothing started again."""
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                        "golden_vectors or uniform_matches_oracle or edge or batch or repeated_and_identity_bases or colliding_partial_sums"], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0, "%r:\n%s" % (env, r.stdout[-3000:])
    assert " passed" in r.stdout and "failed" not in r.stdout
