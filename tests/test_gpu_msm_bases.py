"""GPU parity: amdzk_msm_g1_bases* — best_multiexp over caller-supplied bases, no amdzk_srs and no window table — against the
oracle's best_multiexp restatement. Equality is always on the affine point, bit for bit (exact arithmetic, no tolerance)."""
import ctypes as C
import os

import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 31, 33, 1000, 12345] + [1 << k for k in (1, 4, 8, 10, 11, 12, 13, 14)] + [(1 << 16) + 1]
E_INVALID, E_UNSUPPORTED = -2, -5


@pytest.fixture(scope="module")
def bases(oracle):
    """2^16 + 1 points that are NOT an SRS: random multiples of the generator."""
    return oracle.g1_mul_many(oracle.generator(), zu.random_fr((1 << 16) + 1, seed=0xBA5E5))


def affine(oracle, jac):
    return zu.jac_to_affine_host(oracle, jac)


def check(ctx, pkg, oracle, scalars, pts):
    got = pkg.arithmetic.best_multiexp_bases(ctx, scalars, pts)
    assert np.array_equal(affine(oracle, got), oracle.best_multiexp(scalars, pts))


def edge_scalars(n):
    return zu.fr_array_from_ints([[0, 1, zu.R - 1, 127, 128, 129, 255, 256, (1 << 253) % zu.R, (1 << 64) - 1][i % 10] for i in range(n)])


@pytest.mark.parametrize("n", LENGTHS)
def test_bases_uniform_matches_oracle(ctx, pkg, oracle, bases, n):
    s = zu.random_fr(n, seed=700 + n) if n else np.zeros((0, 4), np.uint64)
    pts = bases[:n].copy()
    if n == 0:
        got = pkg.arithmetic.best_multiexp_bases(ctx, s, pts)
        assert zu.point_to_ints(affine(oracle, got)) is None  # the identity in normal form (0, 1, 0)
        return
    check(ctx, pkg, oracle, s, pts)
    assert np.array_equal(pts, bases[:n]), "the caller's bases are read only"


@pytest.mark.parametrize("n", LENGTHS)
def test_bases_edge_scalar_patterns(ctx, pkg, oracle, bases, n):
    """Skewed witness-like columns, all zero, all one (one bucket of window 0 holds every point), all r - 1, and the
    digit-boundary pattern of test_gpu_msm.test_msm_edge_cases."""
    if n == 0:
        return  # covered above: no scalars, no pattern
    pts = bases[:n]
    check(ctx, pkg, oracle, zu.skewed_fr(n, 710 + n, oracle), pts)
    got = pkg.arithmetic.best_multiexp_bases(ctx, np.zeros((n, 4), np.uint64), pts)
    assert zu.point_to_ints(affine(oracle, got)) is None
    check(ctx, pkg, oracle, np.tile(zu.fr_from_int(1), (n, 1)), pts)
    check(ctx, pkg, oracle, np.tile(zu.fr_from_int(zu.R - 1), (n, 1)), pts)
    check(ctx, pkg, oracle, edge_scalars(n), pts)


def test_bases_repeated_and_identity_points(ctx, pkg, oracle):
    """Bases that collide (the same point many times, P next to -P, identities): the doubling and cancellation branches of
    the mixed addition, the folds and the window combine."""
    n = 1 << 8
    gen = oracle.generator()
    neg = zu.point_from_ints((1, zu.Q - 2))
    pts = np.tile(gen, (n, 1))
    pts[1::3] = neg
    pts[2::7] = 0
    for s in (zu.random_fr(n, seed=41), np.tile(zu.fr_from_int(1), (n, 1)), zu.skewed_fr(n, 3, oracle), edge_scalars(n)):
        check(ctx, pkg, oracle, s, pts)
    # every point the identity
    got = pkg.arithmetic.best_multiexp_bases(ctx, zu.random_fr(n, seed=42), np.zeros((n, 8), np.uint64))
    assert zu.point_to_ints(affine(oracle, got)) is None


def widths_and_lengths(pkg):
    """Every window width the chooser returns for some length up to 2^26, with the largest power of two up to 2^22 it returns
    it for."""
    plan = pkg.arithmetic.multiexp_bases_plan
    probe = sorted({1 << k for k in range(0, 27)} | {3 << k for k in range(0, 25)} | {5 << k for k in range(0, 24)})
    all_widths = {plan(1, n)["window_bits"] for n in probe}
    by_width = {}
    for k in range(0, 23):
        by_width[plan(1, 1 << k)["window_bits"]] = 1 << k
    assert set(by_width) == all_widths, "a width the chooser returns has no test length <= 2^22: %r vs %r" % (sorted(by_width), sorted(all_widths))
    return by_width


def test_bases_every_window_width_the_chooser_returns(ctx, pkg, oracle, bases):
    by_width = widths_and_lengths(pkg)
    assert len(by_width) >= 2
    small = {c: n for c, n in by_width.items() if n <= 1 << 18}
    large = {c: n for c, n in by_width.items() if n > 1 << 18}
    if small:
        top = max(small.values())
        pts = bases if top <= bases.shape[0] else np.concatenate(
            [bases, oracle.g1_mul_many(oracle.generator(), zu.random_fr(top - bases.shape[0], seed=0xBA5E6))])
        for c, n in sorted(small.items()):
            for s in (zu.random_fr(n, seed=800 + c), zu.skewed_fr(n, 810 + c, oracle)):
                got = pkg.arithmetic.best_multiexp_bases(ctx, s, pts[:n])
                assert np.array_equal(affine(oracle, got), oracle.best_multiexp(s, pts[:n])), (c, n)
    if large:
        # above 2^18 the naive oracle is too slow: device-built tau-power bases and MSM(s, g) = eval_polynomial(s, tau) * G
        kmax = max(large.values()).bit_length() - 1
        tau = zu.fr_from_int(7 ** 20)
        params = pkg.kzg.ParamsKZG.setup(ctx, kmax, tau)
        g = params.get_g()
        params.free()
        for c, n in sorted(large.items()):
            for kind in ("uniform", "half zero"):
                s = zu.random_fr(n, seed=820 + c)
                if kind == "half zero":
                    s[zu.splitmix64(830 + c, n) % np.uint64(4) < 2] = 0
                got = affine(oracle, pkg.arithmetic.best_multiexp_bases(ctx, s, g[:n]))
                e = oracle.eval_polynomial(s, tau)
                assert np.array_equal(got, oracle.g1_mul_many(oracle.generator(), e.reshape(1, 4))[0]), (c, n, kind)


@pytest.mark.parametrize("c", range(8, 17))
def test_bases_every_instantiated_width_forced(ctx, pkg, oracle, bases, monkeypatch, c):
    """All nine digit-kernel instantiations, whatever the chooser prefers today: AMDZK_MSM_BASES_C is read at every call.
    The widths with a poorly filled top window (9, 11, 12, 14: two or four very full buckets) are among them."""
    monkeypatch.setenv("AMDZK_MSM_BASES_C", str(c))
    n = 5000
    assert pkg.arithmetic.multiexp_bases_plan(1, n)["window_bits"] == c
    for s in (zu.random_fr(n, seed=840 + c), zu.skewed_fr(n, 850 + c, oracle), edge_scalars(n)):
        check(ctx, pkg, oracle, s, bases[:n])
    cols = [zu.random_fr(n, seed=860 + c), np.zeros((n, 4), np.uint64), zu.skewed_fr(n, 870 + c, oracle)]
    got = pkg.arithmetic.best_multiexp_bases_batch(ctx, cols, bases[:n])
    for i in range(3):
        assert np.array_equal(affine(oracle, got[i]), oracle.best_multiexp(cols[i], bases[:n])), (c, i)


def test_bases_batch_columns_host_and_resident(ctx, pkg, oracle, bases):
    n, ncols = 1 << 12, 7
    pts = bases[:n].copy()
    cols = [zu.skewed_fr(n, 50 + c, oracle) if c % 2 else zu.random_fr(n, seed=60 + c) for c in range(ncols)]
    cols[3] = np.zeros((n, 4), np.uint64)
    want = [oracle.best_multiexp(c, pts) for c in cols]
    got = pkg.arithmetic.best_multiexp_bases_batch(ctx, cols, pts)
    for c in range(ncols):
        assert np.array_equal(affine(oracle, got[c]), want[c]), c
    # resident scalars with col_stride > len, resident bases; the bases come back untouched
    stride = n + 37
    host = np.zeros((ncols, stride, 4), np.uint64)
    for c in range(ncols):
        host[c, :n] = cols[c]
        host[c, n:] = zu.random_fr(stride - n, seed=90 + c)  # what lies between the columns must not be read
    d_s = ctx.alloc(host.nbytes).upload(host)
    d_b = ctx.alloc(pts.nbytes).upload(pts)
    got = pkg.arithmetic.best_multiexp_bases_dev(ctx, d_s, d_b, ncols, n, col_stride=stride)
    for c in range(ncols):
        assert np.array_equal(affine(oracle, got[c]), want[c]), c
    assert np.array_equal(d_b.download(pts.shape), pts), "the bases buffer must come back as it was uploaded"
    assert np.array_equal(d_s.download(host.shape), host)
    # a ragged length over the same resident buffers
    m = 1000
    got = pkg.arithmetic.best_multiexp_bases_dev(ctx, d_s, d_b, ncols, m, col_stride=stride)
    for c in range(ncols):
        assert np.array_equal(affine(oracle, got[c]), oracle.best_multiexp(cols[c][:m], pts[:m])), c
    d_s.free(); d_b.free()


@pytest.mark.parametrize("k", [10, 15])
def test_bases_same_words_as_the_table_route(ctx, pkg, oracle, bases, k):
    """Both routes return the normalised point: the 12 output words are equal, not only the group element."""
    n = 1 << k
    pts = bases[:n].copy()
    s = zu.random_fr(n, seed=1000 + k)
    params = pkg.kzg.ParamsKZG(ctx, k, g=pts)
    via_table = params.commit(s)
    params.free()
    got = pkg.arithmetic.best_multiexp_bases(ctx, s, pts)
    assert got.shape == (12,) and np.array_equal(got, np.asarray(via_table).reshape(12))


def test_bases_refusals_name_their_reason_and_leave_the_ctx_usable(ctx, pkg, oracle, bases):
    L = ctx.L
    n = 1 << 10
    pts = bases[:n].copy()
    s = zu.random_fr(n, seed=5)
    out = np.zeros((4, 12), np.uint64)
    d_s = ctx.alloc(2 * s.nbytes).upload(np.concatenate([s, s]))
    d_b = ctx.alloc(pts.nbytes).upload(pts)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(rc, codes, *words):
        assert rc in codes, rc
        msg = L.amdzk_last_error(ctx.h).decode()
        assert all(w in msg for w in words), msg
        check(ctx, pkg, oracle, s, pts)  # the next valid call on the same ctx gives the oracle's point

    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 0, n, n, d_b.ptr, p(out)), (E_INVALID,), "ncols")
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, None, 1, n, n, d_b.ptr, p(out)), (E_INVALID,), "null")
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 1, n, n, None, p(out)), (E_INVALID,), "null")
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 1, n, n, d_b.ptr, None), (E_INVALID,), "null")
    refused(L.amdzk_msm_g1_bases(ctx.h, None, p(pts), n, p(out)), (E_INVALID,), "null")
    refused(L.amdzk_msm_g1_bases(ctx.h, p(s), None, n, p(out)), (E_INVALID,), "null")
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 2, n, n - 1, d_b.ptr, p(out)), (E_INVALID,), "col_stride")
    windows = pkg.arithmetic.multiexp_bases_plan(1, n)["windows"]
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 65535 // windows + 1, n, 0, d_b.ptr, p(out)), (E_INVALID, E_UNSUPPORTED), "65535")
    refused(L.amdzk_msm_g1_bases_dev(ctx.h, d_s.ptr, 1, 1 << 31, 1 << 31, d_b.ptr, p(out)), (E_INVALID, E_UNSUPPORTED), "2^31")
    d_s.free(); d_b.free()


@pytest.mark.parametrize("env", [{"AMDZK_TAIL_QUAD": "1"}, {"AMDZK_TAIL_QUAD": "0", "AMDZK_TAIL_TREE": "1"}])
def test_bases_alternative_tail_kernels_give_the_same_points(env):
    """The bucket reduction with quad-lane point additions, or with shuffle-tree row / column sums, under the table-free
    driver: the uniform, edge and batch tests above once more in a child process with the switch forced (the switches are
    read once per process). One child per setting, its own timeout, no retries."""
    import subprocess
    import sys
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                        "uniform_matches_oracle or edge_scalar_patterns or batch_columns"], env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, "%r:\n%s" % (env, r.stdout[-3000:])
    assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("k", [6, 13])
def test_cpp_best_multiexp_equals_commit(tmp_path, k):
    """include/amdzk_halo2.hpp's free function best_multiexp(ctx, coeffs, bases), driven from C++
    (tests/native/best_multiexp_check.cpp): the words ParamsKZG::commit returns over the same points, at the full length, a
    ragged one, 1 and 0, and a length mismatch refused. Both widths the chooser returns (k = 6: 12 bits, k = 13: 13)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, libdir = str(tmp_path / "best_multiexp_check"), os.path.join(root, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "native", "best_multiexp_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe, str(k), "%x" % 0x1234567890ABCDEF1234567], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok %d" % k), r.stdout[-2000:]
