"""GPU: amdzk_srs_check — the structure of an SRS checked on the device — and the G2 points of the ParamsKZG file. Expected
verdicts and the four sums come from tests/srs_check_ref.py (Python integers, with the trapdoor), never from the code under
test. Honest parameters come from ParamsKZG.setup / g2_setup; wrong ones are honest ones with entries moved (still on the
curve), parts of two setups put together, or single coordinates changed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import zkutil as zu

import pairing_ref as X
import srs_check_ref as SR
from test_g2_codec import ref_encode, small_x_candidates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

S1, S2 = 0x1234567890ABCDEF1234567, 0x0FEDCBA9876543210FEDCBA987
RHO = 0x2B1C0D9E8F7A6B5C4D3E2F1A0B9C8D7E6F5A4B3C2D1E0F9A8B7C6D5E4F3A2B1 % SR.R
G2, CURVE, POWERS, LAGRANGE, ALL = SR.CHECK_G2, SR.CHECK_CURVE, SR.CHECK_POWERS, SR.CHECK_LAGRANGE, SR.ALL


@pytest.fixture(scope="module")
def kzg(pkg):
    return pkg.kzg


@pytest.fixture(scope="module")
def honest(ctx, kzg):
    """(params with host copies, g2, s_g2) per (k, trapdoor), made once and never modified."""
    made = {}

    def get(k, s=S1):
        if (k, s) not in made:
            made[(k, s)] = (kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(s), want_host_copy=True),) + tuple(kzg.g2_setup(ctx, zu.fr_from_int(s)))
        return made[(k, s)]
    yield get
    for p, _, _ in made.values():
        p.free()


@pytest.fixture(scope="module")
def logs():
    made = {}

    def get(k, s=S1):
        if (k, s) not in made:
            made[(k, s)] = SR.honest_logs(s, k)
        return made[(k, s)]
    return get


def report_points(rep):
    w = np.array(list(rep.points), dtype=np.uint64).reshape(4, 8)
    return [zu.point_to_ints(p) for p in w]


def clean(rep, asked=ALL):
    return rep.ran == asked and rep.failed == 0


# ------------------------------------------------------------------------------------ honest parameters
@pytest.mark.parametrize("k", [0, 1, 2, 3, 6, 10])
def test_an_honest_srs_passes_every_check(kzg, honest, logs, k):
    params, g2, s_g2 = honest(k)
    rep = params.check(g2, s_g2, seed=7)
    assert rep.ran == ALL and rep.failed == 0 and list(rep.g2_status) == [0, 0]
    assert bytes(rep) == bytes(params.check(g2, s_g2, seed=7)), "the same seed gives the same report"
    assert clean(params.check(g2, s_g2))  # a seed from the OS generator
    if k > 3:
        return
    # the four sums, for the caller's rho and for a seed: the shifts, the zero ends, omega^-1 and 1/n, the seed's derivation
    for rho, kw in ((RHO, {"rho": zu.fr_from_int(RHO)}), (SR.rho_of_seed(7), {"seed": 7}), (SR.rho_of_seed(2**64 - 1), {"seed": 2**64 - 1})):
        want = SR.expected(*logs(k), S1, rho, k)
        assert want["powers"] and want["lagrange"]
        rep = params.check(g2, s_g2, **kw)
        assert clean(rep)
        assert report_points(rep) == [SR.point(v) for v in want["logs"]]
    if k == 0:
        pts = report_points(params.check(g2, s_g2, rho=zu.fr_from_int(RHO)))
        assert pts[0] is None and pts[1] is None and pts[2] == pts[3] == SR.G  # no pair: vacuous; C = E = rho^0 g[0]


def test_rho_wins_over_the_seed(honest):
    params, g2, s_g2 = honest(3)
    a, b = params.check(g2, s_g2, rho=zu.fr_from_int(RHO), seed=1), params.check(g2, s_g2, rho=zu.fr_from_int(RHO), seed=2)
    assert bytes(a) == bytes(b) and bytes(a) != bytes(params.check(g2, s_g2, seed=1))


# ------------------------------------------------------------------------------------ one wrong entry, still on the curve
def swapped(arr, i, j):
    out = arr.copy()
    out[[i, j]] = out[[j, i]]
    return out


def swap_cases(k):
    n = 1 << k
    pairs = [(0, 1), (n // 2 - 1, n // 2), (n - 2, n - 1)] if k > 2 else [(0, 1), (1, 2), (2, 3)]
    return [("g", p) for p in pairs] + [("gl", p) for p in (pairs[0], pairs[2])]


@pytest.mark.parametrize("k", [2, 6, 10])
def test_two_swapped_entries_fail_the_check_that_reads_them(ctx, kzg, honest, logs, k):
    params, g2, s_g2 = honest(k)
    g_logs, gl_logs = logs(k)
    rho = SR.rho_of_seed(11)
    for which, (i, j) in swap_cases(k):
        g, gl, gw, glw = params._g, params._gl, list(g_logs), list(gl_logs)
        if which == "g":
            g, gw[i], gw[j] = swapped(g, i, j), gw[j], gw[i]
        else:
            gl, glw[i], glw[j] = swapped(gl, i, j), glw[j], glw[i]
        want = SR.expected(gw, glw, S1, rho, k)
        assert want["powers"] is (which != "g") and (which == "g" or want["lagrange"] is False)
        bad = kzg.ParamsKZG(ctx, k, g, gl)
        try:
            rep = bad.check(g2, s_g2, seed=11)
        finally:
            bad.free()
        assert rep.ran & CURVE and not rep.failed & (CURVE | G2), (which, i, j)
        if which == "g":  # LAGRANGE is sound only given POWERS: not run
            assert rep.ran == G2 | CURVE | POWERS and rep.failed == POWERS, (which, i, j)
        else:
            assert rep.ran == ALL and rep.failed == LAGRANGE, (which, i, j)
        if k == 2:
            assert report_points(rep)[:3 if which == "g" else 4] == [SR.point(v) for v in want["logs"]][:3 if which == "g" else 4]


# ------------------------------------------------------------------------------------ honest parts, wrongly paired
def test_honest_parts_of_two_setups_do_not_pass_together(ctx, kzg, honest, logs):
    k = 3
    params, g2, s_g2 = honest(k)
    other, _, other_s_g2 = honest(k, S2)
    rho = SR.rho_of_seed(5)
    # s_g2 of another trapdoor
    assert not SR.expected(*logs(k), S2, rho, k)["powers"]
    rep = params.check(g2, other_s_g2, seed=5)
    assert rep.ran == G2 | CURVE | POWERS and rep.failed == POWERS
    # g2 and s_g2 swapped: s2 = 1 / s
    assert not SR.expected(*logs(k), pow(S1, -1, SR.R), rho, k)["powers"]
    rep = params.check(s_g2, g2, seed=5)
    assert rep.ran == G2 | CURVE | POWERS and rep.failed == POWERS
    # g_lagrange of another trapdoor, consistent in itself
    want = SR.expected(logs(k)[0], logs(k, S2)[1], S1, rho, k)
    assert want["powers"] and want["lagrange"] is False
    mixed = kzg.ParamsKZG(ctx, k, params._g, other._gl)
    try:
        rep = mixed.check(g2, s_g2, seed=5)
    finally:
        mixed.free()
    assert rep.ran == ALL and rep.failed == LAGRANGE
    assert report_points(rep) == [SR.point(v) for v in want["logs"]]


# ------------------------------------------------------------------------------------ CURVE
def bumped(arr, i):
    out = arr.copy()
    out[i, 4] += np.uint64(1)  # the lowest word of y
    return out


@pytest.mark.parametrize("where,first", [
    ([("g", 0)], (0, 0)), ([("g", -1)], (0, 15)), ([("gl", 0)], (1, 0)), ([("gl", -1)], (1, 15)),
    ([("g", -1), ("gl", 0)], (0, 15)), ([("g", 3), ("g", 9)], (0, 3)), ([("gl", 7), ("gl", 2)], (1, 2)),
])
def test_a_point_off_the_curve_is_found_and_the_first_one_named(ctx, kzg, honest, where, first):
    k = 4
    params, g2, s_g2 = honest(k)
    arrs = {"g": params._g, "gl": params._gl}
    for which, i in where:
        arrs[which] = bumped(arrs[which], i % 16)
    bad = kzg.ParamsKZG(ctx, k, arrs["g"], arrs["gl"])
    try:
        rep = bad.check(g2, s_g2, seed=3)
    finally:
        bad.free()
    assert rep.ran == G2 | CURVE and rep.failed == CURVE  # the sums over off-curve points mean nothing: not run
    assert (rep.curve_basis, rep.curve_index) == first
    assert not any(rep.points)


def test_the_identity_among_the_bases_fails_curve(ctx, kzg, honest):
    k = 4
    params, g2, s_g2 = honest(k)
    gl = params._gl.copy()
    gl[5] = 0
    bad = kzg.ParamsKZG(ctx, k, params._g, gl)
    try:
        rep = bad.check(g2, s_g2, seed=3)
        only = bad.check(g2, s_g2, seed=3, checks=CURVE)
    finally:
        bad.free()
    assert rep.ran == G2 | CURVE and rep.failed == CURVE and (rep.curve_basis, rep.curve_index) == (1, 5)
    assert only.ran == CURVE and only.failed == CURVE and (only.curve_basis, only.curve_index) == (1, 5)


def test_a_bumped_y_is_off_the_curve_in_python_too(honest):
    params, _, _ = honest(4)
    for arr in (params._g, params._gl):
        for i in (0, 15):
            x, y = zu.point_to_ints(bumped(arr, i)[i])
            assert (y * y - x * x * x - 3) % zu.Q != 0
            x, y = zu.point_to_ints(arr[i])
            assert (y * y - x * x * x - 3) % zu.Q == 0


# ------------------------------------------------------------------------------------ G2
def outside_subgroup_point(kzg):
    for x, res in small_x_candidates():
        if res:
            q = X.g2_from_words(kzg.g2_from_bytes(ref_encode((x, (0, 0)))))
            if X.g2_mul(q, X.R) is not None:
                return np.array(X.g2_words(q), dtype=np.uint64)
    raise AssertionError("no small x gives a point outside G2")


def test_bad_g2_points_are_reported_and_nothing_is_paired_with_them(kzg, honest):
    params, g2, s_g2 = honest(3)
    (x0, x1), (y0, y1) = X.G2_GEN
    off_twist = np.array(X.g2_words(((x0, x1), ((y0 + 1) % X.P, y1))), dtype=np.uint64)
    for bad, status in ((np.zeros(16, np.uint64), 3), (outside_subgroup_point(kzg), 4), (off_twist, 2)):
        assert kzg.g2_check(bad) == status
        for args, want in (((bad, s_g2), [status, 0]), ((g2, bad), [0, status])):
            rep = params.check(*args, seed=9)
            assert list(rep.g2_status) == want
            assert rep.ran == G2 | CURVE and rep.failed == G2
            rep = params.check(*args, seed=9, checks=POWERS | LAGRANGE)  # G2 not asked for: still nothing to pair with
            assert rep.ran == 0 and rep.failed == 0 and list(rep.g2_status) == want


# ------------------------------------------------------------------------------------ residency and refusals
def test_checks_that_read_a_missing_basis_are_not_run(ctx, kzg, honest, logs):
    k = 3
    params, g2, s_g2 = honest(k)
    only_g = kzg.ParamsKZG(ctx, k, params._g, None)
    only_gl = kzg.ParamsKZG(ctx, k, None, params._gl)
    try:
        a, b = only_g.check(g2, s_g2, rho=zu.fr_from_int(RHO)), only_gl.check(g2, s_g2, rho=zu.fr_from_int(RHO))
        gl = bumped(params._gl, 6)
        only_bad_gl = kzg.ParamsKZG(ctx, k, None, gl)
        try:
            c = only_bad_gl.check(g2, s_g2, seed=1)
        finally:
            only_bad_gl.free()
    finally:
        only_g.free()
        only_gl.free()
    assert a.ran == G2 | CURVE | POWERS and a.failed == 0
    want = SR.expected(logs(k)[0], None, S1, RHO, k)
    assert report_points(a)[:2] == [SR.point(v) for v in want["logs"][:2]]
    assert b.ran == G2 | CURVE and b.failed == 0
    assert c.ran == G2 | CURVE and c.failed == CURVE and (c.curve_basis, c.curve_index) == (1, 6)


def test_refusals_leave_the_ctx_usable(ctx, pkg, kzg, honest):
    params, g2, s_g2 = honest(3)
    L, ffi = ctx.L, pkg.ffi
    rep = ffi.SrsReport()
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(srs, a, b, opts, r):
        rc = L.amdzk_srs_check(ctx.h, srs, a, b, None if opts is None else C.byref(opts), r)
        msg = L.amdzk_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("srs_check:"), (rc, msg)
        return msg

    refused(None, p(g2), p(s_g2), None, C.byref(rep))
    refused(params.h, None, p(s_g2), None, C.byref(rep))
    refused(params.h, p(g2), None, None, C.byref(rep))
    refused(params.h, p(g2), p(s_g2), None, None)
    size = C.sizeof(ffi.SrsCheckOpts)
    assert "size" in refused(params.h, p(g2), p(s_g2), ffi.SrsCheckOpts(size - 1, 0, 0, None), C.byref(rep))
    assert "size" in refused(params.h, p(g2), p(s_g2), ffi.SrsCheckOpts(0, 0, 0, None), C.byref(rep))
    assert "unknown check bits" in refused(params.h, p(g2), p(s_g2), ffi.SrsCheckOpts(size, 16, 0, None), C.byref(rep))
    assert "unknown check bits" in refused(params.h, p(g2), p(s_g2), ffi.SrsCheckOpts(size, ALL | 1 << 31, 0, None), C.byref(rep))
    for big in (SR.R, 2**256 - 1):
        rho = np.array(zu.limbs(big), dtype=np.uint64)
        assert "rho" in refused(params.h, p(g2), p(s_g2), ffi.SrsCheckOpts(size, 0, 0, rho.ctypes.data), C.byref(rep))
    assert L.amdzk_srs_check(None, params.h, p(g2), p(s_g2), None, C.byref(rep)) == -2
    # NULL options: all checks, seed 0
    assert L.amdzk_srs_check(ctx.h, params.h, p(g2), p(s_g2), None, C.byref(rep)) == 0
    assert bytes(rep) == bytes(params.check(g2, s_g2, seed=0)) and clean(rep)
    # one check alone, and the largest rho
    assert clean(params.check(g2, s_g2, seed=4, checks=G2), G2)
    assert clean(params.check(g2, s_g2, seed=4, checks=CURVE | POWERS), CURVE | POWERS)
    assert clean(params.check(g2, s_g2, rho=np.array(zu.limbs((SR.R - 1) * zu.MONT % SR.R), dtype=np.uint64)))
    lone = params.check(g2, s_g2, seed=4, checks=LAGRANGE)  # sound only given POWERS, which was not asked for
    assert lone.ran == 0 and lone.failed == 0


# ------------------------------------------------------------------------------------ the hole, closed
def test_a_process_with_an_srs_file_and_nothing_else_decides_proofs(ctx, pkg, kzg, oracle):
    import verify_cases as VC
    plonk = __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])
    c = VC.circuit(plonk, "lookup")
    assert c.k == 5
    s = zu.fr_from_int(S1)
    made = kzg.ParamsKZG.setup(ctx, c.k, s)
    g2, s_g2 = kzg.g2_setup(ctx, s)
    data = made.write(kzg.g2_to_bytes(g2), kzg.g2_to_bytes(s_g2))
    bare = made.write()  # the default: zero fields
    made.free()
    del g2, s_g2

    params, g2_bytes, s_g2_bytes = kzg.ParamsKZG.read(ctx, data)
    vparams = kzg.ParamsVerifierKZG.from_bytes(ctx, g2_bytes, s_g2_bytes)
    pk = d_adv = None
    try:
        assert clean(params.check(*vparams.points))
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(77))
        adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
        d_adv = ctx.alloc(adv.nbytes).upload(adv)
        inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
        proof = plonk.create_proof(ctx, pk, inst, d_adv, seed=3)
        assert plonk.decide_proof(ctx, pk, vparams, inst, proof) is True
        for off in (0, len(proof) // 2, len(proof) - 1):
            m = bytearray(proof)
            m[off] ^= 1
            assert plonk.decide_proof(ctx, pk, vparams, inst, bytes(m)) is False
    finally:
        vparams.free()
        if d_adv is not None:
            d_adv.free()
        if pk is not None:
            pk.free()
        params.free()

    params, g2_bytes, s_g2_bytes = kzg.ParamsKZG.read(ctx, bare)
    params.free()
    assert g2_bytes == s_g2_bytes == bytes(64)
    with pytest.raises(pkg.AmdzkError) as e:
        kzg.ParamsVerifierKZG.from_bytes(ctx, g2_bytes, s_g2_bytes)
    assert "identity" in str(e.value)
