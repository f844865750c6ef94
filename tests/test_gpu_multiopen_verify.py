"""GPU: amdzk_multiopen_verify / amdzk_multiopen_decide — the KZG opening argument verified alone over the caller's
commitments and read transcript — against tests/opening_verify_ref.py (Python integers, itself held to the oracle's provers
by tests/test_opening_verify_ref.py): the pair equals the reference as group elements; the verdict is 1 for the oracle's
points and 0 for a wrong evaluation, a wrong commitment, swapped read points and a wrong s_g2; duplicate queries and a second
index for one point value change nothing; amdzk_multiopen_dev followed by amdzk_multiopen_decide round-trips with no oracle
in between; every documented refusal, with the ctx used again after each. The SRS is the test SRS of multiopen_cases.TAU."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import opening_verify_ref as OV  # noqa: E402
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402
from multiopen_cases import TAU, Case, caps_golden, make_case, random_polys  # noqa: E402

pytestmark = pytest.mark.gpu
E_INVALID, Q, R = -2, zu.Q, zu.R
G = zu.point_from_ints(P.G1_GEN)
CASES = [("one", "shplonk"), ("one", "gwc"), ("shared", "shplonk"), ("shared", "gwc"), ("17 sets", "shplonk"), ("17 sets", "gwc"),
         ("17 points", "shplonk"), ("17 points", "gwc"), ("top 10", "shplonk"), ("top 10", "gwc")]
_made = {}


def words(p):
    return np.zeros(8, np.uint64) if p is None else zu.point_from_ints(p)


def ints(w):
    return zu.point_to_ints(w)


class Reading:
    """The oracle's read transcript behind the library's callbacks; fail_at: that call (reads and squeezes counted together)
    returns non-zero; replace: {read index: words}; big_at: that squeeze hands back the modulus."""

    def __init__(self, inner, fail_at=None, replace=None, big_at=None):
        self.inner, self.fail_at, self.replace, self.big_at, self.calls, self.reads, self.order = inner, fail_at, replace or {}, big_at, 0, 0, ""

    def common_point(self, w):
        raise AssertionError("multiopen_verify calls squeeze_challenge and read_point only")

    common_scalar = common_point

    def read_scalar(self):
        raise AssertionError("multiopen_verify calls squeeze_challenge and read_point only")

    def _step(self):
        self.calls += 1
        if self.fail_at == self.calls - 1:
            raise RuntimeError("the caller's transcript fails here")

    def read_point(self):
        self._step()
        self.order += "p"
        w = self.replace.get(self.reads, words(self.inner.read_point()))
        self.reads += 1
        return w

    def squeeze_challenge(self):
        self._step()
        self.order += "c"
        v = zu.fr_from_int(self.inner.squeeze_challenge())
        return np.array(zu.limbs(R), dtype=np.uint64) if self.big_at == self.calls - 1 else v


class Opening:
    """One case as the verifier's arguments, with the reference's pair."""

    def __init__(self, name, scheme):
        self.case, self.scheme = make_case(name), scheme
        self.coms, self.evals, self.proof = OV.opening_of(self.case, scheme, TAU)
        self.ch, self.pts = OV.read(scheme, PR.Blake2bRead(self.proof), self.case.point_vals, self.case.queries)
        self.ref = OV.pair(scheme, self.coms, self.case.point_vals, self.case.queries, self.evals, self.ch, self.pts)
        assert OV.holds(self.ref, TAU)

    def args(self, coms=None, evals=None, queries=None, point_vals=None):
        c = self.case
        return (np.stack([words(p) for p in (self.coms if coms is None else coms)]),
                zu.fr_array_from_ints(c.point_vals if point_vals is None else point_vals),
                c.queries if queries is None else queries, zu.fr_array_from_ints(self.evals if evals is None else evals))


def opening(name, scheme):
    if (name, scheme) not in _made:
        _made[(name, scheme)] = Opening(name, scheme)
    return _made[(name, scheme)]


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
    yield v
    v.free()


def flag(pkg, scheme):
    return pkg.kzg.MULTIOPEN_GWC if scheme == "gwc" else pkg.kzg.MULTIOPEN_SHPLONK


def verify(ctx, pkg, o, transcript=None, vparams=None, **kw):
    coms, points, queries, evals = o.args(**kw)
    T = transcript or Reading(PR.Blake2bRead(o.proof))
    out = pkg.kzg.multiopen_verify(ctx, G, coms, points, queries, evals, T, flag(pkg, o.scheme), vparams=vparams)
    return out if vparams is not None else (ints(out[0]), ints(out[1]))


# ------------------------------------------------------------------------------------ the pair and the verdicts
@pytest.mark.parametrize("name,scheme", CASES)
def test_pair_equals_the_reference_and_only_the_oracles_opening_is_decided_valid(ctx, pkg, vparams, name, scheme):
    o = opening(name, scheme)
    c = o.case
    T = Reading(PR.Blake2bRead(o.proof))
    assert verify(ctx, pkg, o, T) == o.ref
    assert T.order == ("ccpcp" if scheme == "shplonk" else "c" + "p" * len(o.pts) + "c") and T.inner.pos == len(o.proof)
    assert verify(ctx, pkg, o, vparams=vparams) is True
    # a wrong evaluation (query 0 is the first of its pair: both schemes read it), a wrong commitment, swapped read points
    ev = list(o.evals)
    ev[0] = (ev[0] + 1) % R
    assert verify(ctx, pkg, o, evals=ev) == OV.pair(scheme, o.coms, c.point_vals, c.queries, ev, o.ch, o.pts)
    assert verify(ctx, pkg, o, vparams=vparams, evals=ev) is False
    cm = list(o.coms)
    cm[c.queries[0][0]] = P.g1_add(cm[c.queries[0][0]], P.G1_GEN)
    assert verify(ctx, pkg, o, vparams=vparams, coms=cm) is False
    if len(o.pts) > 1 and o.pts[0] != o.pts[1]:
        swapped = Reading(PR.Blake2bRead(o.proof), replace={0: words(o.pts[1]), 1: words(o.pts[0])})
        assert verify(ctx, pkg, o, swapped, vparams=vparams) is False
    # a wrong s_g2: the pairing, not the sums, says no
    other = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU + 1))
    try:
        assert verify(ctx, pkg, o, vparams=other) is False
    finally:
        other.free()
    ctx.check_affinity()


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_duplicate_queries_and_two_indices_for_one_value_change_nothing(ctx, pkg, vparams, scheme):
    o = opening("shared", scheme)
    c = o.case
    assert c.point_vals[5] == c.point_vals[1] and len(set(c.queries)) < len(c.queries)
    # the second index of a value renamed to the first ...
    renamed = [(p, 1 if z == 5 else z) for p, z in c.queries]
    assert verify(ctx, pkg, o, queries=renamed) == o.ref
    # ... and every duplicate of a (commitment, point value) pair dropped
    seen, kept, kept_ev = set(), [], []
    for (p, z), e in zip(renamed, o.evals):
        if (p, z) not in seen:
            seen.add((p, z))
            kept.append((p, z))
            kept_ev.append(e)
    assert len(kept) < len(c.queries)
    if scheme == "shplonk":  # GWC folds every query: fewer queries are another opening
        assert verify(ctx, pkg, o, queries=kept, evals=kept_ev) == o.ref
    # a duplicate query that claims another evaluation: SHPLONK reads the first of a pair, GWC every query's own
    dup = max(i for i, q in enumerate(c.queries) if c.queries.index(q) < i)
    ev = list(o.evals)
    ev[dup] = (ev[dup] + 1) % R
    assert verify(ctx, pkg, o, vparams=vparams, evals=ev) is (scheme == "shplonk")
    assert verify(ctx, pkg, o, evals=ev) == OV.pair(scheme, o.coms, c.point_vals, c.queries, ev, o.ch, o.pts)


def test_three_thousand_points_are_no_cap(ctx, pkg, vparams):
    """GWC over 3000 distinct points and 9000 queries: the oracle's recorded points (tests/golden/multiopen_caps_gwc.bin) are
    decided valid, and one wrong evaluation among the 9000 is not. (The pair's reference would take the pure-Python group
    arithmetic most of a minute; the 17-point case above pins the pair.)"""
    case = make_case("caps")
    proof, _next = caps_golden()
    coms = np.stack([words(PR.commit_tau(p, TAU)) for p in case.polys])
    evals = [P.eval_polynomial(case.polys[p], case.point_vals[z]) for p, z in case.queries]
    pts = zu.fr_array_from_ints(case.point_vals)
    run = lambda ev: pkg.kzg.multiopen_verify(ctx, G, coms, pts, case.queries, zu.fr_array_from_ints(ev), Reading(PR.Blake2bRead(proof)),
                                              pkg.kzg.MULTIOPEN_GWC, vparams=vparams)
    assert run(evals) is True
    evals[4321] = (evals[4321] + 1) % R
    assert run(evals) is False


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_an_identity_commitment_is_allowed(ctx, pkg, vparams, scheme):
    case = make_case("shared")
    case.polys[2] = [0] * case.n
    o = Opening.__new__(Opening)
    o.case, o.scheme = case, scheme
    o.coms, o.evals, o.proof = OV.opening_of(case, scheme, TAU)
    assert o.coms[2] is None
    o.ch, o.pts = OV.read(scheme, PR.Blake2bRead(o.proof), case.point_vals, case.queries)
    o.ref = OV.pair(scheme, o.coms, case.point_vals, case.queries, o.evals, o.ch, o.pts)
    assert verify(ctx, pkg, o) == o.ref and verify(ctx, pkg, o, vparams=vparams) is True


@pytest.mark.parametrize("nb", [63, 64, 65])
def test_the_points_check_around_one_block_of_64(ctx, pkg, vparams, nb):
    """The check launch takes commitments | read points | g, one thread each in blocks of 64: nb = 63, 64 and 65 points in
    all (SHPLONK reads two points: nb - 3 commitments, each opened at one point). The LAST commitment is the identity, the
    last index below which it is allowed, and the opening holds; the identity one index on — read point 0 — is refused; and
    when the only bad point is the last read point or g, the last of all at index nb - 1 = 62, 63, 64 (in a block of its own
    for 65), the refusal names it. (The one other case of this file that is sure to cross 64 points, the 3000 of the caps case,
    is an accepted opening: no test had a bad point beyond index 63.)"""
    n_coms = nb - 3
    rng = random.Random("points check %d" % nb)
    case = Case(2, random_polys(rng, n_coms, 4), [rng.randrange(R)], [(i, 0) for i in range(n_coms)])
    case.polys[n_coms - 1] = [0] * case.n
    o = Opening.__new__(Opening)
    o.case, o.scheme = case, "shplonk"
    o.coms, o.evals, o.proof = OV.opening_of(case, "shplonk", TAU)
    assert o.coms[n_coms - 1] is None and all(c is not None for c in o.coms[:-1])
    o.ch, o.pts = OV.read("shplonk", PR.Blake2bRead(o.proof), case.point_vals, case.queries)
    assert len(o.coms) + len(o.pts) + 1 == nb
    o.ref = OV.pair("shplonk", o.coms, case.point_vals, case.queries, o.evals, o.ch, o.pts)
    assert verify(ctx, pkg, o) == o.ref and verify(ctx, pkg, o, vparams=vparams) is True

    def refused(expect, transcript=None, g=G):
        coms, points, queries, evals = o.args()
        with pytest.raises(pkg.ffi.AmdzkError) as e:
            pkg.kzg.multiopen_verify(ctx, g, coms, points, queries, evals, transcript or Reading(PR.Blake2bRead(o.proof)), flag(pkg, "shplonk"))
        assert e.value.code == E_INVALID and expect in str(e.value), e.value
        assert verify(ctx, pkg, o) == o.ref  # the ctx is used again

    refused("multiopen_verify: read point 0 ", Reading(PR.Blake2bRead(o.proof), replace={0: np.zeros(8, np.uint64)}))
    off_curve = lambda p: words((p[0], (p[1] + 1) % Q))
    refused("multiopen_verify: read point 1 ", Reading(PR.Blake2bRead(o.proof), replace={1: off_curve(o.pts[1])}))  # index nb - 2
    refused("multiopen_verify: g has ", g=off_curve(P.G1_GEN))  # index nb - 1
    refused("multiopen_verify: g has ", g=np.zeros(8, np.uint64))


# ------------------------------------------------------------------------------------ prove, then verify: no oracle between
class Written:
    """A write transcript of the test's own (Blake2b under another personalisation), in Montgomery words throughout."""

    def __init__(self):
        self.inner, self.points = PR.Blake2bWrite(), []
        import hashlib
        self.inner.state = hashlib.blake2b(digest_size=64, person=b"amdzk-roundtrip!")

    def common_point(self, *a):
        raise AssertionError("the opening argument calls squeeze_challenge and write_point / read_point only")

    common_scalar = write_scalar = read_scalar = common_point

    def write_point(self, w):
        self.points.append(np.array(w, dtype=np.uint64))
        self.inner.common_point(ints(w))

    def squeeze_challenge(self):
        return zu.fr_from_int(self.inner.squeeze_challenge())


class ReadBack(Written):
    """Its read side: hands back the points that were written, absorbing them the same way."""

    def __init__(self, points):
        super().__init__()
        self.queue = list(points)

    def read_point(self):
        w = self.queue.pop(0)
        self.inner.common_point(ints(w))
        return w


@pytest.mark.parametrize("name,scheme", [("shared", "shplonk"), ("shared", "gwc"), ("17 points", "gwc"), ("17 sets", "shplonk")])
def test_multiopen_dev_then_multiopen_decide_round_trips(ctx, pkg, oracle, vparams, name, scheme):
    case = make_case(name)
    params = pkg.kzg.ParamsKZG.setup(ctx, case.k, zu.fr_from_int(TAU))
    coeffs = np.concatenate([zu.ints_to_fr(oracle, p) for p in case.polys])
    buf = ctx.alloc(coeffs.nbytes).upload(coeffs)
    try:
        addrs = [buf.ptr.value + i * case.n * 32 for i in range(len(case.polys))]
        pts = zu.fr_array_from_ints(case.point_vals)
        W = Written()
        written = pkg.kzg.multiopen(params, addrs, pts, case.queries, W, flag(pkg, scheme))
        assert len(written) == len(W.points)
        coms = np.stack([zu.jac_to_affine_host(oracle, params.commit(zu.ints_to_fr(oracle, p))) for p in case.polys])
        evals = np.zeros((len(case.queries), 4), np.uint64)
        for i, (p, z) in enumerate(case.queries):
            one = np.zeros(4, np.uint64)
            ctx._chk(ctx.L.amdzk_eval_poly_dev(ctx.h, (C.c_void_p * 1)(addrs[p]), pts[z].ctypes.data, 1, case.n, one.ctypes.data))
            evals[i] = one
        g = params.get_g()[0]
        Rd = ReadBack(W.points)
        assert pkg.kzg.multiopen_verify(ctx, g, coms, pts, case.queries, evals, Rd, flag(pkg, scheme), vparams=vparams) is True
        if scheme == "gwc":
            W.inner.squeeze_challenge()  # GWC's verifier squeezes u behind the last point; its prover has no use for it
        assert Rd.queue == [] and Rd.inner.squeeze_challenge() == W.inner.squeeze_challenge()
        evals[0] = zu.fr_from_int((zu.fr_to_int(evals[0]) + 1) % R)
        assert pkg.kzg.multiopen_verify(ctx, g, coms, pts, case.queries, evals, ReadBack(W.points), flag(pkg, scheme), vparams=vparams) is False
    finally:
        buf.free()
        params.free()


def test_python_verifier_classes_index_commitments_and_points(ctx, pkg, vparams):
    for scheme, cls in (("shplonk", pkg.kzg.VerifierSHPLONK), ("gwc", pkg.kzg.VerifierGWC)):
        o = opening("shared", scheme)
        c = o.case
        qs = [(words(o.coms[p]), zu.fr_from_int(c.point_vals[z]), zu.fr_from_int(e)) for (p, z), e in zip(c.queries, o.evals)]
        v = cls(ctx, G)
        lhs, rhs = v.verify_proof(Reading(PR.Blake2bRead(o.proof)), qs)
        assert (ints(lhs), ints(rhs)) == o.ref
        assert v.decide(Reading(PR.Blake2bRead(o.proof)), qs, vparams) is True


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_refusals_start_with_multiopen_verify_and_leave_the_ctx_usable(ctx, pkg, vparams, scheme):
    o = opening("shared", scheme)
    c = o.case
    coms, points, queries, evals = o.args()
    q = np.array(queries, dtype=pkg.ffi.OPEN_QUERY)
    n_calls = 5 if scheme == "shplonk" else len(o.pts) + 2

    def call(expect=None, code=E_INVALID, transcript="default", decide=False, **kw):
        a = dict(g=G, commitments=coms, points=points, queries=q, evals=evals, scheme=flag(pkg, scheme), opts_size=None)
        a.update(kw)
        T = Reading(PR.Blake2bRead(o.proof)) if transcript == "default" else transcript
        try:
            out = pkg.kzg.multiopen_verify(ctx, a["g"], a["commitments"], a["points"], a["queries"], a["evals"], T, a["scheme"],
                                           vparams=vparams if decide else None, opts_size=a["opts_size"])
        except pkg.ffi.AmdzkError as e:
            assert expect is not None, e
            assert e.code == code and str(e).split(": ", 1)[1].startswith("multiopen_verify:") and expect in str(e), e
            # the ctx is used again after every refusal
            assert verify(ctx, pkg, o) == o.ref
            return None
        assert expect is None, "not refused: %s" % expect
        return out

    assert call() is not None
    for null in ("g", "commitments", "points", "queries", "evals"):
        call("null argument", **{null: None})
    call("a transcript is required", transcript=None)
    call("opts.size", opts_size=8)

    class NoSqueeze(Reading):
        squeeze_challenge = None
    call("null member", transcript=NoSqueeze(PR.Blake2bRead(o.proof)))
    call("no queries", queries=q[:0], evals=evals[:0])
    bad_q = q.copy()
    bad_q[3]["poly"] = len(coms)
    call("query 3", queries=bad_q)
    bad_q = q.copy()
    bad_q[4]["point"] = len(points)
    call("query 4", queries=bad_q)
    call("unknown scheme", scheme=0x200)
    big = np.array(zu.limbs(R), dtype=np.uint64)
    bad = evals.copy()
    bad[7] = big
    call("evaluation 7", evals=bad)
    bad = points.copy()
    bad[2] = big
    call("point 2", points=bad)
    # a commitment / a read point / g that fails its check: the message names which
    bad = coms.copy()
    bad[3] = words((o.coms[3][0], (o.coms[3][1] + 1) % Q))
    call("commitment 3", commitments=bad)
    bad = coms.copy()
    bad[1][:4] = np.array(zu.limbs(Q), dtype=np.uint64)
    call("commitment 1", commitments=bad)
    last = len(o.pts) - 1
    call("read point %d" % last, transcript=Reading(PR.Blake2bRead(o.proof), replace={last: words((o.pts[last][0], (o.pts[last][1] + 1) % Q))}))
    call("read point 0", transcript=Reading(PR.Blake2bRead(o.proof), replace={0: np.zeros(8, np.uint64)}))  # the identity may not be read
    call("multiopen_verify: g ", g=np.zeros(8, np.uint64))
    # every callback of the read order returning non-zero, and a challenge that is not below r
    for i in range(n_calls):
        T = Reading(PR.Blake2bRead(o.proof), fail_at=i)
        with pytest.raises(RuntimeError, match="fails here"):  # the Python mirror re-raises what the callback raised
            call("unreachable", transcript=T)
        assert T.calls == i + 1
        assert ctx.L.amdzk_last_error(ctx.h).decode() == "multiopen_verify: the caller's transcript reported an error"
        assert verify(ctx, pkg, o) == o.ref
    first_squeeze, last_squeeze = 0, n_calls - 1 if scheme == "gwc" else 3
    for i in (first_squeeze, last_squeeze):
        call("challenge is not below the modulus", transcript=Reading(PR.Blake2bRead(o.proof), big_at=i))

    # decide: its own null arguments
    L = ctx.L
    errors = []
    tr, keep = pkg.ffi.read_transcript(Reading(PR.Blake2bRead(o.proof)), errors)
    opts = pkg.ffi.MultiopenVerifyOpts(C.sizeof(pkg.ffi.MultiopenVerifyOpts), flag(pkg, scheme), C.pointer(tr))
    verdict = C.c_uint8(7)
    base = (ctx.h, G.ctypes.data, coms.ctypes.data, len(coms), points.ctypes.data, len(points), q.ctypes.data, evals.ctypes.data, len(q), C.byref(opts))
    for s_g2, g2, out in ((None, vparams.g2.h, C.byref(verdict)), (vparams.s_g2.h, None, C.byref(verdict)), (vparams.s_g2.h, vparams.g2.h, None)):
        assert L.amdzk_multiopen_decide(*base, s_g2, g2, out) == E_INVALID
        assert L.amdzk_last_error(ctx.h).decode().startswith("multiopen_verify: null argument")
    assert L.amdzk_multiopen_verify(*base, None) == E_INVALID and L.amdzk_last_error(ctx.h).decode().startswith("multiopen_verify: null argument")
    assert L.amdzk_multiopen_verify(ctx.h, *base[1:-1], None, np.zeros(16, np.uint64).ctypes.data) == E_INVALID
    assert L.amdzk_multiopen_decide(*base, vparams.s_g2.h, vparams.g2.h, C.byref(verdict)) == 0 and verdict.value == 1 and errors == []
    del keep


def test_the_status_words_limit_is_refused_before_anything_is_read(ctx, pkg):
    """2^30 commitments and points is where the check launch's status word ends: refused before any array is touched (the
    commitments array here has one entry). Below it the only limit is memory — AMDZK_E_NOMEM, which a test cannot reach
    without hundreds of GiB of host arrays."""
    coms = np.zeros((1, 8), np.uint64)
    q = np.zeros(1, dtype=pkg.ffi.OPEN_QUERY)
    errors = []
    tr, keep = pkg.ffi.read_transcript(Reading(PR.Blake2bRead(b"")), errors)
    opts = pkg.ffi.MultiopenVerifyOpts(C.sizeof(pkg.ffi.MultiopenVerifyOpts), 0, C.pointer(tr))
    pair = np.zeros(16, np.uint64)
    one = zu.fr_from_int(1)
    rc = ctx.L.amdzk_multiopen_verify(ctx.h, G.ctypes.data, coms.ctypes.data, 1 << 30, one.ctypes.data, 1, q.ctypes.data, one.ctypes.data, 1,
                                      C.byref(opts), pair.ctypes.data)
    assert rc == E_INVALID and ctx.L.amdzk_last_error(ctx.h).decode().startswith("multiopen_verify: more than 2^30")
    del keep
