"""GPU: the stand-alone opening calls — amdzk_multiopen_dev, amdzk_multiopen_verify, amdzk_multiopen_decide — at degenerate
challenges, points and polynomials. The challenges and the opening points of these calls are the caller's inputs:
tests/scripted_transcript.py replaces squeezes of the oracle's transcript (SHPLONK: 0 y, 1 v, 2 u; GWC: 0 v and, on the
reader only, 1 u), tests/multiopen_cases.py adds the point set {0, 1, r - 1, omega, omega^32, z, -z}, the polynomials
(a constant, upper half zero, X^(n-1), zero, a root at the query point) and a first set with a private point. The prover is
held to the oracle's shplonk_prove / gwc_prove under the same script — written points, transcript bytes, next challenge — and
the verifier to tests/opening_verify_ref.py; amdzk_multiopen_decide says 1. u on a point outside the first set, a point or
an evaluation or a squeezed challenge that is not below r: refusals, each with the ctx used again. All comparisons exact."""
import os
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
import scripted_transcript as ST  # noqa: E402
from multiopen_cases import TAU, make_case  # noqa: E402
from test_gpu_multiopen import Forwarded, run_device  # noqa: E402
from test_gpu_multiopen_verify import G, Reading, ints, words  # noqa: E402

pytestmark = pytest.mark.gpu
E_INVALID, E_UNSUPPORTED, R = -2, -5, zu.R
RAW_R = np.array(zu.limbs(R), dtype=np.uint64)
RAW_MAX = np.array([2**64 - 1] * 4, dtype=np.uint64)
U_TEXT = "multiopen: the challenge u is one of the opening points (probability 2^-254)"
# the prover's script per name: SHPLONK squeezes y, v, u; GWC squeezes v (and the reader u)
SHPLONK_SCRIPTS = {"y=0": {0: 0}, "v=0": {1: 0}, "y=v=0": {0: 0, 1: 0}, "y=v=1": {0: 1, 1: 1}, "y=v=r-1": {0: R - 1, 1: R - 1}, "u=0": {2: 0}}
GWC_SCRIPTS = {"v=0": {0: 0}, "v=1": {0: 1}, "v=r-1": {0: R - 1}, "u=0": {1: 0}, "v=u=0": {0: 0, 1: 0}}
_params, _cases, _proved = {}, {}, {}


@pytest.fixture(scope="module")
def params_of(ctx, pkg):
    def get(k):
        if k not in _params:
            _params[k] = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(TAU))
        return _params[k]
    yield get
    for p in _params.values():
        p.free()
    _params.clear()


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
    yield v
    v.free()


def case_of(name):
    if name not in _cases:
        c = make_case(name)
        coms = [PR.commit_tau(p, TAU) for p in c.polys]
        evals = [P.eval_polynomial(c.polys[p], c.point_vals[z]) for p, z in c.queries]
        _cases[name] = (c, coms, evals)
    return _cases[name]


def flag(pkg, scheme):
    return pkg.kzg.MULTIOPEN_GWC if scheme == "gwc" else pkg.kzg.MULTIOPEN_SHPLONK


def prover_script(scheme, sc):
    """What the prover sees of a script: GWC's u is the reader's squeeze."""
    return sc if scheme == "shplonk" else {i: s for i, s in sc.items() if i == 0}


def oracle_proof(name, scheme, sc):
    """The oracle's (written points, bytes, next challenge) under the script, once per process."""
    key = (name, scheme, tuple(sorted((i, s) for i, s in sc.items())))
    if key not in _proved:
        _proved[key] = case_of(name)[0].oracle(scheme, ST.scripted(PR.Blake2bWrite, prover_script(scheme, sc)))
    return _proved[key]


def check(ctx, pkg, oracle, params_of, vparams, name, scheme, sc, supplied=False):
    """One (case, scheme, script): the prover against the oracle, the verifier against the reference, decide = 1."""
    case, coms, evals = case_of(name)
    want = oracle_proof(name, scheme, sc)
    kw = {"evals": zu.fr_array_from_ints(evals)} if supplied else {}
    got = run_device(ctx, pkg, oracle, params_of(case.k), case, scheme, ST.scripted(PR.Blake2bWrite, prover_script(scheme, sc)), **kw)
    assert got[0] == want[0], "written points"
    assert got[1] == want[1] and got[2] == want[2], "transcript bytes and the next challenge"
    ch, pts = OV.read(scheme, ST.reader("blake2b", sc, want[1]), case.point_vals, case.queries)
    ref = OV.pair(scheme, coms, case.point_vals, case.queries, evals, ch, pts)
    assert OV.holds(ref, TAU), "the reference does not accept the oracle's opening"
    args = (ctx, G, np.stack([words(p) for p in coms]), zu.fr_array_from_ints(case.point_vals), case.queries, zu.fr_array_from_ints(evals))
    T = Reading(ST.reader("blake2b", sc, want[1]))
    pair = pkg.kzg.multiopen_verify(*args, T, flag(pkg, scheme))
    assert (ints(pair[0]), ints(pair[1])) == ref
    assert T.order == ("ccpcp" if scheme == "shplonk" else "c" + "p" * len(pts) + "c") and T.inner.pos == len(want[1])
    assert pkg.kzg.multiopen_verify(*args, Reading(ST.reader("blake2b", sc, want[1])), flag(pkg, scheme), vparams=vparams) is True
    return ch


# ------------------------------------------------------------------------------------ challenges
@pytest.mark.parametrize("scheme,script", [("shplonk", n) for n in SHPLONK_SCRIPTS] + [("gwc", n) for n in GWC_SCRIPTS])
def test_degenerate_challenges_on_the_shared_sets(ctx, pkg, oracle, params_of, vparams, scheme, script):
    sc = (SHPLONK_SCRIPTS if scheme == "shplonk" else GWC_SCRIPTS)[script]
    ch = check(ctx, pkg, oracle, params_of, vparams, "shared", scheme, sc)
    names = ("y", "v", "u") if scheme == "shplonk" else ("v", "u")
    for i, s in sc.items():
        assert ch[i] == s, "the reader squeezed the scripted %s" % names[i]
    assert oracle_proof("shared", scheme, sc)[1] != oracle_proof("shared", scheme, {})[1] or set(sc) == {len(names) - 1} and scheme == "gwc"


def test_the_private_case_has_a_point_in_the_first_set_only():
    case = make_case("private")
    rot_com, super_points = PR.intermediate_sets([(p, case.point_vals[z]) for p, z in case.queries])
    f = case.point_vals[6]
    assert [len(pts) for pts, _ in rot_com] == [3, 3, 5, 1]
    assert f in rot_com[0][0] and all(f not in pts for pts, _ in rot_com[1:])
    shared = make_case("shared")
    rot_com, _ = PR.intermediate_sets([(p, shared.point_vals[z]) for p, z in shared.queries])
    assert [len(pts) for pts, _ in rot_com] == [2, 3, 5, 1]
    assert all(any(p in pts for pts, _ in rot_com[1:]) for p in rot_com[0][0]), '"shared" has no such point'


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_u_on_a_point_of_the_first_set_only_is_legal(ctx, pkg, oracle, params_of, vparams, scheme):
    """z_0(u) is the product over the points OUTSIDE the first set: u on a private point of the first set leaves it non-zero."""
    f = make_case("private").point_vals[6]
    check(ctx, pkg, oracle, params_of, vparams, "private", scheme, {2 if scheme == "shplonk" else 1: f})
    check(ctx, pkg, oracle, params_of, vparams, "private", scheme, {})


# ------------------------------------------------------------------------------------ points and polynomials
@pytest.mark.parametrize("supplied", [False, True], ids=["evals on the device", "evals supplied"])
@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_edge_point_values(ctx, pkg, oracle, params_of, vparams, scheme, supplied):
    case = make_case("edge points")
    v = case.point_vals
    assert v[0] == v[7] == 0 and v[1] == 1 and v[2] == v[4] == R - 1 and pow(v[3], 64, R) == 1 and pow(v[3], 32, R) == R - 1 and (v[5] + v[6]) % R == 0
    assert {z for _, z in case.queries} == set(range(8)), "every index is queried"
    rot_com, _ = PR.intermediate_sets([(p, v[z]) for p, z in case.queries])
    assert [len(pts) for pts, _ in rot_com] == [2, 3, 5, 1]
    check(ctx, pkg, oracle, params_of, vparams, "edge points", scheme, {}, supplied=supplied)


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_edge_polynomials(ctx, pkg, oracle, params_of, vparams, scheme):
    case, coms, evals = case_of("edge polys")
    assert coms[5] is None and not any(case.polys[5]), "the zero polynomial: the verifier takes (0, 0) for it"
    assert all(e == 0 for (p, _), e in zip(case.queries, evals) if p in (5, 6)) and any(case.polys[6])
    assert not any(case.polys[1][32:]) and case.polys[2] == [0] * 63 + [1] and not any(case.polys[0][1:])
    check(ctx, pkg, oracle, params_of, vparams, "edge polys", scheme, {})
    # y = 0 keeps the first polynomial of every set alone (the constant among them); GWC at v = 0 would open the constant alone
    # at a point, whose quotient is zero: the oracle refuses to write the identity there, so GWC gets v = 1
    check(ctx, pkg, oracle, params_of, vparams, "edge polys", scheme, {0: 0} if scheme == "shplonk" else {0: 1})


# ------------------------------------------------------------------------------------ u outside the first set
def test_u_on_a_point_outside_the_first_set(ctx, pkg, oracle, params_of, vparams):
    """The prover refuses (the oracle raises: 1 / z_0(u)); the verifier divides by nothing: its pair is the reference's, whose
    L = z_0(u) h2 is the identity, and decide says 0."""
    case, coms, evals = case_of("shared")
    c_val = case.point_vals[2]  # in {b, c, d} and in the five-point set, not in {a, b}
    sc = {2: c_val}
    with pytest.raises(ValueError):
        case.oracle("shplonk", ST.scripted(PR.Blake2bWrite, sc))
    T = Forwarded(ST.writer("blake2b", sc))
    with pytest.raises(pkg.AmdzkError) as e:
        run_device(ctx, pkg, oracle, params_of(case.k), case, "shplonk", transcript=T)
    assert e.value.code == E_UNSUPPORTED and str(e.value).endswith(U_TEXT)
    honest = oracle_proof("shared", "shplonk", {})
    assert T.writes == 1 and bytes(T.inner.proof) == honest[1][:32]  # h1 was written, u squeezed, nothing behind it
    assert run_device(ctx, pkg, oracle, params_of(case.k), case, "shplonk") == honest
    ch, pts = OV.read("shplonk", ST.reader("blake2b", sc, honest[1]), case.point_vals, case.queries)
    ref = OV.pair("shplonk", coms, case.point_vals, case.queries, evals, ch, pts)
    assert ch[2] == c_val and ref[0] is None and ref[1] is not None
    args = (ctx, G, np.stack([words(p) for p in coms]), zu.fr_array_from_ints(case.point_vals), case.queries, zu.fr_array_from_ints(evals))
    pair = pkg.kzg.multiopen_verify(*args, Reading(ST.reader("blake2b", sc, honest[1])), flag(pkg, "shplonk"))
    assert (ints(pair[0]), ints(pair[1])) == ref
    assert pkg.kzg.multiopen_verify(*args, Reading(ST.reader("blake2b", sc, honest[1])), flag(pkg, "shplonk"), vparams=vparams) is False
    assert pkg.kzg.multiopen_verify(*args, Reading(PR.Blake2bRead(honest[1])), flag(pkg, "shplonk"), vparams=vparams) is True


# ------------------------------------------------------------------------------------ words that are no residues
class Refusing:
    """The "shared" case on the device, and refused(): one amdzk_multiopen_dev call that must be refused with AMDZK_E_INVALID
    and the text, before the transcript is touched unless `calls` is None, with the ctx proving the good case right after."""

    def __init__(self, ctx, pkg, oracle, params_of, scheme):
        self.pkg, self.scheme = pkg, scheme
        self.case, _coms, evals = case_of("shared")
        self.params = params_of(self.case.k)
        self.want = oracle_proof("shared", scheme, {})
        coeffs = np.concatenate([zu.ints_to_fr(oracle, p) for p in self.case.polys])
        self.buf = ctx.alloc(coeffs.nbytes).upload(coeffs)
        self.addrs = [self.buf.ptr.value + i * self.case.n * 32 for i in range(len(self.case.polys))]
        self.good_pts, self.good_ev = zu.fr_array_from_ints(self.case.point_vals), zu.fr_array_from_ints(evals)

    def refused(self, text, points=None, evals=None, transcript=None, calls=0):
        pkg, T = self.pkg, transcript or Forwarded(PR.Blake2bWrite())
        with pytest.raises(pkg.AmdzkError) as e:
            pkg.kzg.multiopen(self.params, self.addrs, self.good_pts if points is None else points, self.case.queries, T, flag(pkg, self.scheme), evals=evals)
        assert e.value.code == E_INVALID and str(e.value).endswith(text), str(e.value)
        assert calls is None or T.calls == calls, "refused before the transcript is touched"
        inner = PR.Blake2bWrite()
        got = pkg.kzg.multiopen(self.params, self.addrs, self.good_pts, self.case.queries, Forwarded(inner), flag(pkg, self.scheme))
        assert [zu.point_to_ints(p) for p in got] == self.want[0] and bytes(inner.proof) == self.want[1]  # the ctx is usable


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_a_point_that_is_not_below_r_is_refused(ctx, pkg, oracle, params_of, scheme):
    rf = Refusing(ctx, pkg, oracle, params_of, scheme)
    try:
        for raw in (RAW_R, RAW_MAX):
            for at in (0, 4, 5):  # queried indices, the last one a second index of a value
                pts = rf.good_pts.copy()
                pts[at] = raw
                rf.refused("multiopen: point %d is not below the modulus" % at, points=pts)
            # an index no query names: a seventh point
            rf.refused("multiopen: point 6 is not below the modulus", points=np.concatenate([rf.good_pts, raw.reshape(1, 4)]))
        # a point and an evaluation: the points are looked at first
        pts, ev = rf.good_pts.copy(), rf.good_ev.copy()
        pts[3], ev[0] = RAW_R, RAW_R
        rf.refused("multiopen: point 3 is not below the modulus", points=pts, evals=ev)
    finally:
        rf.buf.free()


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_a_supplied_evaluation_that_is_not_below_r_is_refused(ctx, pkg, oracle, params_of, scheme):
    rf = Refusing(ctx, pkg, oracle, params_of, scheme)
    try:
        for raw in (RAW_R, RAW_MAX):
            for at in (0, len(rf.case.queries) - 1):
                ev = rf.good_ev.copy()
                ev[at] = raw
                rf.refused("multiopen: evaluation %d is not below the modulus" % at, evals=ev)
    finally:
        rf.buf.free()


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_a_squeezed_challenge_that_is_not_below_r_is_refused(ctx, pkg, oracle, params_of, scheme):
    """Words of r and of 2^256 - 1 at squeeze 0 and at the prover's last squeeze, as amdzk_multiopen_verify refuses them."""
    rf = Refusing(ctx, pkg, oracle, params_of, scheme)
    try:
        for value in (R, (1 << 256) - 1):
            for at in ((0, 2) if scheme == "shplonk" else (0,)):
                T = ST.device_writer("blake2b", {at: ST.Raw(value)})
                rf.refused("multiopen: a squeezed challenge is not below the modulus", transcript=T, calls=None)
                assert T.squeezes == at + 1 and len(T.proof) == (32 if at == 2 else 0)
    finally:
        rf.buf.free()
