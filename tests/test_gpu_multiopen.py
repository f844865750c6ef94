"""GPU: amdzk_multiopen_dev — SHPLONK and GWC over caller polynomials, points and transcript — against the protocol
oracle's shplonk_prove / gwc_prove (oracle/plonk_ref.py) run on an identically fresh transcript: the written points, the
transcript's bytes and its state afterwards must be equal. The SRS is amdzk_srs_setup(k, tau) with the oracle's tau.
Sizes are the smallest that reach each path of the stand-alone call; the composed kernels' own boundaries (segments of
2^16 coefficients, scan tiles) are test_gpu_plonk_ops.py's."""
import hashlib
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import circuits  # noqa: E402
import plonk_ref as PR  # noqa: E402
from multiopen_cases import TAU, caps_golden, make_case  # noqa: E402

pytestmark = pytest.mark.gpu
E_INVALID = -2


class Forwarded:
    """The oracle's transcript writer fed only through the library's callbacks (Montgomery words in, ints inside)."""

    def __init__(self, inner, fail_write_at=None):
        self.inner, self.calls, self.fail_write_at, self.writes = inner, 0, fail_write_at, 0

    def common_point(self, w):
        raise AssertionError("multiopen calls squeeze_challenge and write_point only")

    common_scalar = write_scalar = common_point

    def write_point(self, w):
        self.calls += 1
        self.writes += 1
        if self.fail_write_at == self.writes:
            return 1
        self.inner.write_point((zu.fq_to_int(w[:4]), zu.fq_to_int(w[4:8])))

    def squeeze_challenge(self):
        self.calls += 1
        return zu.fr_from_int(self.inner.squeeze_challenge())


_params = {}


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


def run_device(ctx, pkg, oracle, params, case, scheme, transcript_cls=PR.Blake2bWrite, transcript=None, zero_polys=False, **kw):
    """The case through kzg.multiopen on one upload of all polynomials. Returns (points as ints, bytes, next challenge)."""
    coeffs = np.concatenate([zu.ints_to_fr(oracle, [0] * case.n if zero_polys else p) for p in case.polys])
    buf = ctx.alloc(coeffs.nbytes).upload(coeffs)
    try:
        inner = transcript_cls()
        T = transcript or Forwarded(inner)
        addrs = [buf.ptr.value + i * case.n * 32 for i in range(len(case.polys))]
        got = pkg.kzg.multiopen(params, addrs, zu.fr_array_from_ints(case.point_vals), case.queries, T,
                                pkg.kzg.MULTIOPEN_GWC if scheme == "gwc" else pkg.kzg.MULTIOPEN_SHPLONK, **kw)
    finally:
        buf.free()
    if isinstance(got, int):
        return got, bytes(inner.proof), inner.squeeze_challenge()
    return [zu.point_to_ints(p) for p in got], bytes(inner.proof), inner.squeeze_challenge()


_oracle_cache = {}


def oracle_of(name, scheme, transcript_cls=PR.Blake2bWrite):
    key = (name, scheme, transcript_cls.__name__)
    if key not in _oracle_cache:
        _oracle_cache[key] = make_case(name).oracle(scheme, transcript_cls)
    return _oracle_cache[key]


CASES = [("one", "shplonk"), ("one", "gwc"), ("shared", "shplonk"), ("shared", "gwc"), ("17 sets", "shplonk"), ("17 points", "gwc"),
         ("caps", "gwc"), ("top 10", "shplonk"), ("top 10", "gwc"), ("top 12", "shplonk"), ("top 12", "gwc")]


@pytest.mark.parametrize("name,scheme", CASES)
def test_points_and_transcript_equal_oracle(ctx, pkg, oracle, params_of, name, scheme):
    case = make_case(name)
    if name == "caps" and not os.environ.get("AMDZK_TEST_FULL_ORACLE"):
        # 3000 pure-Python commitments take the oracle most of a minute: its output is a record (multiopen_cases.py),
        # a sample of which test_multiopen_golden.py re-derives live. A compressed point names one point.
        proof, nxt = caps_golden()
        got = run_device(ctx, pkg, oracle, params_of(case.k), case, scheme)
        assert len(got[0]) == 3000 and b"".join(PR.g1_compress(p) for p in got[0]) == proof
        assert got[1] == proof and got[2] == nxt
        return
    want = oracle_of(name, scheme)
    plan = pkg.kzg.multiopen_plan(zu.fr_array_from_ints(case.point_vals), case.queries, len(case.polys), case.k,
                                  pkg.kzg.MULTIOPEN_GWC if scheme == "gwc" else pkg.kzg.MULTIOPEN_SHPLONK)
    if name == "17 sets":
        assert plan["n_sets"] == 17
    if name in ("17 points", "caps"):
        assert plan["n_out"] == len(case.point_vals) > 16
    got = run_device(ctx, pkg, oracle, params_of(case.k), case, scheme)
    assert len(got[0]) == plan["n_out"] == len(want[0])
    assert got[0] == want[0]
    assert got[1] == want[1] and got[2] == want[2]
    ctx.check_affinity()


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_keccak_transcript(ctx, pkg, oracle, params_of, scheme):
    case = make_case("shared")
    assert run_device(ctx, pkg, oracle, params_of(case.k), case, scheme, PR.Keccak256Write) == oracle_of("shared", scheme, PR.Keccak256Write)


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_python_prover_classes_index_buffers_and_points(ctx, pkg, oracle, params_of, scheme):
    """ProverSHPLONK / ProverGWC(params).create_proof(transcript, [(buffer, point)]): buffers by address, points by value."""
    case = make_case("shared")
    bufs = [ctx.alloc(case.n * 32).upload(zu.ints_to_fr(oracle, p)) for p in case.polys]
    inner = PR.Blake2bWrite()
    prover = (pkg.kzg.ProverGWC if scheme == "gwc" else pkg.kzg.ProverSHPLONK)(params_of(case.k))
    got = prover.create_proof(Forwarded(inner), [(bufs[p], zu.fr_from_int(case.point_vals[z])) for p, z in case.queries])
    for b in bufs:
        b.free()
    want = oracle_of("shared", scheme)
    assert [zu.point_to_ints(p) for p in got] == want[0] and bytes(inner.proof) == want[1]


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_supplied_evaluations_and_output_arguments(ctx, pkg, oracle, params_of, scheme):
    case = make_case("shared")
    params = params_of(case.k)
    want = oracle_of("shared", scheme)
    evals = zu.fr_array_from_ints([int(PR.P.eval_polynomial(case.polys[p], case.point_vals[z])) for p, z in case.queries])
    assert run_device(ctx, pkg, oracle, params, case, scheme, evals=evals) == want
    # supplied evaluations are trusted, not checked: a wrong one raises nothing. It does not change the points either —
    # it moves R_i (the constant, for GWC) and every division drops its remainder, as upstream's kate_division does; the
    # claimed value reaches the verifier through what the caller wrote to the transcript, not through this call.
    bad = evals.copy()
    bad[0] = zu.fr_from_int(zu.fr_to_int(bad[0]) + 1)
    assert run_device(ctx, pkg, oracle, params, case, scheme, evals=bad) == want
    # out_points = NULL: the count comes back, the transcript has everything
    n_out, proof, nxt = run_device(ctx, pkg, oracle, params, case, scheme, want_points=False)
    assert n_out == len(want[0]) and (proof, nxt) == want[1:]
    # too little room for the points: refused before the transcript is touched
    T = Forwarded(PR.Blake2bWrite())
    with pytest.raises(pkg.AmdzkError) as e:
        run_device(ctx, pkg, oracle, params, case, scheme, transcript=T, out_cap=len(want[0]) - 1)
    assert e.value.code == E_INVALID and "multiopen:" in str(e.value) and T.calls == 0
    assert run_device(ctx, pkg, oracle, params, case, scheme) == want


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_identity_commitment_is_refused_and_the_ctx_stays_usable(ctx, pkg, oracle, params_of, scheme):
    case = make_case("shared")
    params = params_of(case.k)
    with pytest.raises(pkg.AmdzkError) as e:
        run_device(ctx, pkg, oracle, params, case, scheme, zero_polys=True)
    assert e.value.code == E_INVALID and "multiopen:" in str(e.value) and "identity" in str(e.value)
    assert run_device(ctx, pkg, oracle, params, case, scheme) == oracle_of("shared", scheme)


@pytest.mark.parametrize("scheme", ["shplonk", "gwc"])
def test_transcript_error_ends_the_call(ctx, pkg, oracle, params_of, scheme):
    case = make_case("shared")
    params = params_of(case.k)
    T = Forwarded(PR.Blake2bWrite(), fail_write_at=1)
    with pytest.raises(pkg.AmdzkError) as e:
        run_device(ctx, pkg, oracle, params, case, scheme, transcript=T)
    assert e.value.code == E_INVALID and "multiopen:" in str(e.value) and "transcript" in str(e.value)
    assert T.writes == 1  # nothing is written behind the failure
    assert run_device(ctx, pkg, oracle, params, case, scheme) == oracle_of("shared", scheme)


def test_argument_refusals(ctx, pkg, oracle, params_of):
    case = make_case("one")
    params = params_of(case.k)
    kzg = pkg.kzg

    def refused(**kw):
        a = {"polys": [0x1000], "points": zu.fr_array_from_ints(case.point_vals), "queries": [(0, 0)], "transcript": Forwarded(PR.Blake2bWrite()),
             "params": params}
        a.update(kw)
        T = a["transcript"]
        with pytest.raises(pkg.AmdzkError) as e:
            kzg.multiopen(a.pop("params"), a.pop("polys"), a.pop("points"), a.pop("queries"), a.pop("transcript"), **a)
        assert e.value.code == E_INVALID and str(e.value).split(": ", 1)[1].startswith("multiopen:"), str(e.value)
        assert T is None or T.calls == 0
    refused(transcript=None)
    refused(opts_size=8)
    refused(queries=[])
    refused(queries=[(1, 0)])
    refused(queries=[(0, 1)])
    refused(polys=[None])
    refused(scheme=1)
    no_g = kzg.ParamsKZG(ctx, 4, g=None, g_lagrange=oracle.srs_powers(zu.fr_from_int(5), 16))
    refused(params=no_g)
    no_g.free()
    assert run_device(ctx, pkg, oracle, params, case, "shplonk") == oracle_of("one", "shplonk")


def test_proof_path_is_undisturbed(ctx, pkg, oracle):
    """One k = 5 proof of amdzk_create_proof_ex with each opening scheme, byte for byte the oracle prover's."""
    plonk = pkg.plonk
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    g, gl = zu.test_srs(oracle, c.k, TAU)
    params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(123456789))
    adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=123456789)
    for kind, name in ((0, "shplonk"), (plonk.MULTIOPEN_GWC, "gwc")):
        got = plonk.create_proof(ctx, pk, inst, d_adv, seed=41, transcript=kind)
        want = PR.create_proof(opk, c.instances, c.advice, seed=41, multiopen=name)
        assert hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()
    d_adv.free(); pk.free(); params.free()
