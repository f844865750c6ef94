"""GPU: amdzk_verify_proofs_decide — plonk::verify_proof WITH the pairing, a verdict per proof — on proofs the device prover
made of the small circuits of tests/verify_cases.py. Every expected verdict comes from the oracle side,
verify_ref.holds(verify_ref.pair(...), tau) with the tau the test SRS was made from, never from the code under test; g2 and
s_g2 come from amdzk_g2_setup(tau)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402
from test_gpu_verify import Rig, put  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, R = VC.TAU, zu.R


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


@pytest.fixture(scope="module")
def rigs(ctx, pkg, plonk, oracle):
    made = {}

    def get(name, N=1):
        if (name, N) not in made:
            made[(name, N)] = Rig(ctx, pkg, plonk, oracle, name, N)
        return made[(name, N)]
    yield get
    for r in made.values():
        r.free()


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
    yield v
    v.free()


def decide(plonk, rig, vp, case, proofs, pk=None, **kw):
    return plonk.decide_proofs(rig.ctx, pk or rig.pk, vp, [rig.instances_arg()] * len(proofs), proofs,
                               transcript=VC.kind_flags(plonk, case.transcript, case.multiopen), n_circuits=rig.N, **kw)


def oracle_verdict(case, proof):
    """The oracle side's decision: well formed by the reference decode, and tau * L == R for the reference pair."""
    return case.decode(proof) == (0, 0) and VR.holds(case.pair(proof), TAU)


def false_proof(case):
    """An evaluation scalar + 1, kept below r: well formed and false — asserted from the oracle, so nothing passes vacuously."""
    kinds = VR.element_kinds(case.desc, case.N, case.multiopen)
    psz, end = (64, "big") if case.transcript == "evm" else (32, "little")
    off = 0
    for k in kinds:
        if k == "s":
            v = int.from_bytes(case.proof[off:off + 32], end)
            if v + 1 < R:
                m = put(case.proof, off, (v + 1).to_bytes(32, end))
                assert case.decode(m) == (0, 0) and not VR.holds(case.pair(m), TAU)
                return m
        off += psz if k == "p" else 32
    raise AssertionError("no evaluation to mutate")


# ------------------------------------------------------------------------------------ single proofs
@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_the_devices_valid_proof_is_decided_valid(plonk, rigs, vparams, name, N, transcript, multiopen):
    rig = rigs(name, N)
    case = rig.case(transcript, multiopen)
    assert oracle_verdict(case, case.proof)
    verdicts, statuses = decide(plonk, rig, vparams, case, [case.proof])
    assert statuses == [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)] and verdicts == [True]


@pytest.mark.parametrize("name,transcript,multiopen", [("square", "blake2b", "shplonk"), ("lookup", "evm", "gwc")])
def test_a_well_formed_false_proof_is_decided_false(plonk, rigs, vparams, name, transcript, multiopen):
    rig = rigs(name)
    case = rig.case(transcript, multiopen)
    m = false_proof(case)
    verdicts, statuses = decide(plonk, rig, vparams, case, [m])
    assert statuses == [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)] and verdicts == [False]
    assert decide(plonk, rig, vparams, case, [m], combined=True)[0] == [False]


# ------------------------------------------------------------------------------------ batches
def test_a_mixed_batch_gets_a_verdict_per_proof_and_combined_gets_one_for_all(plonk, rigs, vparams):
    rig = rigs("square")
    a, b = rig.case("blake2b", "shplonk", seed=20), rig.case("blake2b", "shplonk", seed=21)
    malformed = put(a.proof, 32, bytes(32))
    batch = [a.proof, false_proof(a), malformed, b.proof, false_proof(b)]
    cases = [a, a, a, b, b]
    want = [oracle_verdict(c, p) for c, p in zip(cases, batch)]
    assert want == [True, False, False, True, False] and a.decode(malformed) == (2, 32)
    verdicts, statuses = decide(plonk, rig, vparams, a, batch)
    assert verdicts == want and sum(verdicts) == 2
    assert [tuple(s) for s in statuses] == [(0, 0), (0, 0), (2, 32), (0, 0), (0, 0)]
    again, _ = decide(plonk, rig, vparams, a, batch, combine_seed=12345)  # weights are ignored: deterministic
    assert again == want
    verdicts, statuses = decide(plonk, rig, vparams, a, batch, combined=True, combine_seed=0xC0FFEE)
    assert verdicts == [False] * 5 and [s.status for s in statuses] == [0, 0, 2, 0, 0]
    # the raw call reports the count
    n_valid = raw_n_valid(plonk, rig, vparams, a, batch, 0)
    assert n_valid == 2


def raw_n_valid(plonk, rig, vp, case, proofs, flags):
    inst_pp, lens_pp, pp, pl, opts, st, keep = plonk._verify_args([rig.instances_arg()] * len(proofs), proofs,
                                                                  VC.kind_flags(plonk, case.transcript, case.multiopen), rig.N, 0, None, None)
    verdicts = np.full(len(proofs), 7, np.uint8)
    n_valid = C.c_size_t(99)
    rc = rig.ctx.L.amdzk_verify_proofs_decide(rig.ctx.h, rig.pk.h, vp.s_g2.h, vp.g2.h, flags, len(proofs), inst_pp, lens_pp, pp, pl, C.byref(opts), st,
                                              verdicts.ctypes.data, C.byref(n_valid))
    assert rc == 0 and set(verdicts) <= {0, 1} and int(verdicts.sum()) == n_valid.value
    return n_valid.value


def test_an_all_valid_batch_is_all_valid_in_both_modes(plonk, rigs, vparams):
    rig = rigs("lookup")
    cases = [rig.case("evm", "shplonk", seed=30 + b) for b in range(3)]
    proofs = [c.proof for c in cases]
    assert all(oracle_verdict(c, c.proof) for c in cases)
    assert decide(plonk, rig, vparams, cases[0], proofs)[0] == [True] * 3
    assert decide(plonk, rig, vparams, cases[0], proofs, combined=True, combine_seed=0xDEADBEEF12345)[0] == [True] * 3
    rho = np.stack([zu.fr_from_int(v) for v in (3, R - 1, 0x1F1F1F1F1F1F1F1F1F)])
    assert decide(plonk, rig, vparams, cases[0], proofs, combined=True, combine_scalars=rho)[0] == [True] * 3


@pytest.mark.parametrize("at", [15, 16])
def test_one_false_proof_at_the_run_boundary(plonk, rigs, vparams, at):
    """AMDZK_DECIDE_RUN + 1 proofs: two MSM runs, the false proof the last of the first or the only one of the second."""
    rig = rigs("square")
    assert plonk.DECIDE_RUN == 16
    cases = [rig.case("blake2b", "shplonk", seed=20 + b % 3) for b in range(17)]
    proofs = [c.proof for c in cases]
    proofs[at] = false_proof(cases[at])
    want = [b != at for b in range(17)]
    assert all(oracle_verdict(cases[b], proofs[b]) == want[b] for b in (0, 1, 2, at))
    verdicts, statuses = decide(plonk, rig, vparams, cases[0], proofs)
    assert verdicts == want and all(s.status == 0 for s in statuses)


def test_a_run_without_a_well_formed_proof_and_positions_behind_it(plonk, rigs, vparams):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk", seed=20)
    bad = case.proof[:-1]
    proofs = [bad] * 16 + [case.proof, false_proof(case), bad]
    verdicts, statuses = decide(plonk, rig, vparams, case, proofs)
    assert verdicts == [False] * 16 + [True, False, False]
    assert [s.status for s in statuses] == [1] * 16 + [0, 0, 1]


def test_another_trapdoor_in_g2_decides_every_proof_false(ctx, pkg, plonk, rigs):
    rig = rigs("square")
    cases = [rig.case("blake2b", "shplonk", seed=20 + b) for b in range(2)]
    wrong = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU + 1))
    try:
        assert all(oracle_verdict(c, c.proof) for c in cases) and not VR.holds(cases[0].pair(), TAU + 1)
        assert decide(plonk, rig, wrong, cases[0], [c.proof for c in cases])[0] == [False, False]
        assert decide(plonk, rig, wrong, cases[0], [c.proof for c in cases], combined=True, combine_seed=5)[0] == [False, False]
    finally:
        wrong.free()


def test_an_all_malformed_batch_has_no_valid_proof(plonk, rigs, vparams):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk", seed=20)
    batch = [case.proof[:-1], put(case.proof, 0, bytes(32)), case.proof + b"\0"]
    for combined in (False, True):
        verdicts, statuses = decide(plonk, rig, vparams, case, batch, combined=combined)
        assert verdicts == [False] * 3 and [tuple(s) for s in statuses] == [(1, 0), (2, 0), (1, 0)]
        assert raw_n_valid(plonk, rig, vparams, case, batch, 1 if combined else 0) == 0


# ------------------------------------------------------------------------------------ keys, mirrors, refusals
def test_workspace_clones_and_keys_from_a_key_file_decide_the_same(ctx, plonk, rigs, vparams):
    rig = rigs("lookup")
    case = rig.case("blake2b", "shplonk")
    batch = [case.proof, false_proof(case)]
    want = [oracle_verdict(case, p) for p in batch]
    assert want == [True, False]
    clone = rig.pk.clone_workspace()
    loaded = plonk.ProvingKey.read(ctx, rig.params, rig.pk.write())
    try:
        for key in (rig.pk, clone, loaded):
            assert decide(plonk, rig, vparams, case, batch, pk=key)[0] == want
    finally:
        loaded.free()
        clone.free()


def test_python_decide_proof_returns_a_bool_and_raises_on_a_malformed_proof(plonk, rigs, vparams):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk")
    assert oracle_verdict(case, case.proof)
    assert plonk.decide_proof(rig.ctx, rig.pk, vparams, rig.inst, case.proof) is True
    assert plonk.decide_proof(rig.ctx, rig.pk, vparams, rig.inst, false_proof(case)) is False
    with pytest.raises(ValueError, match=r"status 2 \(BAD_POINT\), offset 32"):
        plonk.decide_proof(rig.ctx, rig.pk, vparams, rig.inst, put(case.proof, 32, bytes(32)))
    with pytest.raises(ValueError, match=r"status 1 \(BAD_LENGTH\), offset 0"):
        plonk.decide_proof(rig.ctx, rig.pk, vparams, rig.inst, case.proof[:-1])


def test_refusals_carry_the_calls_prefix_and_leave_the_ctx_usable(ctx, pkg, plonk, rigs, vparams):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk")
    L = ctx.L
    inst_pp, lens_pp, pp, pl, opts, st, keep = plonk._verify_args([rig.inst], [case.proof], 0, 1, 0, None, None)
    verdicts = np.zeros(1, np.uint8)
    n_valid = C.c_size_t(0)
    VO = pkg.ffi.VerifyOpts

    def call(pk=rig.pk.h, s_g2=vparams.s_g2.h, g2=vparams.g2.h, flags=0, n=1, proofs=pp, o=opts, v=verdicts.ctypes.data, nv=C.byref(n_valid)):
        return L.amdzk_verify_proofs_decide(ctx.h, pk, s_g2, g2, flags, n, inst_pp, lens_pp, proofs, pl, C.byref(o), st, v, nv)

    for kw in (dict(pk=None), dict(s_g2=None), dict(g2=None), dict(v=None), dict(flags=2), dict(flags=0x80000001), dict(n=0), dict(proofs=None),
               dict(o=VO(C.sizeof(VO) - 1, 0, 1, 0, None)), dict(o=VO(C.sizeof(VO), 2, 1, 0, None))):
        assert call(**kw) == -2, kw
        assert L.amdzk_last_error(ctx.h).decode().startswith("verify_proofs_decide:"), (kw, L.amdzk_last_error(ctx.h))
        assert call() == 0 and verdicts[0] == 1 and n_valid.value == 1
    assert call(nv=None) == 0 and verdicts[0] == 1  # n_valid may be NULL
    with pytest.raises(pkg.ffi.AmdzkError, match="verify_proofs_decide:"):
        plonk.decide_proofs(ctx, rig.pk, vparams, [rig.inst], [case.proof], opts_size=8)
    # amdzk_verify_proofs keeps its own prefix and its pair
    g = plonk.verify_proof(ctx, rig.pk, rig.inst, case.proof)
    assert (zu.point_to_ints(g.lhs), zu.point_to_ints(g.rhs)) == case.pair()
