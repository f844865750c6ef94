"""GPU: create_proof and verify_proofs at degenerate caller-chosen challenges.

With a caller-owned transcript the challenges are inputs of the library. tests/scripted_transcript.py hands the device the
oracle's transcript with chosen squeezes replaced — 0, 1, r - 1, roots of unity, equal values, an opening point — and
tests/degenerate_cases.py states, from the reference alone (tests/test_scripted_oracle.py asserts it), what each case is.
Where the reference proves and verifies, the device's bytes are the reference's and its verifier gives the reference's
pair and verdict 1; the rest are the outcomes pinned below: a named refusal of the prover (beta = 0 on a key with a
permutation, x = 0, u on an opening point outside SHPLONK's first set, y = 0's identity commitment, a squeezed challenge
that is not below r) or AMDZK_PROOF_BAD_TRANSCRIPT of the verifier (x = 0, x^n = 1). After every refusal the same ctx and
key prove the unscripted proof. All comparisons are exact."""
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import batch_opts_util as U  # noqa: E402
import degenerate_cases as DC  # noqa: E402
import scripted_transcript as ST  # noqa: E402
import verify_ref as VR  # noqa: E402
from degenerate_cases import PR, R, SEED  # noqa: E402
import circuits  # noqa: E402
from test_gpu_phased import Device  # noqa: E402
from test_gpu_verify import Rig  # noqa: E402
from test_scripted_oracle import CASE_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = DC.VC.TAU
INVALID, UNSUPPORTED = -2, -5
WELL, BAD_TRANSCRIPT = 0, 5
MULTIOPENS = ("shplonk", "gwc")
BETA_TEXT = "create_proof: the challenge beta is zero (probability 2^-254): the factored permutation terms need 1 / beta"
X_TEXT = "create_proof: the challenge x is zero (probability 2^-254): rotations of x coincide"
U_TEXT = "create_proof: the challenge u is one of the opening points (probability 2^-254)"
BIG_TEXT = "create_proof: a squeezed challenge is not below the modulus"
U_ON_POINT = ("u=xw", "u=xw^-1", "u=xw^-(bf+1)")
XN_IS_ONE = ("x=1", "x=w^3", "all=r-1")


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
def rig(rigs):
    """The lookup circuit at k = 5 with two workspaces: pks[0] proves alone, both prove a batch or two instances."""
    return rigs("lookup", 2)


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
    yield v
    v.free()


def mo_flag(plonk, multiopen):
    return plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0


def script_of(plonk, name, multiopen):
    return DC.script(multiopen, **DC.cases(plonk)[name][0])


def prove(plonk, rig, sc, multiopen, transcript="blake2b", seed=SEED, N=1):
    """create_proof_opts under the scripted writer: (the writer, its bytes)."""
    t = ST.device_writer(transcript, sc)
    out = plonk.create_proof_opts(rig.ctx, rig.pks[:N], [rig.inst] * N, rig.d_adv[:N], seed=seed, transcript=mo_flag(plonk, multiopen), transcript_object=t)
    assert out == b""  # the bytes are the caller's
    return t, t.proof


def prove_batch(plonk, rig, sc, multiopen, transcript="blake2b"):
    """Two proofs in one call: proof 0 under the scripted writer with seed SEED, proof 1 built-in with seed 9."""
    t = ST.device_writer(transcript, sc)
    got = plonk.create_proof_batch_opts(rig.ctx, rig.pks, [rig.inst] * 2, rig.d_adv, seeds=[SEED, 9], transcript=mo_flag(plonk, multiopen),
                                        transcript_objects=[t, None])
    return t, got


def still_proves(plonk, rig, multiopen="shplonk"):
    """After a refusal: the same ctx and key prove the unscripted proof, and the device verifies it."""
    flags = mo_flag(plonk, multiopen)
    proof = plonk.create_proof(rig.ctx, rig.pk, rig.inst, rig.d_adv[0], seed=SEED, transcript=flags)
    assert proof == DC.unscripted(plonk, multiopen)
    g = plonk.verify_proof(rig.ctx, rig.pk, rig.inst, proof, transcript=flags)
    assert VR.holds((zu.point_to_ints(g.lhs), zu.point_to_ints(g.rhs)), TAU)


def reference_pair(plonk, rig, sc, proof, multiopen, transcript="blake2b", N=1):
    with pytest.MonkeyPatch.context() as mp, ST.installed(mp, transcript, sc):
        return VR.pair(rig.opk, [rig.c.instances] * N, proof, transcript=ST.kind(transcript), multiopen=multiopen)


def ints(g):
    return zu.point_to_ints(g.lhs), zu.point_to_ints(g.rhs)


def verifies(plonk, rig, vparams, sc, proof, multiopen, transcript="blake2b", N=1):
    """verify_proofs and verify_proofs_decide through the scripted reader: a well-formed status, the reference's pair under
    the same script, verdict 1."""
    flags = mo_flag(plonk, multiopen)
    inst = rig.inst if N == 1 else [rig.inst] * N
    g = plonk.verify_proofs(rig.ctx, rig.pk, [inst], [None], transcript=flags, n_circuits=N, transcripts=[ST.device_reader(transcript, sc, proof)])
    assert g.errors == [] and [tuple(s) for s in g.statuses] == [(WELL, 0)]
    want = reference_pair(plonk, rig, sc, proof, multiopen, transcript, N)
    assert ints(g) == want and VR.holds(want, TAU)
    verdicts, statuses = plonk.decide_proofs(rig.ctx, rig.pk, vparams, [inst], [None], transcript=flags, n_circuits=N,
                                             transcripts=[ST.device_reader(transcript, sc, proof)])
    assert verdicts == [True] and [tuple(s) for s in statuses] == [(WELL, 0)]


def legal(plonk):
    """(case, opening scheme) pairs the reference proves and verifies and the device does not refuse by name."""
    out = []
    for name, (_, sh, gw) in DC.cases(plonk).items():
        for mo, cls in zip(MULTIOPENS, (sh, gw)):
            if cls == DC.PROVES and name not in DC.PINNED:
                out.append((name, mo))
    return out


# the parametrisation cannot ask the `plonk` fixture: the list is spelled out here and checked against legal() below
LEGAL = [(n, mo) for n in CASE_NAMES for mo in MULTIOPENS
         if n not in DC.PINNED + XN_IS_ONE + ("y=0",) and not (mo == "shplonk" and n in U_ON_POINT)]


def test_the_legal_list_is_the_references(plonk):
    """No case dropped or reclassified: LEGAL is exactly what degenerate_cases states, which the CPU test asserts."""
    assert LEGAL == legal(plonk)
    for name, mo in LEGAL:
        assert DC.outcome(plonk, name, mo)[0] == DC.PROVES


# ------------------------------------------------------------------------------------ legal cases
@pytest.mark.parametrize("name,multiopen", LEGAL)
def test_legal_cases_give_the_references_bytes_and_verify(plonk, rig, vparams, name, multiopen):
    sc = script_of(plonk, name, multiopen)
    cls, want, _ = DC.outcome(plonk, name, multiopen)
    assert cls == DC.PROVES
    t, proof = prove(plonk, rig, sc, multiopen)
    assert t.squeezes == (8 if multiopen == "shplonk" else 6)
    assert proof == want, "the device's proof differs from the reference's under the same script"
    verifies(plonk, rig, vparams, sc, proof, multiopen)


@pytest.mark.parametrize("multiopen", MULTIOPENS)
@pytest.mark.parametrize("name", DC.KECCAK)
def test_legal_cases_under_keccak(plonk, rig, vparams, name, multiopen):
    sc = script_of(plonk, name, multiopen)
    cls, want, _ = DC.outcome(plonk, name, multiopen, transcript="keccak")
    assert cls == DC.PROVES
    _, proof = prove(plonk, rig, sc, multiopen, transcript="keccak")
    assert proof == want
    verifies(plonk, rig, vparams, sc, proof, multiopen, transcript="keccak")


@pytest.mark.parametrize("name,multiopen", [("gamma=0", "shplonk"), ("all=12345", "gwc"), ("u=x", "shplonk")])
def test_legal_cases_in_a_batch_beside_an_unscripted_proof(plonk, rig, name, multiopen):
    t, got = prove_batch(plonk, rig, script_of(plonk, name, multiopen), multiopen)
    assert got[0] == b"" and t.proof == DC.outcome(plonk, name, multiopen)[1]
    assert got[1] == DC.unscripted(plonk, multiopen, seed=9)


@pytest.mark.parametrize("name", DC.TWO_INSTANCES)
def test_legal_cases_with_two_instances(plonk, rig, vparams, name):
    sc = script_of(plonk, name, "shplonk")
    cls, want, _ = DC.outcome(plonk, name, "shplonk", N=2)
    assert cls == DC.PROVES
    _, proof = prove(plonk, rig, sc, "shplonk", N=2)
    assert proof == want
    verifies(plonk, rig, vparams, sc, proof, "shplonk", N=2)


@pytest.mark.parametrize("multiopen", MULTIOPENS)
@pytest.mark.parametrize("name", list(DC.PHASED))
def test_phased_key_with_degenerate_phase_challenges(ctx, pkg, plonk, oracle, vparams, name, multiopen):
    """rlc_circuit at k = 6, three phases, both phase challenges 0 and both equal: the callback is handed the scripted values,
    the bytes are the phased harness's, the verifier gives the harness's pair and verdict 1."""
    c, opk = DC.phased_circuit(plonk, 6)
    want, ch = DC.phased_outcome(plonk, name, multiopen, k=6)
    sc = dict(enumerate(ch))
    dev = Device(ctx, pkg, plonk, oracle, c)
    try:
        flags = mo_flag(plonk, multiopen)
        t = ST.device_writer("blake2b", sc)
        assert dev.prove(seed=SEED, transcript=flags, transcript_object=t) == b""
        assert dev.challenges() == ch
        assert t.proof == want
        g = plonk.verify_proofs(ctx, dev.pk, [dev.inst[0]], [None], transcript=flags, transcripts=[ST.device_reader("blake2b", sc, want)])
        assert g.errors == [] and [tuple(s) for s in g.statuses] == [(WELL, 0)]
        with pytest.MonkeyPatch.context() as mp, ST.phased("blake2b", sc) as tname:
            ref = VR.pair_phased(mp, opk, c.desc, [c.instances], want, ch, transcript=tname, multiopen=multiopen)
        assert ints(g) == ref and VR.holds(ref, TAU)
        verdicts, statuses = plonk.decide_proofs(ctx, dev.pk, vparams, [dev.inst[0]], [None], transcript=flags,
                                                 transcripts=[ST.device_reader("blake2b", sc, want)])
        assert verdicts == [True] and [tuple(s) for s in statuses] == [(WELL, 0)]
    finally:
        dev.free()


# ------------------------------------------------------------------------------------ pinned: refusals of the prover
def refused_alone(pkg, plonk, rig, sc, multiopen, code, text):
    t = ST.device_writer("blake2b", sc)
    with pytest.raises(pkg.AmdzkError) as e:
        plonk.create_proof_opts(rig.ctx, [rig.pk], [rig.inst], [rig.d_adv[0]], seed=SEED, transcript=mo_flag(plonk, multiopen), transcript_object=t)
    assert e.value.code == code and str(e.value).endswith(text), str(e.value)
    return t


def refused_in_a_batch(pkg, plonk, rig, sc, multiopen, code, text):
    """Only the scripted member fails; the other member's bytes are the reference's."""
    t, got = prove_batch(plonk, rig, sc, multiopen)
    assert isinstance(got[0], pkg.AmdzkError) and got[0].code == code, got[0]
    assert "proof 0: create_proof: " in str(got[0]) and str(got[0]).endswith(text), str(got[0])
    assert got[1] == DC.unscripted(plonk, multiopen, seed=9)
    return t


@pytest.mark.parametrize("multiopen", MULTIOPENS)
@pytest.mark.parametrize("name", ["beta=0", "beta=gamma=0"])
def test_beta_zero_on_a_key_with_a_permutation_is_refused_by_name(pkg, plonk, rig, name, multiopen):
    assert rig.c.desc["permutation_columns"]
    assert DC.outcome(plonk, name, multiopen)[0] == DC.PROVES  # the reference proves it: the refusal is the device's own
    sc = script_of(plonk, name, multiopen)
    t = refused_alone(pkg, plonk, rig, sc, multiopen, UNSUPPORTED, BETA_TEXT)
    assert t.squeezes == 3  # theta, beta, gamma: the transcript is advanced by what was called
    still_proves(plonk, rig, multiopen)
    t = refused_in_a_batch(pkg, plonk, rig, sc, multiopen, UNSUPPORTED, BETA_TEXT)
    assert t.squeezes == 3
    still_proves(plonk, rig, multiopen)


def lookup_without_permutation(plonk, k=5, seed=1):
    """One gate and one range lookup, no equality-enabled column: S = 0, and beta still reaches the lookup's product. The
    looked-up values are 1..7: at beta = 0 a permuted input of 0 would be a zero denominator of that product."""
    rnd = np.random.RandomState(seed)
    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    q, t = cs.selector(), cs.fixed_column()
    cs.create_gate(lambda m: [m.query_selector(q) * (m.query_advice(b, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))])
    cs.lookup(lambda m: [(m.query_selector(q) * m.query_advice(a, 0), m.query_fixed(t, 0))])
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    for row in range(c.usable):
        x = int(rnd.randint(1, 8))
        c.fixed[t.index][row], c.fixed[q.index][row] = row % 8, 1
        c.advice[a.index][row], c.advice[b.index][row] = x, x * x
    c.instances = []
    circuits.check_satisfied(c)
    return c


def test_beta_zero_without_a_permutation_gives_the_references_bytes(ctx, pkg, plonk, oracle):
    c = lookup_without_permutation(plonk, 5)
    assert c.desc["permutation_columns"] == [] and len(c.desc["lookups"]) == 1
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None)])
    try:
        for multiopen in MULTIOPENS:
            sc = DC.script(multiopen, beta=0)
            with pytest.MonkeyPatch.context() as mp, ST.installed(mp, "blake2b", sc):
                want = bytes(PR.create_proof(B.opk(0), c.instances, c.advice, seed=SEED, multiopen=multiopen))
                assert PR.verify_proof(B.opk(0), c.instances, want, multiopen=multiopen)
            assert want != bytes(PR.create_proof(B.opk(0), c.instances, c.advice, seed=SEED, multiopen=multiopen)), "beta is used"
            t = ST.device_writer("blake2b", sc)
            assert B.single(0, SEED, transcript=mo_flag(plonk, multiopen), transcript_object=t) == b""
            assert t.proof == want
    finally:
        B.free()


@pytest.mark.parametrize("multiopen", MULTIOPENS)
def test_y_zero_is_refused_as_the_reference_refuses_it(pkg, plonk, rig, multiopen):
    cls, _, why = DC.outcome(plonk, "y=0", multiopen)
    assert cls == DC.PROVER_RAISES and "infinity" in why
    sc = script_of(plonk, "y=0", multiopen)
    text = "commitment is the identity (cannot write points at infinity to the transcript)"
    refused_alone(pkg, plonk, rig, sc, multiopen, INVALID, text)
    still_proves(plonk, rig, multiopen)
    refused_in_a_batch(pkg, plonk, rig, sc, multiopen, INVALID, text)
    still_proves(plonk, rig, multiopen)


@pytest.mark.parametrize("name", U_ON_POINT)
def test_u_on_an_opening_point_outside_the_first_set_is_refused(pkg, plonk, rig, name):
    """SHPLONK: 1 / z_0(u) does not exist and the reference raises; the device used to go on with inv(0) = 0. On the single and
    on the gang path, per member; everything up to the first opening commitment has been written, the second has not."""
    assert DC.outcome(plonk, name, "shplonk")[0] == DC.PROVER_RAISES
    sc = script_of(plonk, name, "shplonk")
    head = DC.outcome(plonk, "u=x", "shplonk")[1][:-32]  # the same x: the bytes in front of u's squeeze do not depend on u
    t = refused_alone(pkg, plonk, rig, sc, "shplonk", UNSUPPORTED, U_TEXT)
    assert t.squeezes == 8 and t.proof == head
    still_proves(plonk, rig)
    t = refused_in_a_batch(pkg, plonk, rig, sc, "shplonk", UNSUPPORTED, U_TEXT)
    assert t.squeezes == 8 and t.proof == head
    still_proves(plonk, rig)


@pytest.mark.parametrize("multiopen", MULTIOPENS)
def test_x_zero_is_refused_before_anything_is_evaluated(pkg, plonk, rig, multiopen):
    """The reference merges the coinciding rotations of x = 0 by value and proves; the key's opening plan cannot."""
    cls, ref_proof, _ = DC.outcome(plonk, "x=0", multiopen)
    assert cls == DC.PROVES
    sc = script_of(plonk, "x=0", multiopen)
    kinds = VR.element_kinds(rig.c.desc, 1, multiopen)
    commitments = ref_proof[:32 * kinds.index("s")]  # everything in front of x's squeeze
    t = refused_alone(pkg, plonk, rig, sc, multiopen, UNSUPPORTED, X_TEXT)
    assert t.squeezes == 5 and t.proof == commitments  # not one evaluation was written
    still_proves(plonk, rig, multiopen)
    t = refused_in_a_batch(pkg, plonk, rig, sc, multiopen, UNSUPPORTED, X_TEXT)
    assert t.squeezes == 5 and t.proof == commitments
    still_proves(plonk, rig, multiopen)


@pytest.mark.parametrize("value", [R, (1 << 256) - 1])
@pytest.mark.parametrize("multiopen", MULTIOPENS)
def test_a_write_transcripts_challenge_that_is_not_below_r_is_refused(pkg, plonk, rig, multiopen, value):
    """Words of r and of 2^256 - 1, at squeeze 0 and at the prover's last squeeze, as the read transcripts refuse them."""
    last = 7 if multiopen == "shplonk" else 5
    for at in (0, last):
        sc = {at: ST.Raw(value)}
        t = refused_alone(pkg, plonk, rig, sc, multiopen, INVALID, BIG_TEXT)
        assert t.squeezes == at + 1
        t = refused_in_a_batch(pkg, plonk, rig, sc, multiopen, INVALID, BIG_TEXT)
        assert t.squeezes == at + 1
    still_proves(plonk, rig, multiopen)


# ------------------------------------------------------------------------------------ pinned: x^n = 1
@pytest.mark.parametrize("multiopen", MULTIOPENS)
@pytest.mark.parametrize("name", XN_IS_ONE)
def test_the_prover_at_a_root_of_unity_gives_the_references_bytes(plonk, rig, name, multiopen):
    """Nothing in the prover divides by x^n - 1: the reference proves, and so does the device, byte for byte."""
    cls, want, _ = DC.outcome(plonk, name, multiopen)
    assert cls == DC.VERIFIER_RAISES
    _, proof = prove(plonk, rig, script_of(plonk, name, multiopen), multiopen)
    assert proof == want


def degenerate_x_in_the_middle(plonk, rig, name, multiopen, call):
    """The case's reference proof as the second of three, read through the scripted reader: `call` runs one of the verify
    forms on (instances, proofs, transcripts, weights) and returns the statuses; the proof gets BAD_TRANSCRIPT with offset =
    the reads made before x's squeeze, its neighbours are untouched."""
    sc = script_of(plonk, name, multiopen)
    bad = DC.outcome(plonk, name, multiopen)[1]
    good = DC.unscripted(plonk, multiopen)
    rd = ST.device_reader("blake2b", sc, bad)
    w = np.stack([zu.fr_from_int(v) for v in (2, 11, 7)])
    statuses = call([rig.inst] * 3, [good, None, good], [None, rd, None], w)
    assert rd.order.count("c") == DC.X + 1, "no member is called behind the refused squeeze"
    want_off = rd.reads_before_squeeze(DC.X)
    assert want_off == VR.element_kinds(rig.c.desc, 1, multiopen).index("s")
    assert [tuple(s) for s in statuses] == [(WELL, 0), (BAD_TRANSCRIPT, want_off), (WELL, 0)]
    return good


@pytest.mark.parametrize("multiopen", MULTIOPENS)
@pytest.mark.parametrize("name", ("x=0",) + XN_IS_ONE)
def test_the_verifier_reports_a_degenerate_x_as_a_bad_transcript(plonk, rig, name, multiopen):
    """x = 0 and x^n = 1 (x = 1, w^3, r - 1), where upstream's verifier panics and the reference raises: that proof alone
    drops out, and the combined pair is the reference's over the other two."""
    flags = mo_flag(plonk, multiopen)
    out = {}

    def call(inst, proofs, trs, w):
        out["g"] = plonk.verify_proofs(rig.ctx, rig.pk, inst, proofs, transcript=flags, combine_scalars=w, transcripts=trs)
        assert out["g"].errors == []
        return out["g"].statuses
    good = degenerate_x_in_the_middle(plonk, rig, name, multiopen, call)
    one = VR.pair(rig.opk, [rig.c.instances], good, multiopen=multiopen)
    assert ints(out["g"]) == VR.combine([one, one], [2, 7])


def test_the_other_verify_forms_report_a_degenerate_x_the_same_way(plonk, rig, vparams):
    """One case each: the verifying-key form, the mixed form, and the three decide forms."""
    vk = rig.pk.get_vk()
    try:
        def with_vk(inst, proofs, trs, w):
            return plonk.verify_proofs(rig.ctx, vk, inst, proofs, combine_scalars=w, transcripts=trs).statuses
        degenerate_x_in_the_middle(plonk, rig, "x=1", "shplonk", with_vk)

        def mixed(inst, proofs, trs, w):
            items = [plonk.VerifyItem(rig.pk if b != 2 else vk, inst[b], proofs[b], transcript=plonk.MULTIOPEN_GWC, reader=trs[b]) for b in range(3)]
            return plonk.verify_proofs_mixed(rig.ctx, items, combine_scalars=w).statuses
        degenerate_x_in_the_middle(plonk, rig, "x=w^3", "gwc", mixed)

        def decide(key):
            def run(inst, proofs, trs, w):
                verdicts, statuses = plonk.decide_proofs(rig.ctx, key, vparams, inst, proofs, transcripts=trs)
                assert verdicts == [True, False, True]
                return statuses
            return run
        degenerate_x_in_the_middle(plonk, rig, "all=r-1", "shplonk", decide(rig.pk))
        degenerate_x_in_the_middle(plonk, rig, "x=0", "shplonk", decide(vk))

        def decide_mixed(inst, proofs, trs, w):
            items = [plonk.VerifyItem(vk if b != 2 else rig.pk, inst[b], proofs[b], reader=trs[b]) for b in range(3)]
            verdicts, statuses = plonk.decide_proofs_mixed(rig.ctx, vparams, items)
            assert verdicts == [True, False, True]
            return statuses
        degenerate_x_in_the_middle(plonk, rig, "x=1", "shplonk", decide_mixed)
    finally:
        vk.free()


# ------------------------------------------------------------------------------------ pinned: the verifier with u on a point
def test_the_verifier_with_u_on_an_opening_point_gives_the_references_pair(plonk, rig, vparams):
    """An honest proof under x = 7, read back with u = x w scripted: upstream's verifier divides by nothing here, so the pair
    is the reference's — whose L = z_0(u) h2 is the identity — and decide says 0 with a well-formed status."""
    w = DC.omega(plonk)
    honest = DC.script("shplonk", x=7)
    _, proof = prove(plonk, rig, honest, "shplonk")
    with pytest.MonkeyPatch.context() as mp, ST.installed(mp, "blake2b", honest):
        assert proof == bytes(PR.create_proof(rig.opk, rig.c.instances, rig.c.advice, seed=SEED))
    sc = DC.script("shplonk", x=7, u=DC.x_times(w, 1))
    want = reference_pair(plonk, rig, sc, proof, "shplonk")
    assert want[0] is None and want[1] is not None, "z_0(u) = 0: L is the identity"
    g = plonk.verify_proofs(rig.ctx, rig.pk, [rig.inst], [None], transcripts=[ST.device_reader("blake2b", sc, proof)])
    assert g.errors == [] and [tuple(s) for s in g.statuses] == [(WELL, 0)]
    assert ints(g) == want
    verdicts, statuses = plonk.decide_proofs(rig.ctx, rig.pk, vparams, [rig.inst], [None], transcripts=[ST.device_reader("blake2b", sc, proof)])
    assert verdicts == [False] and [tuple(s) for s in statuses] == [(WELL, 0)]
    # under the honest script the same bytes verify
    verifies(plonk, rig, vparams, honest, proof, "shplonk")
