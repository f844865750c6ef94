"""CPU: what the reference does at degenerate caller-chosen challenges, asserted from oracle/plonk_ref.py alone.

tests/degenerate_cases.py holds the cases and the class each is stated to have — the reference proves and its verifier
accepts, proves and its verifier raises (1 / (x^n - 1)), or the prover itself raises (the identity written at y = 0,
1 / z_0(u) with u on an opening point outside SHPLONK's first set). This file runs the reference under each script and
asserts the class; the GPU tests take their expectations from the same outcome() and may not reclassify a case."""
import pytest

import degenerate_cases as DC
import scripted_transcript as ST
import verify_cases as VC
from degenerate_cases import PR, R

CASE_NAMES = ["theta=0", "theta=1", "beta=0", "gamma=0", "beta=gamma=0", "y=1", "y'=0", "v=0", "y'=v=0", "y'=v=1", "all=12345",
              "theta=beta=gamma=y=x", "x=0", "x=1", "x=w^3", "all=r-1", "y=0", "u=x", "u=xw", "u=xw^-1", "u=xw^-(bf+1)"]


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def test_the_case_list_is_the_one_the_gpu_tests_use(plonk):
    assert list(DC.cases(plonk)) == CASE_NAMES
    assert VC.oracle_key(plonk, "lookup")[0].desc["blinding_factors"] == 5, "u = x w^-6 is x w^-(bf+1) on this circuit"


def test_the_scripted_transcript_replaces_only_the_value(plonk):
    """The hash goes on as if nothing had happened: the squeezes behind a replaced one are the unscripted ones, a callable
    sees the values handed out so far, writer and reader agree, and the oracle refuses raw words."""
    for transcript in ("blake2b", "keccak"):
        plain, w = ST.writer(transcript, {}), ST.writer(transcript, {1: 5, 2: lambda sq: sq[0] + sq[1], 3: R + 9})
        for t in (plain, w):
            t.common_scalar(77)
        a = [plain.squeeze_challenge() for _ in range(5)]
        b = [w.squeeze_challenge() for _ in range(5)]
        assert b == [a[0], 5, (a[0] + 5) % R, 9, a[4]] and w.squeezed == b and plain.squeezed == a
        w.write_scalar(3)
        rd = ST.reader(transcript, {1: 5}, bytes(w.proof))
        rd.common_scalar(77)
        assert [rd.squeeze_challenge() for _ in range(5)][:2] == [a[0], 5] and rd.read_scalar() == 3
    with pytest.raises(AssertionError, match="raw words"):
        ST.writer("blake2b", {0: ST.Raw(R)}).squeeze_challenge()
    dw = ST.device_writer("blake2b", {0: ST.Raw(R), 1: ST.Raw((1 << 256) - 1)})
    assert [int(x) for x in dw.squeeze_challenge()] == [(R >> (64 * i)) & (2**64 - 1) for i in range(4)]
    assert [int(x) for x in dw.squeeze_challenge()] == [2**64 - 1] * 4


def test_install_restores_the_oracles_names(plonk, monkeypatch):
    before = {n: getattr(PR, n) for n in ("Blake2bWrite", "Blake2bRead", "Keccak256Write", "Keccak256Read")}
    with pytest.raises(KeyError):
        with ST.installed(monkeypatch, "blake2b", {0: 1}):
            assert PR.Blake2bWrite is not before["Blake2bWrite"] and PR.Blake2bWrite().squeeze_challenge() == 1
            raise KeyError("inside")
    assert {n: getattr(PR, n) for n in before} == before


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_reference_has_the_stated_class(plonk, name, multiopen):
    kw, shplonk_class, gwc_class = DC.cases(plonk)[name]
    cls, proof, why = DC.outcome(plonk, name, multiopen)
    print(name, multiopen, "->", cls, why)
    assert cls == (shplonk_class if multiopen == "shplonk" else gwc_class), why
    if cls == DC.VERIFIER_RAISES:
        assert "ZeroDivisionError" in why or "not invertible" in why, why  # 1 / (x^n - 1)
    if name == "y=0":
        assert "infinity" in why
    if cls == DC.PROVER_RAISES and name != "y=0":
        assert multiopen == "shplonk" and ("ZeroDivisionError" in why or "not invertible" in why), why  # 1 / z_0(u)
    if proof is not None and not set(kw) & {"theta", "beta", "gamma", "y", "x"} and multiopen == "shplonk" and "u" not in kw:
        assert proof != DC.unscripted(plonk, multiopen), "the script changed nothing"


def test_scripted_challenges_really_are_the_ones_used(plonk):
    """The proof under x = 7 differs from the unscripted one from the evaluations on and equals it in every commitment
    before them; a GWC proof does not depend on u (the reader's squeeze)."""
    c, opk = VC.oracle_key(plonk, "lookup")
    with pytest.MonkeyPatch.context() as mp, ST.installed(mp, "blake2b", {DC.X: 7}):
        p7 = bytes(PR.create_proof(opk, c.instances, c.advice, seed=DC.SEED))
    plain = DC.unscripted(plonk)
    import verify_ref as VR
    kinds = VR.element_kinds(c.desc, 1)
    first_scalar = 32 * kinds.index("s")
    assert p7[:first_scalar] == plain[:first_scalar] and p7[first_scalar:first_scalar + 32] != plain[first_scalar:first_scalar + 32]
    assert DC.outcome(plonk, "u=xw", "gwc")[1] == DC.outcome(plonk, "u=x", "gwc")[1]


@pytest.mark.parametrize("name", DC.KECCAK)
def test_keccak_has_the_same_class(plonk, name):
    for multiopen in ("shplonk", "gwc"):
        assert DC.outcome(plonk, name, multiopen, transcript="keccak")[0] == DC.PROVES


@pytest.mark.parametrize("name", DC.TWO_INSTANCES)
def test_two_instances_have_the_same_class(plonk, name):
    cls, proof, why = DC.outcome(plonk, name, "shplonk", N=2)
    assert cls == DC.PROVES, why
    assert len(proof) > len(DC.outcome(plonk, name, "shplonk")[1])


@pytest.mark.parametrize("name", list(DC.PHASED))
def test_a_phased_circuit_proves_and_verifies_with_degenerate_phase_challenges(plonk, name):
    """rlc_circuit, three phases, through tests/phased_oracle.py: both phase challenges 0, then both equal. The harness
    asserts that the wrapped transcript squeezes the very values the description was specialised to."""
    proof, ch = DC.phased_outcome(plonk, name, k=5)
    assert ch == list(DC.PHASED[name]) and len(proof) > 0
