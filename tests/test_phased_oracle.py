"""CPU: the phased-order harness (tests/phased_oracle.py) is self-consistent, the phased test circuits are satisfiable
under it, and the Python mirror validates and flattens a phase table. Nothing here needs a device; the GPU tests compare
the library's bytes with what this harness produces."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import phased_circuits as PC  # noqa: E402
import phased_oracle as PO  # noqa: E402
import plonk_ref as PR  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
# seeds of phased_circuits.random_phased_circuit the GPU suite proves: each one proves and verifies under the wrapped
# oracle (test_random_phased_circuits_prove_and_verify_on_cpu), so none is skipped on the device
RANDOM_SEEDS = list(range(24))


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def phased_lookup_circuit(plonk, k=5, seed=3):
    """lookup_circuit with its last advice column treated as phase 1 and one challenge after phase 0 (no expression uses
    it: the witness is the plain one, only the order of commitments, squeezes and draws changes)."""
    c = circuits.lookup_circuit(plonk, k, seed=seed)
    desc = dict(c.desc)
    desc["advice_column_phase"] = [0] * (desc["num_advice"] - 1) + [1]
    desc["challenge_phase"] = [0]
    return c, desc


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("transcript", ["blake2b", "keccak"])
def test_harness_is_self_consistent(plonk, monkeypatch, N, transcript):
    c, desc = phased_lookup_circuit(plonk)
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=77)
    inst, adv = [c.instances] * N, [c.advice] * N
    ch = PO.synthesize_on_cpu(monkeypatch, opk, desc, inst, adv, [lambda *a: None] * N, seed=4, transcript=transcript)
    assert len(ch) == 1 and 0 < ch[0] < PO.R
    proof = PO.create_proof(monkeypatch, opk, desc, inst, adv, 4, ch, transcript=transcript)
    assert PO.verify_proof(monkeypatch, opk, desc, inst, proof, ch, transcript=transcript)
    # the order matters: other bytes than the phase-0 proof of the same witness, and the plain verifier rejects them
    plain = PR.create_proof_multi(opk, inst, adv, 4, transcript=transcript)
    assert len(plain) == len(proof) and plain != proof
    assert PR.verify_proof_multi(opk, inst, plain, transcript=transcript)
    with pytest.raises(AssertionError):
        PR.verify_proof_multi(opk, inst, proof, transcript=transcript)
    # a wrong challenge value is rejected by the wrapped verifier, and so is a proof made for one
    with pytest.raises(AssertionError):
        PO.verify_proof(monkeypatch, opk, desc, inst, proof, [ch[0] + 1], transcript=transcript)
    with pytest.raises(AssertionError):
        PO.create_proof(monkeypatch, opk, desc, inst, adv, 4, [ch[0] + 1], transcript=transcript)
    # the harness leaves the oracle as it found it
    assert PR.create_proof_multi(opk, inst, adv, 4, transcript=transcript) == plain


def test_phased_draw_order_is_a_permutation_with_phase_zero_first(plonk):
    c, desc = phased_lookup_circuit(plonk)
    A, bf = desc["num_advice"], desc["blinding_factors"]
    for N in (1, 2, 3):
        order = PO.phased_positions(desc, N)
        assert sorted(order) == list(range(N * A * (bf + 2)))
        # instance 0, column 0, row 0 is the first draw in both orders; the phase-1 column's tails come after every
        # phase-0 draw of every instance
        assert order[0] == 0
        first_phase1 = order[(A - 1) * (bf + 1)]
        assert first_phase1 == N * (A - 1) * (bf + 2)
    one = dict(desc, advice_column_phase=[0] * A)
    assert PO.phased_positions(one, 1) == list(range(A * (bf + 2)))  # one phase, one instance: the oracle's own order


def prove_on_cpu(monkeypatch, c, N=1, seed=9, transcript="blake2b", multiopen="shplonk"):
    opk = PR.keygen(PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])), c.fixed, c.assembly.mapping, TAU, transcript_repr=77)
    wit = [(c.advice, c.fill)] + [c.witness_for(100 + i) for i in range(1, N)]
    adv, fills = [[list(col) for col in w[0]] for w in wit], [w[1] for w in wit]
    inst = [c.instances] * N
    ch = PO.synthesize_on_cpu(monkeypatch, opk, c.desc, inst, adv, fills, seed, transcript=transcript)
    proof = PO.create_proof(monkeypatch, opk, c.desc, inst, adv, seed, ch, transcript=transcript, multiopen=multiopen)
    return opk, inst, adv, ch, proof


@pytest.mark.parametrize("three,N,transcript,multiopen", [(False, 1, "blake2b", "shplonk"), (False, 2, "keccak", "gwc"), (True, 1, "blake2b", "shplonk"),
                                                          (True, 2, "blake2b", "shplonk"), (True, 1, "sha256", "shplonk")])
def test_rlc_circuit_proves_and_verifies_on_cpu(plonk, monkeypatch, three, N, transcript, multiopen):
    c = PC.rlc_circuit(plonk, 5, seed=2, three_phases=three)
    assert c.desc["advice_column_phase"] == ([0, 0, 1, 2] if three else [0, 0, 1]) and c.desc["challenge_phase"] == ([0, 1] if three else [0])
    opk, inst, adv, ch, proof = prove_on_cpu(monkeypatch, c, N=N, transcript=transcript, multiopen=multiopen)
    assert len(set(ch)) == len(ch)
    assert PO.verify_proof(monkeypatch, opk, c.desc, inst, proof, ch, transcript=transcript, multiopen=multiopen)
    with pytest.raises(AssertionError):
        PO.verify_proof(monkeypatch, opk, c.desc, inst, proof, [v + 1 for v in ch], transcript=transcript, multiopen=multiopen)


def test_rlc_witness_that_ignores_the_challenge_does_not_verify(plonk, monkeypatch):
    c = PC.rlc_circuit(plonk, 5, seed=2, ignore_challenge=True)
    opk, inst, adv, ch, proof = prove_on_cpu(monkeypatch, c)
    with pytest.raises(AssertionError):
        PO.verify_proof(monkeypatch, opk, c.desc, inst, proof, ch)


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_phased_circuits_prove_and_verify_on_cpu(plonk, monkeypatch, seed):
    c = PC.random_phased_circuit(plonk, 5, seed=seed)
    opk, inst, adv, ch, proof = prove_on_cpu(monkeypatch, c, seed=seed)
    assert PO.verify_proof(monkeypatch, opk, c.desc, inst, proof, ch)


def test_random_phased_circuits_cover_the_shapes(plonk):
    shapes = [PC.random_phased_circuit(plonk, 5, seed=s).desc for s in RANDOM_SEEDS]
    assert {max(d["advice_column_phase"]) for d in shapes} == {1, 2}
    assert {len(d["challenge_phase"]) for d in shapes} >= {1, 2, 3}
    assert any(d["lookups"] for d in shapes) and any(not d["lookups"] for d in shapes)
    assert any(d["permutation_columns"] for d in shapes)
    assert any(max(d["challenge_phase"]) == max(d["advice_column_phase"]) for d in shapes)  # a challenge behind the last phase


# ---- the Python mirror: ConstraintSystem::{advice_column_in, challenge_usable_after}, Expression::Challenge -------------
def test_mirror_validates_phases_like_upstream(plonk):
    cs = plonk.ConstraintSystem()
    with pytest.raises(ValueError, match="no advice column in phase 0, the one before phase 1"):
        cs.advice_column_in(1)
    with pytest.raises(ValueError, match="no advice column in phase 0"):
        cs.challenge_usable_after(0)
    cs.advice_column()
    with pytest.raises(ValueError, match="no advice column in phase 1, the one before phase 2"):
        cs.advice_column_in(2)
    with pytest.raises(ValueError, match="phases are 0, 1, 2"):
        cs.advice_column_in(3)
    with pytest.raises(ValueError, match="no advice column in phase 1"):
        cs.challenge_usable_after(1)
    ch = cs.challenge_usable_after(0)
    cs.advice_column_in(1)
    assert (ch.index, ch.phase) == (0, 0) and cs.challenge_usable_after(1).index == 1


def test_mirror_challenge_has_degree_zero_and_flattens_to_word_9(plonk):
    c = PC.rlc_circuit(plonk, 5, three_phases=True)
    E = plonk.Expression
    assert E.challenge(1).degree() == 0 and (E.challenge(1) * E("advice", 0, 0)).degree() == 1
    assert c.desc["cs_degree"] == 4  # the lookup's 2 + 1 + 1; the gates have degree 2 with the challenges free
    cc, arrs = plonk.flatten_circuit(c.desc)
    chal_words = [int(w) for w in arrs["words"] if int(w) >> 24 == 9]
    assert sorted(set(w & 0xFFFFFF for w in chal_words)) == [0, 1] and len(chal_words) == 1 + 2 + 2
    ph, keep = plonk.flatten_phases(c.desc)
    assert ph.num_challenges == 2 and list(keep[0]) == [0, 0, 1, 2] and list(keep[1]) == [0, 1]
    # a phase-0 circuit keeps the description (and the entry point) it always had
    plain = circuits.lookup_circuit(plonk, 5, seed=1)
    assert "advice_column_phase" not in plain.desc and plonk.flatten_phases(plain.desc) == (None, None)
