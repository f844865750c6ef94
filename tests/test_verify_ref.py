"""CPU: tests/verify_ref.py, the reference the verifier tests compare with, against the oracle's own verifier: tau * L == R
holds exactly when oracle/plonk_ref.py's verify_proof* accepts — on valid proofs and on mutated ones of the hand-written
circuits, with both transcripts and both openings — and L and R of an accepted proof are not the identity (a pair of
identities would pass every tau check). The reference decode agrees with the oracle's readers on what is malformed."""
import random

import pytest

import verify_cases as VC
import verify_ref as VR


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def mutations(case, seed, count):
    """Single-byte mutations at fixed seeds, spread over the proof."""
    rnd = random.Random(seed)
    out = []
    for _ in range(count):
        m = bytearray(case.proof)
        i = rnd.randrange(len(m))
        m[i] ^= 1 << rnd.randrange(8)
        out.append(bytes(m))
    return out


@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_valid_proofs_satisfy_the_pair_and_neither_side_is_the_identity(plonk, name, N, transcript, multiopen):
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    assert case.accepts()
    assert case.decode() == (VR.WELL_FORMED, 0)
    L, Rr = case.pair()
    assert L is not None and Rr is not None
    assert VR.holds((L, Rr), VC.TAU)
    assert not VR.holds((L, Rr), VC.TAU + 1)


MUTATED = ([("square", 1) + k for k in VC.KINDS] + [("lookup", 1) + k for k in VC.KINDS] + [("lookup", 2) + VC.KINDS[3]] +
           [("rlc", 1) + VC.KINDS[0], ("rlc", 1) + VC.KINDS[1]])


@pytest.mark.parametrize("name,N,transcript,multiopen", MUTATED)
def test_the_pair_holds_exactly_when_the_oracle_accepts_mutated_proofs(plonk, name, N, transcript, multiopen):
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    seen = {"malformed": 0, "rejected": 0}
    for m in mutations(case, 1000 + N, 8):
        status = case.decode(m)[0]
        if status != VR.WELL_FORMED:
            assert not case.accepts(m)
            seen["malformed"] += 1
            continue
        ok = VR.holds(case.pair(m), VC.TAU)
        assert ok == case.accepts(m)
        seen["rejected"] += not ok
    assert seen["malformed"] + seen["rejected"] == 8, seen  # every bit of a proof matters: none of them leaves it valid
    # wrong public inputs: well formed, rejected
    if any(case.c.instances):
        bad = [[list(col) for col in inst] for inst in case.instances_list]
        j = next(i for i, col in enumerate(bad[0]) if col)
        bad[0][j][0] = (bad[0][j][0] + 1) % VR.R
        assert not case.accepts(instances_list=bad) and not VR.holds(case.pair(instances_list=bad), VC.TAU)


def test_reference_decode_classes(plonk):
    for transcript in ("blake2b", "evm"):
        case = VC.cpu_case(plonk, "square", 1, transcript, "shplonk")
        kinds = VR.element_kinds(case.desc, 1)
        psz = 64 if transcript == "evm" else 32
        first_scalar = kinds.index("s") * psz
        big = "big" if transcript == "evm" else "little"
        m = bytearray(case.proof)
        m[first_scalar:first_scalar + 32] = VR.R.to_bytes(32, big)
        assert case.decode(bytes(m)) == (VR.BAD_SCALAR, first_scalar) and not case.accepts(bytes(m))
        m[first_scalar:first_scalar + 32] = (VR.R - 1).to_bytes(32, big)
        assert case.decode(bytes(m)) == (VR.WELL_FORMED, 0)
        m = bytearray(case.proof)
        m[psz:psz + 32] = VR.Q.to_bytes(32, big)
        assert case.decode(bytes(m)) == (VR.BAD_POINT, psz) and not case.accepts(bytes(m))
        m[psz:2 * psz] = bytes(psz)
        assert case.decode(bytes(m)) == (VR.BAD_POINT, psz)
        assert case.decode(case.proof[:-1]) == (VR.BAD_LENGTH, 0) and case.decode(case.proof[:32]) == (VR.BAD_LENGTH, 0)
        assert case.decode(instances_list=[[[VR.R]] * len(case.c.instances)])[0] == VR.BAD_INSTANCE
