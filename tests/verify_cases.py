"""Shared by the verifier tests (CPU and GPU): the small circuits amdzk_verify_proofs is pinned on, proofs of them made by
the CPU oracle, the proof elements decoded in Python integers, and the input file of tests/native/verifier_check.cpp.
Everything is made once per process and never modified."""
import os
import struct
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import phased_circuits as PC  # noqa: E402
import phased_oracle as PO  # noqa: E402
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402
import verify_ref as VR  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
Q, R = zu.Q, zu.R
# random_circuit seeds at k = 6: between them instance queries (all but 11), negative rotations (all) and 0 (16), 1 (11, 12,
# 14, 17), 2 (10, 13) and 3 (4) lookups
RANDOM_SEEDS = [4, 10, 11, 12, 13, 14, 16, 17]
KINDS = [("blake2b", "shplonk"), ("evm", "shplonk"), ("blake2b", "gwc"), ("evm", "gwc")]


def kind_flags(plonk, transcript, multiopen):
    return (plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM) | (plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0)


def po_name(transcript):
    """The phased harness's name of a transcript."""
    return "blake2b" if transcript == "blake2b" else "keccak"


def circuit(plonk, name):
    if name == "square":
        return circuits.square_circuit(plonk, 4)
    if name == "lookup":
        return circuits.lookup_circuit(plonk, 5, seed=2)
    if name == "high_degree":
        return circuits.high_degree_circuit(plonk, 5)
    if name == "rlc":
        return PC.rlc_circuit(plonk, 5, seed=1)
    assert name.startswith("random")
    return circuits.random_circuit(plonk, 6, int(name[6:]))


# (circuit, instances per proof, [(transcript, opening)]): every circuit with both transcripts and both openings somewhere
CASES = ([("square", 1, KINDS), ("lookup", 1, KINDS), ("high_degree", 1, [KINDS[0], KINDS[3]]), ("lookup", 2, [KINDS[0], KINDS[3]]),
          ("rlc", 1, [KINDS[0], KINDS[1], KINDS[2]])] +
         [("random%d" % s, 1, [KINDS[i % 4], KINDS[(i + 3) % 4]]) for i, s in enumerate(RANDOM_SEEDS)])
CASE_IDS = [(name, N, tr, mo) for name, N, kinds in CASES for tr, mo in kinds]


class Case:
    """One proof: the circuit, the oracle key `opk` to verify it with (for a phased circuit: of the description specialised
    to the squeezed `challenges`, and `desc` keeps the challenge words), the public inputs and the bytes."""

    def __init__(self, name, c, desc, opk, instances_list, proof, transcript, multiopen, challenges):
        self.name, self.c, self.desc, self.opk, self.instances_list, self.proof = name, c, desc, opk, instances_list, bytes(proof)
        self.transcript, self.multiopen, self.challenges, self.N = transcript, multiopen, challenges, len(instances_list)

    def accepts(self, proof=None, instances_list=None):
        """The oracle's verify_proof* (through the phased harness for a phased key)."""
        proof = self.proof if proof is None else proof
        inst = self.instances_list if instances_list is None else instances_list
        try:
            if self.challenges is None:
                return bool(PR.verify_proof_multi(self.opk, inst, proof, transcript=self.transcript, multiopen=self.multiopen))
            with pytest.MonkeyPatch.context() as mp:
                return bool(PO.verify_proof(mp, self.opk, self.desc, inst, proof, self.challenges, transcript=po_name(self.transcript), multiopen=self.multiopen))
        except (AssertionError, IndexError, ValueError, KeyError):
            return False

    def pair(self, proof=None, instances_list=None):
        proof = self.proof if proof is None else proof
        inst = self.instances_list if instances_list is None else instances_list
        if self.challenges is None:
            return VR.pair(self.opk, inst, proof, transcript=self.transcript, multiopen=self.multiopen)
        with pytest.MonkeyPatch.context() as mp:
            return VR.pair_phased(mp, self.opk, self.desc, inst, proof, self.challenges, transcript=po_name(self.transcript), multiopen=self.multiopen)

    def decode(self, proof=None, instances_list=None):
        return VR.decode(self.desc, self.N, self.instances_list if instances_list is None else instances_list,
                         self.proof if proof is None else proof, transcript=self.transcript, multiopen=self.multiopen)


_circuits, _keys, _cases = {}, {}, {}


def oracle_key(plonk, name):
    if name not in _keys:
        c = _circuits.setdefault(name, circuit(plonk, name))
        odesc = PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])) if "challenge_phase" in c.desc else c.desc
        _keys[name] = (c, PR.keygen(odesc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR))
    return _keys[name]


def cpu_case(plonk, name, N, transcript, multiopen, seed=5):
    """The case with its proof made by the CPU oracle."""
    key = (name, N, transcript, multiopen, seed)
    if key not in _cases:
        import plonk_fast as PF
        c, opk = oracle_key(plonk, name)
        inst = [c.instances] * N
        if "challenge_phase" in c.desc:
            with pytest.MonkeyPatch.context() as mp:
                adv = [[list(col) for col in c.advice] for _ in range(N)]
                ch = PO.synthesize_on_cpu(mp, opk, c.desc, inst, adv, [c.fill] * N, seed, transcript=po_name(transcript))
                proof = PO.create_proof(mp, opk, c.desc, inst, adv, seed, ch, transcript=po_name(transcript), multiopen=multiopen)
        else:
            ch = None
            if N == 1 and multiopen == "shplonk":  # the C++-backed prover: same bytes (tests/test_oracle_plonk.py)
                proof = PF.create_proof(PF.FastKey(c.desc, c.fixed, c.assembly.mapping, TAU, REPR), c.instances, c.advice, seed=seed, transcript=transcript)
            else:
                proof = PR.create_proof_multi(opk, inst, [c.advice] * N, seed, transcript=transcript, multiopen=multiopen)
        _cases[key] = Case(name, c, c.desc, opk, inst, proof, transcript, multiopen, ch)
    return _cases[key]


# ------------------------------------------------------------------------------------ decoded elements, in integers
def decoded_elements(case, proof=None):
    """(points, scalars) of a WELL-FORMED proof in read order: affine (x, y) and integers."""
    proof = case.proof if proof is None else proof
    evm = case.transcript != "blake2b"
    pts, scs, off = [], [], 0
    for k in VR.element_kinds(case.desc, case.N, case.multiopen):
        if k == "p" and evm:
            pts.append((int.from_bytes(proof[off:off + 32], "big"), int.from_bytes(proof[off + 32:off + 64], "big")))
            off += 64
        elif k == "p":
            b = bytearray(proof[off:off + 32])
            sign = b[31] >> 7
            b[31] &= 0x7F
            x = int.from_bytes(b, "little")
            y = pow((x * x * x + 3) % Q, (Q + 1) // 4, Q)
            pts.append((x, y if (y & 1) == sign else Q - y))
            off += 32
        else:
            scs.append(int.from_bytes(proof[off:off + 32], "big" if evm else "little"))
            off += 32
    assert off == len(proof)
    return pts, scs


def bases(case, points):
    """The bases of the host half's table: the proof's points, the fixed and the permutation commitments, G."""
    return list(points) + list(case.opk.fixed_commitments) + list(case.opk.permutation_commitments) + [P.G1_GEN]


def fold_table(case, points, table):
    """table: [(base index, L scalar, R scalar)] -> (L, R) with the oracle's G1 arithmetic."""
    bs = bases(case, points)
    L = Rr = None
    for i, ls, rs in table:
        if ls:
            L = P.g1_add(L, P.g1_mul(bs[i], ls))
        if rs:
            Rr = P.g1_add(Rr, P.g1_mul(bs[i], rs))
    return L, Rr


def write_case_file(path, case, rho=1, proof=None):
    """Input of tests/native/verifier_check.cpp, little-endian: N u32 | transcript_kind u32 | omega, rho (4 x u64, Montgomery) |
    per circuit and instance column: len u32, values | NP u32, points 8 x u64 | NS u32, scalars 4 x u64."""
    pts, scs = decoded_elements(case, proof)
    kind = (0 if case.transcript == "blake2b" else 1) | (0x100 if case.multiopen == "gwc" else 0)
    fr = lambda v: np.ascontiguousarray(zu.fr_from_int(v), dtype="<u8").tobytes()
    out = [struct.pack("<II", case.N, kind), fr(case.opk.domain.omega), fr(rho)]
    for instances in case.instances_list:
        for col in instances:
            out.append(struct.pack("<I", len(col)) + b"".join(fr(v) for v in col))
    out.append(struct.pack("<I", len(pts)) + b"".join(np.ascontiguousarray(zu.point_from_ints(p), dtype="<u8").tobytes() for p in pts))
    out.append(struct.pack("<I", len(scs)) + b"".join(fr(v) for v in scs))
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return pts
