"""Provers and verifiers at degenerate caller-chosen challenges: the cases, and what the REFERENCE does with each.

A case is a script (tests/scripted_transcript.py) for the proof of verify_cases' "lookup" circuit (k = 5: gates, two lookups, a
permutation) with proof seed 3. Squeeze indices of a phase-0 key: 0 theta, 1 beta, 2 gamma, 3 y, 4 x; SHPLONK then 5 y', 6 v,
7 u; GWC 5 v and — on the reader only — 6 u. outcome() runs oracle/plonk_ref.py alone under the script and returns the case's
class — PROVES (and the verifier accepts), VERIFIER_RAISES, PROVER_RAISES — with the proof bytes; results are kept per
process, so tests/test_scripted_oracle.py (which asserts the classes stated in cases() against the reference) and the GPU tests
(which take their expectations from outcome() and from nowhere else) pay for each oracle run once."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import phased_circuits as PC  # noqa: E402
import phased_oracle as PO  # noqa: E402
import plonk_ref as PR  # noqa: E402
import scripted_transcript as ST  # noqa: E402
import verify_cases as VC  # noqa: E402

R = PR.R
SEED = 3
PROVES, VERIFIER_RAISES, PROVER_RAISES = "proves and verifies", "proves, the verifier raises", "the prover raises"
TH, BE, GA, Y, X = range(5)


def omega(plonk):
    return VC.oracle_key(plonk, "lookup")[1].domain.omega


def script(multiopen, theta=None, beta=None, gamma=None, y=None, x=None, yp=None, v=None, u=None):
    """{squeeze index: value} of the named challenges for the opening scheme (GWC has no y'; its u is the reader's)."""
    named = {TH: theta, BE: beta, GA: gamma, Y: y, X: x}
    named.update({5: yp, 6: v, 7: u} if multiopen == "shplonk" else {5: v, 6: u})
    return {i: s for i, s in named.items() if s is not None}


def x_times(w, rot):
    """u = x * omega^rot, whatever x was squeezed."""
    return lambda squeezed: squeezed[X] * pow(w, rot, R) % R


def cases(plonk):
    """name -> (keyword arguments of script(), the class stated for SHPLONK, for GWC). u = x w^rot: the rotations of this
    circuit's queries, of which only 0 is in SHPLONK's first point set."""
    w = omega(plonk)
    bf = VC.oracle_key(plonk, "lookup")[0].desc["blinding_factors"]
    every = lambda val: dict(theta=val, beta=val, gamma=val, y=val, x=val, yp=val, v=val, u=val)
    return {
        "theta=0": (dict(theta=0), PROVES, PROVES),
        "theta=1": (dict(theta=1), PROVES, PROVES),
        "beta=0": (dict(beta=0), PROVES, PROVES),
        "gamma=0": (dict(gamma=0), PROVES, PROVES),
        "beta=gamma=0": (dict(beta=0, gamma=0), PROVES, PROVES),
        "y=1": (dict(y=1), PROVES, PROVES),
        "y'=0": (dict(yp=0), PROVES, PROVES),
        "v=0": (dict(v=0), PROVES, PROVES),
        "y'=v=0": (dict(yp=0, v=0), PROVES, PROVES),
        "y'=v=1": (dict(yp=1, v=1), PROVES, PROVES),
        "all=12345": (every(12345), PROVES, PROVES),
        "theta=beta=gamma=y=x": (dict(theta=777, beta=777, gamma=777, y=777, x=777), PROVES, PROVES),
        "x=0": (dict(x=0), PROVES, PROVES),
        "x=1": (dict(x=1), VERIFIER_RAISES, VERIFIER_RAISES),
        "x=w^3": (dict(x=pow(w, 3, R)), VERIFIER_RAISES, VERIFIER_RAISES),
        "all=r-1": (every(R - 1), VERIFIER_RAISES, VERIFIER_RAISES),
        "y=0": (dict(y=0), PROVER_RAISES, PROVER_RAISES),
        "u=x": (dict(x=7, u=x_times(w, 0)), PROVES, PROVES),
        "u=xw": (dict(x=7, u=x_times(w, 1)), PROVER_RAISES, PROVES),
        "u=xw^-1": (dict(x=7, u=x_times(w, -1)), PROVER_RAISES, PROVES),
        "u=xw^-(bf+1)": (dict(x=7, u=x_times(w, -(bf + 1))), PROVER_RAISES, PROVES),
    }


# What the GPU tests call legal: the reference proves and verifies, and the device is asked for the same bytes. Not these:
# the reference proves them; the device refuses them by name: beta = 0 (its factored permutation terms; beta = gamma = 0 is
# a beta = 0) and x = 0 (its opening plan)
PINNED = ("beta=0", "beta=gamma=0", "x=0")
KECCAK = ("theta=0", "y'=v=0", "all=12345")
TWO_INSTANCES = ("y'=v=0", "u=x")
_RAISES = (AssertionError, ValueError, ZeroDivisionError)
_outcomes = {}


def outcome(plonk, name, multiopen="shplonk", transcript="blake2b", N=1):
    """(class, proof bytes or None, the exception's text or None) of the reference under the case's script."""
    key = (name, multiopen, transcript, N)
    if key not in _outcomes:
        c, opk = VC.oracle_key(plonk, "lookup")
        sc = script(multiopen, **cases(plonk)[name][0])
        with pytest.MonkeyPatch.context() as mp, ST.installed(mp, transcript, sc):
            try:
                proof = PR.create_proof_multi(opk, [c.instances] * N, [c.advice] * N, SEED, transcript=transcript, multiopen=multiopen)
            except _RAISES as e:
                _outcomes[key] = (PROVER_RAISES, None, repr(e))
                return _outcomes[key]
            try:
                ok = PR.verify_proof_multi(opk, [c.instances] * N, proof, transcript=transcript, multiopen=multiopen)
                assert ok, "the reference's verifier returned false on its own proof"
                _outcomes[key] = (PROVES, bytes(proof), None)
            except _RAISES as e:
                _outcomes[key] = (VERIFIER_RAISES, bytes(proof), repr(e))
    return _outcomes[key]


def unscripted(plonk, multiopen="shplonk", transcript="blake2b", seed=SEED):
    key = ("", multiopen, transcript, seed)
    if key not in _outcomes:
        c, opk = VC.oracle_key(plonk, "lookup")
        _outcomes[key] = bytes(PR.create_proof(opk, c.instances, c.advice, seed=seed, transcript=transcript, multiopen=multiopen))
    return _outcomes[key]


# ---- one phased circuit: rlc_circuit, three phases (two challenges, squeezes 0 and 1; theta is squeeze 2) ----------------
PHASED = {"phase challenges 0": (0, 0), "phase challenges equal": (4242, 4242)}
_phased = {}


def phased_circuit(plonk, k=6):
    if k not in _phased:
        c = PC.rlc_circuit(plonk, k, seed=4, three_phases=True)
        opk = PR.keygen(PO.specialise(c.desc, [0, 0]), c.fixed, c.assembly.mapping, VC.TAU, transcript_repr=VC.REPR)
        _phased[k] = (c, opk)
    return _phased[k]


def phased_outcome(plonk, name, multiopen="shplonk", k=6):
    """(proof bytes, challenges) of the phased harness under the script; raises if the reference does not prove and verify."""
    key = (name, multiopen, k)
    if key not in _phased:
        c, opk = phased_circuit(plonk, k)
        ch = list(PHASED[name])
        adv = [list(col) for col in c.advice]
        for phase in (1, 2):
            c.fill(phase, dict(enumerate(ch)), adv)
        with pytest.MonkeyPatch.context() as mp, ST.phased("blake2b", dict(enumerate(ch))) as tname:
            proof = PO.create_proof(mp, opk, c.desc, [c.instances], [adv], SEED, ch, transcript=tname, multiopen=multiopen)
            assert PO.verify_proof(mp, opk, c.desc, [c.instances], proof, ch, transcript=tname, multiopen=multiopen)
        _phased[key] = (bytes(proof), ch)
    return _phased[key]
