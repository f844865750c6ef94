"""Harness that pins the ORDER of a create_proof with challenge phases, without touching oracle/.

oracle/plonk_ref.py is phase 0 only: it blinds and commits every advice column of an instance, instance after instance,
and squeezes theta. Upstream's create_proof at the pin loops over the phases OUTSIDE the loop over the circuits:

    for each phase p, for each circuit instance:
        the instance's columns of phase p, in column-index order, get their bf + 1 blinding tails
        one unused blind is drawn per column of the phase
        the columns are committed and the commitments written
    after all instances: one squeeze_challenge per challenge whose phase is p, in challenge-index order
    theta follows the last phase

The harness drives the unmodified oracle through three substitutions on its module-level names (monkeypatch.setattr):
  * a transcript writer that buffers the N * A advice points the oracle writes (instance-major) and replays them phase-major
    with the phase's squeezes in between, before theta; a reader that does the inverse;
  * a ChaCha20Rng that serves the first N * A * (bf + 2) draws re-indexed from the phased order above into the oracle's;
  * the description SPECIALISED to the challenges: each ("challenge", i) becomes ("const", value). The values the wrapped
    transcript squeezes are recorded, and every entry point here asserts that they are the values the description was
    specialised to — a proof is only "the phased proof" if the two agree.
The circuits used with it have their advice columns ordered by phase (the harness relies on it; the library does not).
"""
import copy
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402

R = PR.R
# transcript name -> (the oracle's module-level names to replace, the writer / reader classes to wrap). The oracle takes
# Blake2b for "blake2b" and its Keccak256 pair for any other name: a third transcript goes in under those names.
_ORIG = {name: getattr(PR, name) for name in ("Blake2bWrite", "Blake2bRead", "Keccak256Write", "Keccak256Read")}
WRITERS = {"blake2b": ("Blake2bWrite", "Blake2bRead", PR.Blake2bWrite, PR.Blake2bRead),
           "keccak": ("Keccak256Write", "Keccak256Read", PR.Keccak256Write, PR.Keccak256Read)}
_ORIG_RNG = PR.ChaCha20Rng


class ChallengesKnown(Exception):
    """Raised by a probing writer once the challenges of the phase asked for have been squeezed."""

    def __init__(self, squeezed):
        self.squeezed = squeezed


def layout(desc):
    ap, cp = list(desc["advice_column_phase"]), list(desc["challenge_phase"])
    assert ap == sorted(ap), "the harness needs advice columns ordered by phase"
    return ap, cp, max(ap) + 1


def specialise(desc, values):
    """The description with ("challenge", i) replaced by ("const", values[i]) and without its phase table."""
    def sub(e):
        if e[0] == "challenge":
            return ("const", values[e[1]] % R)
        return tuple(sub(x) if isinstance(x, tuple) else x for x in e)
    out = {k: v for k, v in desc.items() if k not in ("advice_column_phase", "challenge_phase")}
    out["gates"] = [sub(g) for g in desc["gates"]]
    out["lookups"] = [{"inputs": [sub(e) for e in lk["inputs"]], "tables": [sub(e) for e in lk["tables"]]} for lk in desc["lookups"]]
    return out


def phased_positions(desc, N):
    """For the oracle's j-th advice draw, its position in upstream's phased draw order (both orders as stated above)."""
    ap, _, nph = layout(desc)
    A, bf = desc["num_advice"], desc["blinding_factors"]
    pos, idx = {}, 0
    for p in range(nph):
        cols = [c for c in range(A) if ap[c] == p]
        for ci in range(N):
            for c in cols:
                for i in range(bf + 1):
                    pos[("tail", ci, c, i)] = idx
                    idx += 1
            for c in cols:
                pos[("blind", ci, c)] = idx
                idx += 1
    assert idx == N * A * (bf + 2)
    order = []
    for ci in range(N):
        order += [pos[("tail", ci, c, i)] for c in range(A) for i in range(bf + 1)]
        order += [pos[("blind", ci, c)] for c in range(A)]
    return order


def install(monkeypatch, desc, N, transcript, squeezed, stop_after=None):
    """Replace the oracle's writer, reader and RNG by the phased ones. `squeezed` receives (challenge index, value)."""
    ap, cp, nph = layout(desc)
    A = desc["num_advice"]
    wname, rname, WBase, RBase = WRITERS[transcript]

    def phase_major(emit, squeeze):
        for p in range(nph):
            for ci in range(N):
                for c in range(A):
                    if ap[c] == p:
                        emit(ci, c)
            for i, ph in enumerate(cp):
                if ph == p:
                    squeezed.append((i, squeeze()))
            if stop_after == p:
                raise ChallengesKnown(list(squeezed))

    class Write(WBase):
        def __init__(self):
            super().__init__()
            self._buf = []

        def write_point(self, p):
            if self._buf is None:
                return WBase.write_point(self, p)
            self._buf.append(p)
            if len(self._buf) == N * A:
                buf, self._buf = self._buf, None
                phase_major(lambda ci, c: WBase.write_point(self, buf[ci * A + c]), lambda: WBase.squeeze_challenge(self))

    class Read(RBase):
        def __init__(self, proof):
            super().__init__(proof)
            self._queue = None

        def read_point(self):
            if self._queue is None:
                got = {}
                self._queue = []
                phase_major(lambda ci, c: got.__setitem__((ci, c), RBase.read_point(self)), lambda: RBase.squeeze_challenge(self))
                self._queue = [got[(ci, c)] for ci in range(N) for c in range(A)]
            if self._queue:
                return self._queue.pop(0)
            return RBase.read_point(self)

    order = phased_positions(desc, N)

    class Rng(_ORIG_RNG):
        def __init__(self, seed):
            super().__init__(seed)
            drawn = [_ORIG_RNG.fr(self) for _ in order]  # upstream's order
            self._pre = [drawn[j] for j in order]          # served in the oracle's

        def fr(self):
            return self._pre.pop(0) if self._pre else _ORIG_RNG.fr(self)

    monkeypatch.setattr(PR, wname, Write)
    monkeypatch.setattr(PR, rname, Read)
    monkeypatch.setattr(PR, "ChaCha20Rng", Rng)


def uninstall(monkeypatch):
    for name, cls in _ORIG.items():
        monkeypatch.setattr(PR, name, cls)
    monkeypatch.setattr(PR, "ChaCha20Rng", _ORIG_RNG)


def _with_desc(opk, desc):
    k = copy.copy(opk)
    k.desc = desc
    return k


def check_squeezed(squeezed, challenges):
    got = dict(squeezed)
    assert sorted(got) == list(range(len(challenges))) and len(squeezed) == len(challenges), "not every challenge was squeezed once"
    for i, v in enumerate(challenges):
        assert got[i] == v % R, "challenge %d: the transcript squeezes %x, the description was specialised to %x" % (i, got[i], v % R)


def create_proof(monkeypatch, opk, desc, instances_list, advice_list, seed, challenges, transcript="blake2b", multiopen="shplonk"):
    """The expected bytes of the phased proof: the wrapped oracle's proof of `desc` specialised to `challenges`; asserts
    that the wrapped transcript squeezes exactly those values."""
    squeezed = []
    install(monkeypatch, desc, len(instances_list), transcript, squeezed)
    try:
        proof = PR.create_proof_multi(_with_desc(opk, specialise(desc, challenges)), instances_list, advice_list, seed,
                                      transcript=transcript, multiopen=multiopen)
    finally:
        uninstall(monkeypatch)
    check_squeezed(squeezed, challenges)
    return proof


def probe(monkeypatch, opk, desc, instances_list, advice_list, seed, known, phase, transcript="blake2b"):
    """The challenges squeezed up to and including `phase`, given advice that is final for the phases <= phase (later
    columns may hold anything: their commitments are written after the squeeze). `known`: challenges so far, by index."""
    squeezed = []
    install(monkeypatch, desc, len(instances_list), transcript, squeezed, stop_after=phase)
    values = [known.get(i, 0) for i in range(len(desc["challenge_phase"]))]
    try:
        PR.create_proof_multi(_with_desc(opk, specialise(desc, values)), instances_list, advice_list, seed, transcript=transcript)
    except ChallengesKnown as e:
        return dict(e.squeezed)
    finally:
        uninstall(monkeypatch)
    raise AssertionError("the oracle finished without reaching the end of phase %d" % phase)


def synthesize_on_cpu(monkeypatch, opk, desc, instances_list, advice_list, fills, seed, transcript="blake2b"):
    """What the device's phase callback does, on the CPU: fills[ci](phase, challenges by index, advice) assigns instance
    ci's columns of `phase` in place. Returns the challenges in index order."""
    _, cp, nph = layout(desc)
    known = {}
    for p in range(nph):
        if p > 0:
            for ci, fill in enumerate(fills):
                fill(p, dict(known), advice_list[ci])
        known = probe(monkeypatch, opk, desc, instances_list, advice_list, seed, known, p, transcript=transcript)
    return [known[i] for i in range(len(cp))]


def verify_proof(monkeypatch, vk, desc, instances_list, proof, challenges, transcript="blake2b", multiopen="shplonk"):
    """The wrapped verifier: the oracle's checks on `desc` specialised to `challenges`, reading the advice commitments
    phase-major, and the assertion that the reader squeezes those challenges. Raises AssertionError otherwise."""
    squeezed = []
    install(monkeypatch, desc, len(instances_list), transcript, squeezed)
    try:
        ok = PR.verify_proof_multi(_with_desc(vk, specialise(desc, challenges)), instances_list, proof, transcript=transcript, multiopen=multiopen)
    finally:
        uninstall(monkeypatch)
    check_squeezed(squeezed, challenges)
    return ok


# ---- a third transcript, for the caller-owned-transcript tests: SHA-256 with its own framing -------------------------
class Sha256Write:
    """Not a halo2 transcript: state = SHA-256 chain; a point is absorbed as b"P" | x (32 BE) | y (32 BE) and written as
    64 bytes; a scalar as b"S" | 32 BE; a challenge is SHA-256(state | b"C" | counter) widened with a second block."""

    def __init__(self):
        self.state = b"phased-test-transcript".ljust(32, b"\0")
        self.proof = bytearray()
        self.count = 0

    def _absorb(self, data):
        self.state = hashlib.sha256(self.state + data).digest()

    def squeeze_challenge(self):
        self.count += 1
        tag = b"C" + self.count.to_bytes(4, "big")
        wide = hashlib.sha256(self.state + tag + b"\0").digest() + hashlib.sha256(self.state + tag + b"\1").digest()
        self._absorb(tag)
        return int.from_bytes(wide, "big") % R

    def common_point(self, p):
        assert p is not None, "cannot write points at infinity to the transcript"
        self._absorb(b"P" + p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big"))

    def common_scalar(self, s):
        self._absorb(b"S" + (s % R).to_bytes(32, "big"))

    def write_point(self, p):
        self.common_point(p)
        self.proof += p[0].to_bytes(32, "big") + p[1].to_bytes(32, "big")

    def write_scalar(self, s):
        self.common_scalar(s)
        self.proof += (s % R).to_bytes(32, "big")


class Sha256Read(Sha256Write):
    def __init__(self, proof):
        super().__init__()
        self.data, self.pos = bytes(proof), 0

    def read_point(self):
        x, y = int.from_bytes(self.data[self.pos:self.pos + 32], "big"), int.from_bytes(self.data[self.pos + 32:self.pos + 64], "big")
        self.pos += 64
        assert x < PR.Q and y < PR.Q and y * y % PR.Q == (x * x * x + 3) % PR.Q, "point not on curve"
        self.common_point((x, y))
        return (x, y)

    def read_scalar(self):
        s = int.from_bytes(self.data[self.pos:self.pos + 32], "big")
        self.pos += 32
        assert s < R
        self.common_scalar(s)
        return s


WRITERS["sha256"] = ("Keccak256Write", "Keccak256Read", Sha256Write, Sha256Read)
