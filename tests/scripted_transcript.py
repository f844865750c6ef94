"""The oracle's transcripts with chosen squeezes replaced: "squeeze number i gives this value".

Since the caller-owned transcripts a challenge is an INPUT of the library, so the tests have to be able to choose one. A
script is {squeeze index: value}; squeezes are counted from 0 per transcript object. The hash absorbs and squeezes as
usual — only the value handed out changes — so everything written afterwards stays a function of the script and of the
witness, and a writer and a reader under the same script squeeze the same values from the same proof.

A script value is
  * an int (taken mod r),
  * a callable of the list of values squeezed so far (ints), for "u = x * omega^rot" without fixing x, or
  * Raw(v): the 256-bit words of v, which need not be below r. Only the device wrappers hand these out; the oracle, which
    computes in integers mod r, refuses to squeeze one.

install() / uninstall() put the scripted classes under oracle/plonk_ref.py's module-level names the way tests/phased_oracle.py
does (monkeypatch, restored in `finally`); installed() is both as a context manager. phased() registers the scripted pair
with tests/phased_oracle.py under a transcript name of its own, so that the phased harness wraps it like any other.
DeviceWriter / DeviceReader wrap an oracle transcript for the library's callbacks (Montgomery words at the boundary), as
the ForwardedTranscript classes of the GPU tests do."""
import contextlib
import os
import sys

import numpy as np
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import phased_oracle as PO  # noqa: E402
import plonk_ref as PR  # noqa: E402

R = PR.R
_NAMES = {"blake2b": ("Blake2bWrite", "Blake2bRead"), "keccak": ("Keccak256Write", "Keccak256Read")}
_ORIG = {name: getattr(PR, name) for pair in _NAMES.values() for name in pair}


class Raw:
    """256-bit words as they are: a value the callback hands to the library unreduced."""

    def __init__(self, value):
        assert 0 <= value < 1 << 256
        self.value = value

    def words(self):
        return np.array(zu.limbs(self.value), dtype=np.uint64)


def kind(transcript):
    """"blake2b", or "keccak" for every other name (the oracle's own rule; the verifier tests say "evm")."""
    return "blake2b" if transcript == "blake2b" else "keccak"


def scripted(base, script):
    """`base` (an oracle writer or reader class) with squeeze number i replaced by script[i]. Instances keep `squeezed`
    (the values handed out, ints) and `last_raw` (the Raw of the last squeeze, if it was one and `allow_raw` is set)."""
    class Scripted(base):
        allow_raw = False

        def squeeze_challenge(self):
            hashed = base.squeeze_challenge(self)
            done = self.__dict__.setdefault("squeezed", [])
            self.last_raw = None
            s = script.get(len(done), hashed)
            if callable(s):
                s = s(list(done))
            if isinstance(s, Raw):
                assert self.allow_raw, "raw words are for the device wrappers: the oracle computes with residues"
                self.last_raw, s = s, s.value
            done.append(s % R)
            return s % R
    Scripted.__name__ = "Scripted" + base.__name__
    return Scripted


def recording(base, log):
    """`base` (an oracle writer class) that also appends every call it receives to `log`, as (name, value): the call list of
    the oracle's prover when the oracle constructs it, of the library when its callbacks feed it (DeviceWriter and the
    ForwardedTranscript classes of the GPU tests)."""
    class Recording(base):
        _nested = False  # a writer's write_* absorbs through its own common_*: only the caller's call is one

        def _call(self, name, value, fn):
            outer, self._nested = not self._nested, True
            try:
                out = fn()
            finally:
                if outer:
                    self._nested = False
            if outer:
                log.append((name, out if name == "squeeze_challenge" else value))
            return out

        def common_point(self, p):
            return self._call("common_point", tuple(p), lambda: base.common_point(self, p))

        def common_scalar(self, s):
            return self._call("common_scalar", s % R, lambda: base.common_scalar(self, s))

        def write_point(self, p):
            return self._call("write_point", tuple(p), lambda: base.write_point(self, p))

        def write_scalar(self, s):
            return self._call("write_scalar", s % R, lambda: base.write_scalar(self, s))

        def squeeze_challenge(self):
            return self._call("squeeze_challenge", None, lambda: base.squeeze_challenge(self))
    Recording.__name__ = "Recording" + base.__name__
    return Recording


def writer(transcript, script):
    return scripted(_ORIG[_NAMES[kind(transcript)][0]], script)()


def reader(transcript, script, proof):
    return scripted(_ORIG[_NAMES[kind(transcript)][1]], script)(proof)


def install(monkeypatch, transcript, script):
    wname, rname = _NAMES[kind(transcript)]
    monkeypatch.setattr(PR, wname, scripted(_ORIG[wname], script))
    monkeypatch.setattr(PR, rname, scripted(_ORIG[rname], script))


def uninstall(monkeypatch):
    for name, cls in _ORIG.items():
        monkeypatch.setattr(PR, name, cls)


@contextlib.contextmanager
def installed(monkeypatch, transcript, script):
    install(monkeypatch, transcript, script)
    try:
        yield
    finally:
        uninstall(monkeypatch)


@contextlib.contextmanager
def phased(transcript, script):
    """The transcript name under which tests/phased_oracle.py wraps the scripted pair (its squeezes: the phase challenges
    first, in the harness's order, then theta ...). The oracle takes its Keccak names for every name but "blake2b"."""
    wname, rname = _NAMES[kind(transcript)]
    name = "scripted-" + kind(transcript)
    PO.WRITERS[name] = ("Keccak256Write", "Keccak256Read", scripted(_ORIG[wname], script), scripted(_ORIG[rname], script))
    try:
        yield name
    finally:
        del PO.WRITERS[name]


class DeviceWriter:
    """An oracle writer behind amdzk_transcript's callbacks. `multiopen`: the opening scheme's bit, read by plonk.create_proof."""

    def __init__(self, inner, multiopen=0):
        self.inner, self.multiopen, self.calls, self.squeezes = inner, multiopen, 0, 0
        inner.allow_raw = True

    def common_point(self, w):
        self.calls += 1
        self.inner.common_point(zu.point_to_ints(w))

    def write_point(self, w):
        self.calls += 1
        self.inner.write_point(zu.point_to_ints(w))

    def common_scalar(self, w):
        self.calls += 1
        self.inner.common_scalar(zu.fr_to_int(w))

    def write_scalar(self, w):
        self.calls += 1
        self.inner.write_scalar(zu.fr_to_int(w))

    def squeeze_challenge(self):
        self.calls += 1
        self.squeezes += 1
        v = self.inner.squeeze_challenge()
        raw = getattr(self.inner, "last_raw", None)
        return raw.words() if raw is not None else zu.fr_from_int(v)

    @property
    def proof(self):
        return bytes(self.inner.proof)


class DeviceReader:
    """An oracle reader behind amdzk_transcript_read's callbacks. order: "p" / "s" / "c" per completed call."""

    def __init__(self, inner):
        self.inner, self.order = inner, []
        inner.allow_raw = True

    def common_point(self, w):
        raise AssertionError("the verifier does not call common_point")

    def common_scalar(self, w):
        self.inner.common_scalar(zu.fr_to_int(w))

    def read_point(self):
        v = zu.point_from_ints(self.inner.read_point())
        self.order.append("p")
        return v

    def read_scalar(self):
        v = zu.fr_from_int(self.inner.read_scalar())
        self.order.append("s")
        return v

    def squeeze_challenge(self):
        v = self.inner.squeeze_challenge()
        self.order.append("c")
        raw = getattr(self.inner, "last_raw", None)
        return raw.words() if raw is not None else zu.fr_from_int(v)

    def reads_before_squeeze(self, i):
        """read_* calls completed before squeeze number i: AMDZK_PROOF_BAD_TRANSCRIPT's offset when that squeeze is refused."""
        at = [j for j, k in enumerate(self.order) if k == "c"][i]
        return at - i


def device_writer(transcript, script, multiopen=0):
    return DeviceWriter(writer(transcript, script), multiopen)


def device_reader(transcript, script, proof):
    return DeviceReader(reader(transcript, script, proof))
