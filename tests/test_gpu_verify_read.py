"""GPU: amdzk_verify_proofs* through the CALLER's read transcript (amdzk_transcript_read, amdzk_verify_opts.transcripts). The
oracle's own Blake2bRead / Keccak256Read over a proof's bytes, wrapped as callbacks, must give word for word what the bytes
route gives — pair_out, statuses, verdicts — through a proving key and a verifying key, through verify and decide, alone and
mixed with bytes proofs in one batch. A third transcript the library knows nothing about (Blake2b under another
personalisation) is proved through the caller's write transcript and decided through the caller's read transcript, against
the oracle's verifier run over the same class. Every failure a callback can produce gets its documented status and offset.
All comparisons are exact."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402
from test_gpu_phased import ForwardedTranscript  # noqa: E402
from test_gpu_verify import Rig, put  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, Q, R = VC.TAU, zu.Q, zu.R
WELL, BAD_POINT, BAD_SCALAR, BAD_TRANSCRIPT = 0, 2, 3, 5
RAW_R = np.array(zu.limbs(R), dtype=np.uint64)  # the modulus itself as words: not a residue
RAW_Q = np.array(zu.limbs(Q), dtype=np.uint64)


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


class Reader:
    """An oracle read transcript (ints inside) behind the library's callbacks (Montgomery words outside). Hooks for the bad
    inputs: fail = ("read" | "squeeze", i): that call returns non-zero; replace = {read index: words to hand back instead};
    big_challenge = i: the i-th squeeze hands back the modulus."""

    def __init__(self, inner, fail=None, replace=None, big_challenge=None):
        self.inner, self.fail, self.replace, self.big_challenge = inner, fail, replace or {}, big_challenge
        self.reads = self.squeezes = self.commons = 0
        self.order = []

    def common_point(self, w):
        raise AssertionError("the verifier does not call common_point")

    def common_scalar(self, w):
        self.commons += 1
        self.inner.common_scalar(zu.fr_to_int(w))

    def _read(self, kind, get, conv):
        i = self.reads
        if self.fail == ("read", i):
            raise _Refuse()
        v = conv(get())
        self.reads += 1
        self.order.append(kind)
        return self.replace.get(i, v)

    def read_point(self):
        return self._read("p", self.inner.read_point, zu.point_from_ints)

    def read_scalar(self):
        return self._read("s", self.inner.read_scalar, zu.fr_from_int)

    def squeeze_challenge(self):
        i = self.squeezes
        if self.fail == ("squeeze", i):
            raise _Refuse()
        self.squeezes += 1
        self.order.append("c")
        v = zu.fr_from_int(self.inner.squeeze_challenge())
        return RAW_R if self.big_challenge == i else v


class _Refuse(Exception):
    """Raised inside a callback: ffi.read_transcript turns it into a non-zero return."""


def reader_of(case, proof=None, cls=None, **kw):
    proof = case.proof if proof is None else proof
    cls = cls or (PR.Blake2bRead if case.transcript == "blake2b" else PR.Keccak256Read)
    return Reader(cls(proof), **kw)


def mo_flag(plonk, case):
    return plonk.MULTIOPEN_GWC if case.multiopen == "gwc" else 0


def same_guard(a, b):
    assert a.statuses == b.statuses
    assert np.array_equal(a.lhs, b.lhs) and np.array_equal(a.rhs, b.rhs)


def bump_scalar(case, which=0):
    """The proof with its `which`-th scalar + 1 (kept below r): well formed, false."""
    kinds = VR.element_kinds(case.desc, case.N, case.multiopen)
    psz, end = (64, "big") if case.transcript == "evm" else (32, "little")
    off, seen = 0, 0
    for k in kinds:
        if k == "s":
            if seen == which:
                v = int.from_bytes(case.proof[off:off + 32], end)
                return put(case.proof, off, ((v + 1) % R).to_bytes(32, end))
            seen += 1
        off += psz if k == "p" else 32
    raise AssertionError("no such scalar")


# ------------------------------------------------------------------------------------ parity with the bytes route
@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_the_oracles_reader_as_callbacks_gives_the_bytes_routes_words(plonk, rigs, vparams, name, N, transcript, multiopen):
    rig = rigs(name, N)
    case = rig.case(transcript, multiopen)
    flags = VC.kind_flags(plonk, transcript, multiopen)
    batch = [case.proof, bump_scalar(case)]
    inst = [rig.instances_arg()] * 2
    w = np.stack([zu.fr_from_int(v) for v in (3, 5)])
    vk = rig.pk.get_vk()
    try:
        for key in (rig.pk, vk):
            want = plonk.verify_proofs(rig.ctx, key, inst, batch, transcript=flags, n_circuits=N, combine_scalars=w)
            assert want.well_formed
            readers = [reader_of(case, p) for p in batch]
            # only the opening scheme's bit counts for a transcript proof; the bytes are not read
            got = plonk.verify_proofs(rig.ctx, key, inst, [None, None], transcript=mo_flag(plonk, case), n_circuits=N, combine_scalars=w,
                                      transcripts=readers)
            assert got.errors == []
            same_guard(got, want)
            kinds = VR.element_kinds(case.desc, N, multiopen)
            for rd in readers:  # every element was read once, in the proof's order, and the bytes ran out exactly
                assert "".join(k for k in rd.order if k != "c") == kinds and rd.inner.pos == len(rd.inner.data)
                assert rd.commons == 1 + N * sum(len(col) for col in case.c.instances)
            want_v = plonk.decide_proofs(rig.ctx, key, vparams, inst, batch, transcript=flags, n_circuits=N)
            got_v = plonk.decide_proofs(rig.ctx, key, vparams, inst, [None, None], transcript=mo_flag(plonk, case), n_circuits=N,
                                        transcripts=[reader_of(case, p) for p in batch])
            assert got_v == want_v and want_v[0] == [True, False]
        one = plonk.verify_proof(rig.ctx, rig.pk, rig.instances_arg(), None, transcript=reader_of(case), n_circuits=N, multiopen=mo_flag(plonk, case))
        same_guard(one, plonk.verify_proof(rig.ctx, rig.pk, rig.instances_arg(), case.proof, transcript=flags, n_circuits=N))
        assert plonk.decide_proof(rig.ctx, vk, vparams, rig.instances_arg(), None, transcript=reader_of(case), n_circuits=N,
                                  multiopen=mo_flag(plonk, case)) is True
    finally:
        vk.free()


# ------------------------------------------------------------------------------------ mixed batches
@pytest.mark.parametrize("transcript,multiopen", [("blake2b", "shplonk"), ("evm", "gwc")])
def test_a_batch_mixes_bytes_and_transcripts_in_every_position(plonk, rigs, vparams, transcript, multiopen):
    rig = rigs("lookup")
    cases = [rig.case(transcript, multiopen, seed=s) for s in (20, 21, 22)]
    flags = VC.kind_flags(plonk, transcript, multiopen)
    proofs = [cases[0].proof, bump_scalar(cases[1], 2), cases[2].proof]
    inst = [rig.inst] * 3
    w = np.stack([zu.fr_from_int(v) for v in (2, 3, 4)])
    want = plonk.verify_proofs(rig.ctx, rig.pk, inst, proofs, transcript=flags, combine_scalars=w)
    want_v = plonk.decide_proofs(rig.ctx, rig.pk, vparams, inst, proofs, transcript=flags)
    assert want_v[0] == [True, False, True]
    for mask in range(1, 8):
        trs = lambda: [reader_of(cases[b], proofs[b]) if mask >> b & 1 else None for b in range(3)]
        given = [None if mask >> b & 1 else proofs[b] for b in range(3)]
        same_guard(plonk.verify_proofs(rig.ctx, rig.pk, inst, given, transcript=flags, combine_scalars=w, transcripts=trs()), want)
        assert plonk.decide_proofs(rig.ctx, rig.pk, vparams, inst, given, transcript=flags, transcripts=trs()) == want_v
    # seeded weights belong to batch positions on both routes
    same_guard(plonk.verify_proofs(rig.ctx, rig.pk, inst, [None] * 3, transcript=flags, combine_seed=77,
                                   transcripts=[reader_of(c, p) for c, p in zip(cases, proofs)]),
               plonk.verify_proofs(rig.ctx, rig.pk, inst, proofs, transcript=flags, combine_seed=77))


def test_seventeen_transcript_proofs_cross_the_decide_run(plonk, rigs, vparams):
    rig = rigs("square")
    assert plonk.DECIDE_RUN == 16 and rig.c.k == 4
    case = rig.case("blake2b", "shplonk")
    proofs = [case.proof] * 15 + [bump_scalar(case), case.proof]
    inst = [rig.inst] * 17
    want = plonk.decide_proofs(rig.ctx, rig.pk, vparams, inst, proofs)
    assert want[0] == [True] * 15 + [False, True]
    assert plonk.decide_proofs(rig.ctx, rig.pk, vparams, inst, [None] * 17, transcripts=[reader_of(case, p) for p in proofs]) == want
    same_guard(plonk.verify_proofs(rig.ctx, rig.pk, inst, [None] * 17, combine_seed=5, transcripts=[reader_of(case, p) for p in proofs]),
               plonk.verify_proofs(rig.ctx, rig.pk, inst, proofs, combine_seed=5))


# ------------------------------------------------------------------------------------ a third transcript
class OtherWrite(PR.Blake2bWrite):
    """Blake2b under another personalisation: bytes as Blake2bWrite's, challenges of its own."""

    def __init__(self):
        super().__init__()
        self.state = hashlib.blake2b(digest_size=64, person=b"amdzk-test-other")


class OtherRead(PR.Blake2bRead):
    def __init__(self, proof):
        super().__init__(proof)
        self.state = hashlib.blake2b(digest_size=64, person=b"amdzk-test-other")


@pytest.mark.parametrize("name,multiopen", [("square", "shplonk"), ("square", "gwc"), ("lookup", "gwc")])
def test_a_third_transcript_proved_and_decided_through_the_callers_objects(plonk, rigs, vparams, monkeypatch, name, multiopen):
    rig = rigs(name)
    mo = plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0
    t = ForwardedTranscript(OtherWrite(), multiopen=mo)
    assert plonk.create_proof(rig.ctx, rig.pk, rig.inst, rig.d_adv[0], seed=9, transcript=t) == b""
    proof = bytes(t.inner.proof)
    builtin = rig.case("blake2b", multiopen, seed=9)
    assert len(proof) == len(builtin.proof) and proof != builtin.proof
    case = VC.Case(name, rig.c, rig.c.desc, rig.opk, [rig.c.instances], proof, "blake2b", multiopen, None)
    kinds = VR.element_kinds(case.desc, 1, multiopen)
    n_sc = kinds.count("s")
    mutants = [bump_scalar(case, i) for i in range(n_sc if name == "square" else 3)]
    mutants.append(put(put(proof, 0, proof[32:64]), 32, proof[0:32]))  # the first two commitments swapped
    assert kinds[:2] == "pp" and proof[0:32] != proof[32:64]
    batch = [proof] + mutants
    # the oracle's verifier over the same transcript class (its pair with tau known)
    monkeypatch.setattr(PR, "Blake2bWrite", OtherWrite)
    monkeypatch.setattr(PR, "Blake2bRead", OtherRead)
    want = [case.decode(p) == (0, 0) and VR.holds(case.pair(p), TAU) for p in batch]
    monkeypatch.undo()
    assert want == [True] + [False] * len(mutants)
    assert not VR.holds(case.pair(proof), TAU), "under the built-in Blake2b the third transcript's proof must not verify"
    verdicts, statuses = plonk.decide_proofs(rig.ctx, rig.pk, vparams, [rig.inst] * len(batch), [None] * len(batch), transcript=mo,
                                             transcripts=[Reader(OtherRead(p)) for p in batch])
    assert [tuple(s) for s in statuses] == [(0, 0)] * len(batch)
    assert verdicts == want
    # the pair is the oracle's, as group elements
    monkeypatch.setattr(PR, "Blake2bRead", OtherRead)
    ref = case.pair(proof)
    monkeypatch.undo()
    g = plonk.verify_proof(rig.ctx, rig.pk, rig.inst, None, transcript=Reader(OtherRead(proof)), multiopen=mo)
    assert (zu.point_to_ints(g.lhs), zu.point_to_ints(g.rhs)) == ref
    # the bytes route reads the same bytes with the built-in Blake2b: other challenges, a false proof
    assert plonk.decide_proof(rig.ctx, rig.pk, vparams, rig.inst, proof, transcript=mo) is False


# ------------------------------------------------------------------------------------ bad inputs through callbacks
def off_curve(p):
    return zu.point_from_ints((p[0], (p[1] + 1) % Q))


@pytest.mark.parametrize("transcript,multiopen", [("blake2b", "shplonk"), ("evm", "gwc")])
def test_callback_failures_get_their_status_and_offset_and_spare_the_rest(plonk, rigs, vparams, transcript, multiopen):
    rig = rigs("lookup")
    case = rig.case(transcript, multiopen)
    flags = VC.kind_flags(plonk, transcript, multiopen)
    kinds = VR.element_kinds(case.desc, 1, multiopen)
    E, first_s, last_p = len(kinds), kinds.index("s"), len(kinds) - 1
    pts, _scs = VC.decoded_elements(case)
    probe = reader_of(case)
    plonk.verify_proof(rig.ctx, rig.pk, rig.inst, None, transcript=probe, multiopen=mo_flag(plonk, case))
    n_squeeze = probe.squeezes
    reads_before_squeeze = [probe.order[:i].count("p") + probe.order[:i].count("s") for i, k in enumerate(probe.order) if k == "c"]

    class NoScalars(Reader):
        read_scalar = None

    zero_pt = np.zeros(8, np.uint64)
    big_x = zu.point_from_ints(pts[1]).copy()
    big_x[:4] = RAW_Q
    big_y = zu.point_from_ints(pts[last_p - kinds.count("s")]).copy()
    big_y[4:] = RAW_Q
    bad = [  # (reader arguments, expected (status, offset))
        (dict(fail=("read", 0)), (BAD_TRANSCRIPT, 0)),
        (dict(fail=("read", first_s + 1)), (BAD_TRANSCRIPT, first_s + 1)),
        (dict(fail=("read", E - 1)), (BAD_TRANSCRIPT, E - 1)),
        (dict(fail=("squeeze", 0)), (BAD_TRANSCRIPT, reads_before_squeeze[0])),
        (dict(fail=("squeeze", n_squeeze - 1)), (BAD_TRANSCRIPT, reads_before_squeeze[n_squeeze - 1])),
        (dict(big_challenge=1), (BAD_TRANSCRIPT, reads_before_squeeze[1])),
        (dict(big_challenge=n_squeeze - 1), (BAD_TRANSCRIPT, reads_before_squeeze[n_squeeze - 1])),
        (dict(replace={0: off_curve(pts[0])}), (BAD_POINT, 0)),
        (dict(replace={1: big_x}), (BAD_POINT, 1)),
        (dict(replace={last_p: big_y}), (BAD_POINT, last_p)),
        (dict(replace={2: zero_pt}), (BAD_POINT, 2)),
        (dict(replace={first_s: RAW_R}), (BAD_SCALAR, first_s)),
        (dict(replace={last_p - 2: RAW_R if kinds[last_p - 2] == "s" else zero_pt}), (BAD_SCALAR if kinds[last_p - 2] == "s" else BAD_POINT, last_p - 2)),
        (dict(replace={3: zero_pt, first_s: RAW_R}), (BAD_POINT, 3)),  # the first offender in read order
    ]
    good = plonk.verify_proofs(rig.ctx, rig.pk, [rig.inst] * 2, [case.proof] * 2, transcript=flags, combine_scalars=np.stack([zu.fr_from_int(2), zu.fr_from_int(7)]))
    for kw, want in bad:
        w = np.stack([zu.fr_from_int(v) for v in (2, 11, 7)])
        g = plonk.verify_proofs(rig.ctx, rig.pk, [rig.inst] * 3, [None, None, case.proof], transcript=flags, combine_scalars=w,
                                transcripts=[reader_of(case), reader_of(case, **kw), None])
        assert [tuple(s) for s in g.statuses] == [(0, 0), want, (0, 0)], kw
        assert np.array_equal(g.lhs, good.lhs) and np.array_equal(g.rhs, good.rhs), kw
        assert all(isinstance(e, _Refuse) for e in g.errors) and (len(g.errors) == 1) == ("fail" in kw), kw
    # a NULL member: nothing is called
    nul = NoScalars(PR.Blake2bRead(case.proof) if transcript == "blake2b" else PR.Keccak256Read(case.proof))
    verdicts, statuses = plonk.decide_proofs(rig.ctx, rig.pk, vparams, [rig.inst] * 3, [case.proof, None, None], transcript=flags,
                                             transcripts=[None, nul, reader_of(case)])
    assert [tuple(s) for s in statuses] == [(0, 0), (BAD_TRANSCRIPT, 0), (0, 0)] and verdicts == [True, False, True]
    assert nul.commons == 0 and nul.reads == 0 and nul.squeezes == 0
    # a batch whose every proof fails in its transcript: both points are the identity, the call still ran
    g = plonk.verify_proofs(rig.ctx, rig.pk, [rig.inst], [None], transcript=flags, transcripts=[reader_of(case, fail=("read", 5))])
    assert [tuple(s) for s in g.statuses] == [(BAD_TRANSCRIPT, 5)] and not g.lhs.any() and not g.rhs.any()
    with pytest.raises(ValueError, match=r"status 5 \(BAD_TRANSCRIPT\), offset 5"):
        plonk.verify_proof(rig.ctx, rig.pk, rig.inst, None, transcript=reader_of(case, fail=("read", 5)), multiopen=mo_flag(plonk, case))


# ------------------------------------------------------------------------------------ the struct's sizes
def test_the_old_struct_size_means_no_transcripts_and_one_byte_less_is_refused(ctx, pkg, plonk, rigs):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk")
    VO = pkg.ffi.VerifyOpts
    legacy = pkg.ffi.VERIFY_OPTS_LEGACY_SIZE
    assert legacy == VO.combine_scalars.offset + C.sizeof(C.c_void_p) and legacy < C.sizeof(VO)
    want = plonk.verify_proofs(ctx, rig.pk, [rig.inst], [case.proof])
    rd = reader_of(case, fail=("read", 0))
    got = plonk.verify_proofs(ctx, rig.pk, [rig.inst], [case.proof], opts_size=legacy, transcripts=[rd])  # the field is not read
    same_guard(got, want)
    assert rd.commons == 0 and rd.reads == 0
    for size in (legacy - 1, legacy + 1, C.sizeof(VO) - 1):
        with pytest.raises(pkg.ffi.AmdzkError, match="verify_proofs: amdzk_verify_opts.size") as e:
            plonk.verify_proofs(ctx, rig.pk, [rig.inst], [case.proof], opts_size=size)
        assert e.value.code == -2
    # proofs / proof_lens may be NULL only when every proof has a transcript
    L = ctx.L
    errors = []
    tr, keep = pkg.ffi.read_transcript(reader_of(case), errors)
    trs = (C.POINTER(pkg.ffi.TranscriptRead) * 2)(C.pointer(tr), None)
    cols = [np.ascontiguousarray(v) for v in rig.inst]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[v.ctypes.data if v.size else None for v in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[v.shape[0] for v in cols])
    ipp = (C.POINTER(C.c_void_p) * 2)(*[C.cast(ptrs, C.POINTER(C.c_void_p))] * 2)
    lpp = (C.POINTER(C.c_size_t) * 2)(*[C.cast(lens, C.POINTER(C.c_size_t))] * 2)
    st = (pkg.ffi.ProofStatus * 2)()
    pair = np.zeros(16, np.uint64)
    opts = VO(C.sizeof(VO), 0, 1, 0, None, trs)
    assert L.amdzk_verify_proofs(ctx.h, rig.pk.h, 2, ipp, lpp, None, None, C.byref(opts), st, pair.ctypes.data) == -2
    assert L.amdzk_last_error(ctx.h).decode().startswith("verify_proofs: null argument")
    assert L.amdzk_verify_proofs(ctx.h, rig.pk.h, 1, ipp, lpp, None, None, C.byref(opts), st, pair.ctypes.data) == 0
    assert (st[0].status, st[0].offset) == (0, 0) and errors == []
    assert np.array_equal(pair[:8], want.lhs) and np.array_equal(pair[8:], want.rhs)
    del keep
