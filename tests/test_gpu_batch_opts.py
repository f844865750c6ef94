"""GPU: amdzk_create_proof_batch_opts — the lock-step batch for keys with challenge phases, proofs with the caller's
transcript and different circuits on one SRS.

Expected bytes never come from the code under test: a phased proof's from tests/phased_oracle.py on the challenges the
callback was handed for that proof (the harness asserts that its own transcript squeezes them), an unphased proof's from
oracle/plonk_ref.py. Equality with amdzk_create_proof_opts on the same workspace is a second assertion."""
import ctypes as C

import numpy as np
import pytest
import zkutil as zu

import batch_opts_util as U
import circuits
import phased_circuits as PC
from batch_opts_util import INVALID, PR
from test_phased_oracle import RANDOM_SEEDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def gate_only_circuit(plonk, k=5, seed=1):
    """No lookup, no permutation, no instance column: one gate q * (b - a * a)."""
    rnd = np.random.RandomState(seed)
    cs = plonk.ConstraintSystem()
    a, b, q = cs.advice_column(), cs.advice_column(), cs.selector()
    cs.create_gate(lambda m: [m.query_selector(q) * (m.query_advice(b, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))])
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    for row in range(c.usable):
        x = int(rnd.randint(1, 1 << 30))
        c.fixed[q.index][row], c.advice[a.index][row], c.advice[b.index][row] = 1, x, x * x % circuits.R
    c.instances = []
    circuits.check_satisfied(c)
    return c


class ForwardedTranscript:
    """The oracle's own transcript writer, fed only through the library's callbacks (Montgomery words in, ints inside)."""

    def __init__(self, inner, fail_on_write=0):
        self.inner, self.calls, self.writes, self.fail_on_write = inner, 0, 0, fail_on_write

    def _write(self):
        self.writes += 1
        return self.writes == self.fail_on_write

    def common_point(self, w):
        self.calls += 1
        self.inner.common_point(zu.point_to_ints(w))

    def common_scalar(self, w):
        self.calls += 1
        self.inner.common_scalar(zu.fr_to_int(w))

    def write_point(self, w):
        self.calls += 1
        if self._write():
            return 3
        self.inner.write_point(zu.point_to_ints(w))

    def write_scalar(self, w):
        self.calls += 1
        if self._write():
            return 3
        self.inner.write_scalar(zu.fr_to_int(w))

    def squeeze_challenge(self):
        self.calls += 1
        return zu.fr_from_int(self.inner.squeeze_challenge())


def check_phased_batch(monkeypatch, B, seeds, idx=None, transcript=0, names=("blake2b", "shplonk")):
    """One batch of phased members: bytes equal the harness's, the callbacks are as documented, inspect(3) agrees."""
    idx = list(range(len(B.m))) if idx is None else idx
    got = B.batch(seeds, idx=idx, transcript=transcript)
    B.check_calls(idx)
    chs = [B.challenges(b) for b in idx]
    for j, b in enumerate(idx):
        assert isinstance(got[j], bytes), got[j]
        assert len(got[j]) == B.plonk.proof_size(B.ctx, B.pks[b], transcript)
        assert got[j] == B.expected(monkeypatch, b, seeds[j], chs[j], transcript=names[0], multiopen=names[1]), "proof %d" % j
    return got, chs


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("k", [5, 6])
def test_phased_bytes(ctx, pkg, plonk, oracle, monkeypatch, k, three):
    """rlc_circuit, two and three phases, B = 1, 2, 3 with different witnesses and seeds."""
    c = PC.rlc_circuit(plonk, k, seed=k, three_phases=three)
    B = U.Batch(ctx, pkg, plonk, oracle, k, [(c, None), (c, 101), (c, 102)])
    seeds = [31, 32, 33]
    got3, chs = check_phased_batch(monkeypatch, B, seeds)
    assert len(chs[0]) == (2 if three else 1) and all(0 < v < zu.R for ch in chs for v in ch)
    assert len({tuple(ch) for ch in chs}) == 3, "the proofs' challenges are pairwise different"
    assert len(set(got3)) == 3
    for nb in (1, 2):
        got, _ = check_phased_batch(monkeypatch, B, seeds[:nb], idx=list(range(nb)))
        assert got == got3[:nb]
    assert B.batch(seeds) == got3 and [B.challenges(b) for b in range(3)] == chs  # the workspaces are reused cleanly
    for b in range(3):
        assert B.single(b, seeds[b]) == got3[b] and B.challenges(b) == chs[b]
    B.free()


@pytest.mark.parametrize("transcript", ["blake2b", "keccak"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_modes(ctx, pkg, plonk, oracle, monkeypatch, transcript, multiopen):
    c = PC.rlc_circuit(plonk, 5, seed=4, three_phases=True)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, 103)])
    tk = (plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM) | (plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0)
    got, _ = check_phased_batch(monkeypatch, B, [8, 9], transcript=tk, names=(transcript, multiopen))
    assert got == [B.single(0, 8, tk), B.single(1, 9, tk)]
    B.free()


def test_non_consecutive_columns(ctx, pkg, plonk, oracle, monkeypatch):
    """interleaved: columns a, r, b, s in phases 0, 1, 0, 2 — phase 0 is two runs of columns per member. The bytes are those
    of the circuit whose columns are ordered by phase (the one the harness can produce), as in test_gpu_phased."""
    c = PC.rlc_circuit(plonk, 5, seed=7, three_phases=True, interleaved=True)
    assert c.desc["advice_column_phase"] == [0, 1, 0, 2]
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, 104)])
    got = B.batch([21, 22])
    B.check_calls([0, 1])
    c0 = PC.rlc_circuit(plonk, 5, seed=7, three_phases=True)
    opk0 = PR.keygen(U.PO.specialise(c0.desc, [0, 0]), c0.fixed, c0.assembly.mapping, U.TAU, transcript_repr=U.REPR)
    for b, w in enumerate((None, 104)):
        ch = B.challenges(b)
        adv0, fill0 = (c0.advice, c0.fill) if w is None else c0.witness_for(w)
        adv0 = [list(col) for col in adv0]
        for phase in (1, 2):
            fill0(phase, dict(enumerate(ch)), adv0)
        assert got[b] == U.PO.create_proof(monkeypatch, opk0, c0.desc, [c0.instances], [adv0], 21 + b, ch), "proof %d" % b
    assert got == [B.single(0, 21), B.single(1, 22)]
    B.free()


@pytest.mark.parametrize("seed", RANDOM_SEEDS[:6])
def test_random_phased_circuits(ctx, pkg, plonk, oracle, monkeypatch, seed):
    c = PC.random_phased_circuit(plonk, 5, seed=seed)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, None)])
    got, _ = check_phased_batch(monkeypatch, B, [seed, seed + 50])
    assert got[0] != got[1]
    B.free()


def test_the_phases_really_are_merged(ctx, pkg, plonk, oracle):
    """Per-kernel profiling, as test_the_commitments_really_are_merged: a B = 3 batch of three-phase proofs launches the
    level-1 accumulation exactly as often as a B = 1 batch — one submission per commitment step and per phase, whatever B —
    and fewer than three times the kernels in all."""
    c = PC.rlc_circuit(plonk, 5, seed=3, three_phases=True)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, 105), (c, 106)])
    B.batch([1, 2, 3])  # first use: workspaces, multiopen lists
    counts = []
    ctx.prof_enable(True)
    try:
        for idx in ([0], [0, 1, 2]):
            ctx.prof_reset()
            B.batch([1, 2, 3][: len(idx)], idx=idx)
            counts.append({k: v[0] for k, v in ctx.prof_dump().items()})
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    one, three = counts
    print("launches B=1: l1 %d, all %d; B=3: l1 %d, all %d" % (one["msm_accum_l1"], sum(one.values()), three["msm_accum_l1"], sum(three.values())))
    assert one["msm_accum_l1"] > 0 and three["msm_accum_l1"] == one["msm_accum_l1"]
    assert sum(three.values()) < 3 * sum(one.values())
    B.free()


def test_caller_transcripts(ctx, pkg, plonk, oracle, monkeypatch):
    """Per-proof objects that forward to the oracle's Blake2b collect the built-in transcript's bytes; a batch mixes built-in,
    caller's, built-in; a transcript that fails on proof 1's third write drops proof 1 alone."""
    c = PC.rlc_circuit(plonk, 5, seed=4, three_phases=True)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, 107), (c, 108)])
    seeds = [8, 9, 10]
    builtin, chs = check_phased_batch(monkeypatch, B, seeds)
    ts = [ForwardedTranscript(PR.Blake2bWrite()) for _ in range(3)]
    assert B.batch(seeds, transcript_objects=ts) == [b""] * 3  # the bytes are the callers'
    assert [bytes(t.inner.proof) for t in ts] == builtin and [B.challenges(b) for b in range(3)] == chs
    single = ForwardedTranscript(PR.Blake2bWrite())
    assert B.single(1, 9, transcript_object=single) == b"" and single.calls == ts[1].calls  # the same calls as alone
    t1 = ForwardedTranscript(PR.Blake2bWrite())
    assert B.batch(seeds, transcript_objects=[None, t1, None]) == [builtin[0], b"", builtin[2]]
    assert bytes(t1.inner.proof) == builtin[1]
    bad = ForwardedTranscript(PR.Blake2bWrite(), fail_on_write=3)
    got = B.batch(seeds, transcript_objects=[None, bad, None])
    assert isinstance(got[1], pkg.AmdzkError) and got[1].code == INVALID
    assert "proof 1: " in str(got[1]) and "transcript reported an error" in str(got[1])
    assert got[0] == builtin[0] and got[2] == builtin[2]
    assert B.batch(seeds) == builtin
    B.free()


def mixed(ctx, pkg, plonk, oracle, lookup_witness=None):
    cl = circuits.lookup_circuit(plonk, 5, seed=2)
    cr = PC.rlc_circuit(plonk, 5, seed=5, three_phases=True)
    cg = gate_only_circuit(plonk, 5)
    return U.Batch(ctx, pkg, plonk, oracle, 5, [(cl, lookup_witness), (cr, None), (cg, None)])


def test_mixed_circuits_on_one_srs(ctx, pkg, plonk, oracle, monkeypatch):
    """lookup_circuit, a three-phase rlc_circuit and a circuit without lookups or permutation on one ParamsKZG at k = 5: each
    proof equals its oracle and its single twin; the sizes differ and proof_stride is the largest; the unphased members are
    never wanted."""
    B = mixed(ctx, pkg, plonk, oracle)
    assert B.m[2].c.desc["lookups"] == [] and B.m[2].c.desc["permutation_columns"] == []
    seeds = [5, 6, 7]
    got = B.batch(seeds)
    B.check_calls([0, 1, 2])
    assert [list(w) for _, w, _ in B.calls] == [[0, 1, 0], [0, 1, 0]]
    sizes = [plonk.proof_size(ctx, pk) for pk in B.pks]
    assert len(set(sizes)) == 3 and [len(p) for p in got] == sizes
    ch = B.challenges(1)
    for b in range(3):
        assert got[b] == B.expected(monkeypatch, b, seeds[b], ch), "proof %d" % b
    assert got == [B.single(b, seeds[b]) for b in range(3)]
    assert B.batch(seeds, proof_stride=max(sizes)) == got
    with pytest.raises(pkg.AmdzkError, match="create_proof_batch_opts: proof_stride"):
        B.batch(seeds, proof_stride=max(sizes) - 1)
    assert B.batch(seeds[::-1], idx=[2, 1, 0]) == [B.single(b, s) for b, s in zip([2, 1, 0], seeds[::-1])]  # any order of keys
    B.free()


def dropped(pkg, e, b, text):
    assert isinstance(e, pkg.AmdzkError) and e.code == INVALID, e
    assert "proof %d: " % b in str(e) and text in str(e), str(e)


def test_proof_zero_drops_out_on_its_lookup(ctx, pkg, plonk, oracle, monkeypatch):
    """(a) proof 0's lookup input is outside its table: the gang's SRS, n and staging come from that proof's key."""
    cl = circuits.lookup_circuit(plonk, 5, seed=2)
    bad = [list(col) for col in cl.advice]
    bad[0][[r for r in range(cl.usable) if cl.fixed[2][r] == 1][0]] = 9  # not in the 0..7 range table
    cr = PC.rlc_circuit(plonk, 5, seed=5, three_phases=True)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(cl, (bad, cl.instances)), (cl, None), (cr, None)])
    got = B.batch([5, 6, 7])
    dropped(pkg, got[0], 0, "lookup 0 input not in table")
    B.check_calls([0, 1, 2])
    assert got[1] == B.expected(monkeypatch, 1, 6) and got[2] == B.expected(monkeypatch, 2, 7, B.challenges(2))
    B.m[0].adv0 = cl.advice  # every workspace is quiet and proves the right bytes alone
    want = B.expected(monkeypatch, 0, 11)
    assert B.single(0, 11) == want and B.single(1, 11) == want
    assert B.single(2, 7) == got[2]
    assert B.batch([11, 11, 7]) == [want, want, got[2]]
    B.free()


def test_the_callback_refuses_proof_zero(ctx, pkg, plonk, oracle, monkeypatch):
    """(b) proof_rc[0] = 1 in phase 1 drops proof 0 alone: phase 2 does not want it and shows it no challenge."""
    cr = PC.rlc_circuit(plonk, 5, seed=5, three_phases=True)
    cl = circuits.lookup_circuit(plonk, 5, seed=2)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(cr, None), (cr, 109), (cl, None)])
    good = B.batch([5, 6, 7])
    B.on_phase = lambda phase, wanted, chal: [1, 0, 0] if phase == 1 else None
    got = B.batch([5, 6, 7])
    B.on_phase = None
    dropped(pkg, got[0], 0, "the phase callback refused it in phase 1")
    assert [p for p, _, _ in B.calls] == [1, 2]
    assert list(B.calls[0][1]) == [1, 1, 0] and list(B.calls[1][1]) == [0, 1, 0] and not B.calls[1][2][0].any()
    assert got[1:] == good[1:]
    assert got[1] == B.expected(monkeypatch, 1, 6, B.challenges(1)) and got[2] == B.expected(monkeypatch, 2, 7)
    assert [B.single(b, s) for b, s in enumerate([5, 6, 7])] == good and B.batch([5, 6, 7]) == good
    B.free()


def test_the_callback_fails_in_a_mixed_batch(ctx, pkg, plonk, oracle, monkeypatch):
    """(c) the callback returns 1 in phase 1: every wanted proof drops, the unphased one finishes with its exact bytes, and
    the phase-2 callback is not made."""
    cr = PC.rlc_circuit(plonk, 5, seed=5, three_phases=True)
    cl = circuits.lookup_circuit(plonk, 5, seed=2)
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(cr, None), (cl, None), (cr, 110)])
    B.on_phase = lambda phase, wanted, chal: 1
    got = B.batch([5, 6, 7])
    B.on_phase = None
    assert [p for p, _, _ in B.calls] == [1]
    dropped(pkg, got[0], 0, "the phase callback returned 1 in phase 1")
    assert isinstance(got[2], pkg.AmdzkError) and got[2].code == INVALID
    assert got[1] == B.expected(monkeypatch, 1, 6)
    after = B.batch([5, 6, 7])
    assert after[1] == got[1] and after == [B.single(b, s) for b, s in enumerate([5, 6, 7])]
    assert after[0] == B.expected(monkeypatch, 0, 5, B.challenges(0))
    # a Python exception in the callback comes back as that exception, and the batch proves right after it
    def raising(phase, wanted, chal, stream):
        raise KeyError("synthesize failed")
    with pytest.raises(KeyError):
        B.batch([5, 6, 7], synthesize=raising)
    assert B.batch([5, 6, 7]) == after
    B.free()


def test_refusals(ctx, pkg, plonk, oracle):
    """Every whole-call refusal: AMDZK_E_INVALID, the prefix, every status = the code, every length 0 — and a good batch
    succeeds right after it. A second ParamsKZG of the same k gives the other-SRS refusal."""
    B = mixed(ctx, pkg, plonk, oracle)
    other = mixed(ctx, pkg, plonk, oracle)  # the same circuits on another ParamsKZG
    seeds = [5, 6, 7]
    want = B.batch(seeds)
    ffi, n = pkg.ffi, 32
    keys, adv = [pk.h for pk in B.pks], [d.ptr for d in B.d_adv]
    noop = ffi.BATCH_PHASE_FN(lambda *a: 0)
    stride = max(plonk.proof_size(ctx, pk) for pk in B.pks)
    cnt = max(plonk.proof_random_count(ctx, pk) for pk in B.pks)
    draws = np.zeros((cnt, 4), np.uint64)
    sc = (C.c_void_p * 3)(*[draws.ctypes.data] * 3)
    sc_hole = (C.c_void_p * 3)(draws.ctypes.data, None, draws.ctypes.data)
    holed = ffi.Transcript(None, *[ffi._T_IN(lambda *a: 0) for _ in range(4)], ffi._T_IN())  # squeeze_challenge is NULL
    trs = (C.POINTER(ffi.Transcript) * 3)(None, C.pointer(holed), None)

    def refused(match, **kw):
        k, a = kw.pop("keys", keys), kw.pop("adv", adv)
        kw.setdefault("phase_fn", noop)
        kw.setdefault("proof_stride", stride)
        rc, st, lens, msg = U.raw_call(ctx, pkg, k, a, n, **kw)
        assert rc == INVALID and msg.startswith("create_proof_batch_opts:") and match in msg, msg
        assert st == [INVALID] * len(k) and lens == ([0] * len(k) if not kw.get("lens_null") else [7] * len(k))  # (no array: nothing to write)
        assert B.batch(seeds) == want

    refused("null argument", seeds=seeds, opts_null=True)
    refused("no proofs", seeds=seeds, keys_null=True)
    refused("null argument", seeds=seeds, lens_null=True)
    refused("null key (proof 1)", seeds=seeds, keys=[keys[0], None, keys[2]])
    refused("null advice (proof 2)", seeds=seeds, adv=[adv[0], adv[1], None])
    refused("null scalars (proof 1)", seeds=None, scalars=sc_hole, scalar_count=cnt)
    refused("no proofs", seeds=[], keys=[], adv=[])
    refused("amdzk_batch_proof_opts.size is 8", seeds=seeds, opts_size=8)
    refused("amdzk_batch_proof_opts.size", seeds=seeds, opts_size=C.sizeof(ffi.BatchProofOpts) - 8)
    refused("neither rng_seeds nor scalars", seeds=None)
    refused("proofs 0 and 2 share one workspace", seeds=seeds, keys=[keys[0], keys[1], keys[0]])
    refused("proof 1's key was made on another amdzk_srs", seeds=seeds, keys=[keys[0], other.pks[1].h, keys[2]])
    refused("a phase callback is needed", seeds=seeds, phase_fn=ffi.BATCH_PHASE_FN())
    refused("amdzk_transcript of proof 1 has a null member", seeds=seeds, transcripts=trs)
    refused("advice stride < n", seeds=seeds, advice_stride=n - 1)
    refused("proof_stride", seeds=seeds, proof_stride=stride - 1)
    refused("scalars given", seeds=None, scalars=sc, scalar_count=cnt - 1)
    refused("unknown transcript kind 7", seeds=seeds, kind=7)
    # through the Python mirror a refusal raises
    with pytest.raises(pkg.AmdzkError, match="create_proof_batch_opts: proof 0's key has advice in 3 phases") as e:
        B.batch(seeds[:1], idx=[1], synthesize=None)
    assert e.value.code == INVALID
    # amdzk_create_proof_batch still refuses what it refused
    with pytest.raises(pkg.AmdzkError, match="not the first key or a workspace clone"):
        plonk.create_proof_batch(ctx, [B.pks[0], B.pks[2]], [B.inst[0], B.inst[2]], [B.d_adv[0], B.d_adv[2]], [1, 2])
    assert B.batch(seeds) == want
    other.free()
    B.free()


class Stopped(Exception):
    """Raised by StoppingTranscript at the call it was told to fail."""


class StoppingTranscript(ForwardedTranscript):
    """Fails (the callback returns non-zero) at call number `stop`, counted from 0 over all five members, and goes on
    counting the calls it receives afterwards."""

    def __init__(self, inner, stop):
        super().__init__(inner)
        self.stop = stop

    def _tick(self):
        if self.calls == self.stop:
            self.calls += 1
            raise Stopped(self.stop)

    def common_point(self, w):
        self._tick()
        super().common_point(w)

    def common_scalar(self, w):
        self._tick()
        super().common_scalar(w)

    def write_point(self, w):
        self._tick()
        super().write_point(w)

    def write_scalar(self, w):
        self._tick()
        super().write_scalar(w)

    def squeeze_challenge(self):
        self._tick()
        return super().squeeze_challenge()


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_a_proof_alone_and_a_batch_of_one_stop_at_the_same_call(ctx, pkg, plonk, oracle, multiopen):
    """The caller's transcript reports an error at call j, for every j of the proof: amdzk_create_proof_opts and
    amdzk_create_proof_batch_opts with that one proof end with the same message (the batch's behind "proof 0: ") after the
    same number of calls — one statement of the order serves both. Behind the last call both give the proof's bytes."""
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(circuits.lookup_circuit(plonk, 5, seed=2), None)])
    tk = plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0
    whole = ForwardedTranscript(PR.Blake2bWrite())
    assert B.single(0, 9, transcript=tk, transcript_object=whole) == b""
    assert bytes(whole.inner.proof) == B.expected(None, 0, 9, multiopen=multiopen)
    last_error = lambda: ctx.L.amdzk_last_error(ctx.h).decode()
    for j in range(whole.calls):
        alone, batched = StoppingTranscript(PR.Blake2bWrite(), j), StoppingTranscript(PR.Blake2bWrite(), j)
        with pytest.raises(Stopped):
            B.single(0, 9, transcript=tk, transcript_object=alone)
        said = last_error()
        with pytest.raises(Stopped):
            B.batch([9], transcript=tk, transcript_objects=[batched])
        assert said == "create_proof: the caller's transcript reported an error" and last_error() == "proof 0: " + said, "call %d" % j
        assert alone.calls == batched.calls > j, "call %d" % j
    alone, batched = StoppingTranscript(PR.Blake2bWrite(), whole.calls), StoppingTranscript(PR.Blake2bWrite(), whole.calls)
    assert B.single(0, 9, transcript=tk, transcript_object=alone) == b"" and B.batch([9], transcript=tk, transcript_objects=[batched]) == [b""]
    assert bytes(alone.inner.proof) == bytes(batched.inner.proof) == bytes(whole.inner.proof) and alone.calls == batched.calls == whole.calls
    B.free()


def test_every_single_fault_refusal_word_for_word(ctx, pkg, plonk, oracle):
    """Both batch entry points, one fault per call: the whole message, the status in every proof's slot, every length 0,
    and a good batch right after. amdzk_create_proof_batch_opts on three circuits of one SRS, amdzk_create_proof_batch on a
    key and its clone."""
    UNSUPPORTED = -5
    ffi, n = pkg.ffi, 32
    B = mixed(ctx, pkg, plonk, oracle)
    other = mixed(ctx, pkg, plonk, oracle)  # the same circuits on another ParamsKZG
    cl = circuits.lookup_circuit(plonk, 5, seed=2)
    S = U.Batch(ctx, pkg, plonk, oracle, 5, [(cl, None), (cl, None)])  # one key, two workspaces
    noop = ffi.BATCH_PHASE_FN(lambda *a: 0)
    holed = ffi.Transcript(None, *[ffi._T_IN(lambda *a: 0) for _ in range(4)], ffi._T_IN())  # squeeze_challenge is NULL
    draws = np.zeros((max(plonk.proof_random_count(ctx, pk) for pk in B.pks), 4), np.uint64)

    def entry(batch, strict, who):
        seeds = list(range(5, 5 + len(batch.pks)))
        want = batch.batch(seeds)
        keys, adv = [pk.h for pk in batch.pks], [d.ptr for d in batch.d_adv]
        stride = max(plonk.proof_size(ctx, pk) for pk in batch.pks)
        N = len(keys)

        def refused(text, code=INVALID, **kw):
            k, a = kw.pop("keys", keys), kw.pop("adv", adv)
            kw.setdefault("seeds", seeds)
            if not strict:
                kw.setdefault("phase_fn", noop)
            kw.setdefault("proof_stride", stride)
            rc, st, lens, msg = U.raw_call(ctx, pkg, k, a, n, strict=strict, **kw)
            assert (rc, msg) == (code, who + ": " + text)
            assert st == [code] * len(k) and lens == ([7] * len(k) if kw.get("lens_null") else [0] * len(k))  # (no array: nothing to write)
            assert batch.batch(seeds) == want
        return refused, keys, adv, stride, N

    refused, keys, adv, stride, N = entry(B, False, "create_proof_batch_opts")
    counts = [plonk.proof_random_count(ctx, pk) for pk in B.pks]
    short = max(counts) - 1
    first_short = [b for b in range(N) if counts[b] > short][0]
    sc = lambda *ptrs: (C.c_void_p * N)(*ptrs)
    refused("no proofs", keys_null=True)
    refused("no proofs", seeds=[], keys=[], adv=[])
    refused("null argument", opts_null=True)
    refused("null argument", lens_null=True)
    refused("null argument", out_null=True)
    refused("amdzk_batch_proof_opts.size is 8, this library needs %d" % C.sizeof(ffi.BatchProofOpts), opts_size=8)
    refused("neither rng_seeds nor scalars", seeds=None)
    refused("null key (proof 1)", keys=[keys[0], None, keys[2]])
    refused("proofs 0 and 2 share one workspace", keys=[keys[0], keys[1], keys[0]])
    refused("proof 1's key was made on another amdzk_srs than proof 0's: the batch commits over one SRS", keys=[keys[0], other.pks[1].h, keys[2]])
    refused("null advice (proof 2)", adv=[adv[0], adv[1], None])
    refused("null scalars (proof 1)", seeds=None, scalars=sc(draws.ctypes.data, None, draws.ctypes.data), scalar_count=len(draws))
    refused("%d scalars given, proof %d needs %d" % (short, first_short, counts[first_short]), seeds=None, scalars=sc(*[draws.ctypes.data] * N),
            scalar_count=short)
    refused("advice stride < n", advice_stride=n - 1)
    refused("unknown transcript kind 7", kind=7)
    refused("proof_stride %d < proof size %d" % (stride - 1, stride), proof_stride=stride - 1)
    refused("proof 1's key has advice in 3 phases: a phase callback is needed", phase_fn=ffi.BATCH_PHASE_FN())
    refused("amdzk_transcript of proof 1 has a null member", transcripts=(C.POINTER(ffi.Transcript) * N)(None, C.pointer(holed), None))

    phased_key = B.pks[1].h
    refused, keys, adv, stride, N = entry(S, True, "create_proof_batch")
    count = plonk.proof_random_count(ctx, S.pks[0])
    sc = lambda *ptrs: (C.c_void_p * N)(*ptrs)
    refused("no proofs", keys_null=True)
    refused("no proofs", seeds=[], keys=[], adv=[])
    refused("null argument", opts_null=True)
    refused("null argument", lens_null=True)
    refused("null argument", out_null=True)
    refused("amdzk_batch_opts.size is 8, this library needs %d" % C.sizeof(ffi.BatchOpts), opts_size=8)
    refused("neither rng_seeds nor scalars", seeds=None)
    refused("null key (proof 1)", keys=[keys[0], None])
    refused("proofs 0 and 1 share one workspace", keys=[keys[0], keys[0]])
    refused("proof 1's key is not the first key or a workspace clone of it", keys=[keys[0], B.pks[0].h])  # the same circuit, another key
    refused("null advice (proof 1)", adv=[adv[0], None])
    refused("null scalars (proof 1)", seeds=None, scalars=sc(draws.ctypes.data, None), scalar_count=count)
    refused("%d scalars given, %d needed" % (count - 1, count), seeds=None, scalars=sc(*[draws.ctypes.data] * N), scalar_count=count - 1)
    refused("advice stride < n", advice_stride=n - 1)
    refused("unknown transcript kind 7", kind=7)
    refused("proof_stride %d < proof size %d" % (stride - 1, stride), proof_stride=stride - 1)
    refused("the key has challenge phases or challenges: prove it with amdzk_create_proof_opts", code=UNSUPPORTED, keys=[phased_key], adv=[B.d_adv[1].ptr],
            seeds=[5])
    S.free()
    other.free()
    B.free()
