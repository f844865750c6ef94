"""GPU: create_proof with challenge phases and with a caller-owned transcript, through the C ABI.

A phased key (amdzk_keygen_phased) is proved with amdzk_create_proof_opts: the phase callback fills the later-phase
columns on the device from the challenges it is handed; the bytes equal those of the phased-order harness
(tests/phased_oracle.py: the unmodified oracle driven in upstream's phased order on the description specialised to the
challenges), and the harness asserts that its transcript squeezes the very values the device reported to the callback."""
import ctypes as C
import os
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
import scripted_transcript as ST  # noqa: E402
from test_phased_oracle import RANDOM_SEEDS  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
_srs_cache = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


class Device:
    """One phased circuit on the device: the key (and clones for N instances), the advice buffers with the later phases
    still zero, and the phase callback that fills them from the circuit's own `fill`."""

    def __init__(self, ctx, pkg, plonk, oracle, c, N=1, flags=None):
        self.ctx, self.plonk, self.oracle, self.c, self.N = ctx, plonk, oracle, c, N
        if c.k not in _srs_cache:
            _srs_cache[c.k] = zu.test_srs(oracle, c.k, TAU)
        g, gl = _srs_cache[c.k]
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=flags)
        self.pks = [self.pk] + [self.pk.clone_workspace() for _ in range(N - 1)]
        self.wit = [(c.advice, c.fill)] + [c.witness_for(100 + i) for i in range(1, N)]
        self.inst_ints = [c.instances] * N
        self.inst = [[zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]] * N
        self.d_adv = [ctx.alloc(len(c.advice) * c.n * 32) for _ in range(N)]
        self.calls = []

    def reset(self):
        """Fresh witnesses: phase-0 columns uploaded, later phases zero on the host and on the device."""
        self.adv = [[list(col) for col in w[0]] for w in self.wit]
        for d, a in zip(self.d_adv, self.adv):
            d.upload(np.stack([zu.ints_to_fr(self.oracle, col) for col in a]))
        self.calls = []

    def synthesize(self, phase, challenges, stream):
        known = {i: zu.fr_to_int(challenges[i]) for i in range(len(challenges))}
        self.calls.append((phase, known))
        ap = self.c.desc["advice_column_phase"]
        for ci in range(self.N):
            self.wit[ci][1](phase, known, self.adv[ci])
            for col in range(len(ap)):
                if ap[col] == phase:
                    host = np.ascontiguousarray(zu.ints_to_fr(self.oracle, self.adv[ci][col]))
                    self.ctx._chk(self.ctx.L.amdzk_dev_upload(self.ctx.h, C.c_void_p(self.d_adv[ci].ptr.value + col * self.c.n * 32),
                                                              host.ctypes.data, host.nbytes))

    def prove(self, seed=0, scalars=None, transcript=0, transcript_object=None, synthesize="default", opts_size=None):
        self.reset()
        return self.plonk.create_proof_opts(self.ctx, self.pks, self.inst, self.d_adv, seed=seed, scalars=scalars, transcript=transcript,
                                            synthesize=self.synthesize if synthesize == "default" else synthesize,
                                            transcript_object=transcript_object, opts_size=opts_size)

    def challenges(self):
        """The challenges of the last proof as the device reported them: to the last callback, and through pk_inspect."""
        got = [zu.fr_to_int(x) for x in self.pk.inspect(3)]
        nph = max(self.c.desc["advice_column_phase"]) + 1
        assert [p for p, _ in self.calls] == list(range(1, nph)), "one callback per phase >= 1, in order"
        cp = self.c.desc["challenge_phase"]
        for phase, known in self.calls:
            for i, v in known.items():
                assert v == (got[i] if cp[i] < phase else 0), "callback of phase %d: challenge %d" % (phase, i)
        return got

    def vk(self):
        f, p = self.pk.commitments()
        return PR.VerifyingKey(self.c.desc, [zu.point_to_ints(x) for x in f], [zu.point_to_ints(x) for x in p], TAU, REPR)

    def opk(self):
        c = self.c
        return PR.keygen(PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])), c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)

    def free(self):
        for d in self.d_adv:
            d.free()
        for pk in self.pks[1:]:
            pk.free()
        self.pk.free()
        self.params.free()


def expected(monkeypatch, dev, opk, seed, ch, transcript="blake2b", multiopen="shplonk"):
    return PO.create_proof(monkeypatch, opk, dev.c.desc, dev.inst_ints, dev.adv, seed, ch, transcript=transcript, multiopen=multiopen)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_phased_proof_bytes_equal_the_harness(ctx, pkg, plonk, oracle, monkeypatch, k):
    """Two and three phases: the device's bytes are the harness's, the challenges it handed to the callback are the ones
    the harness's transcript squeezes, the wrapped verifier accepts the proof under a VK made of the device's
    commitments, and a second proof on the same key gives the same bytes (the workspace is reused cleanly)."""
    for three in (False, True):
        c = PC.rlc_circuit(plonk, k, seed=k, three_phases=three)
        dev = Device(ctx, pkg, plonk, oracle, c)
        got = dev.prove(seed=31)
        ch = dev.challenges()
        assert len(ch) == (2 if three else 1) and all(0 < v < zu.R for v in ch)
        assert len(got) == plonk.proof_size(ctx, dev.pk)
        opk = dev.opk()
        fk, pk_ = dev.pk.commitments()
        assert [zu.point_to_ints(x) for x in fk] == opk.fixed_commitments and [zu.point_to_ints(x) for x in pk_] == opk.permutation_commitments
        assert got == expected(monkeypatch, dev, opk, 31, ch)
        assert PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, got, ch)
        assert dev.prove(seed=31) == got and dev.challenges() == ch
        assert dev.prove(seed=32) != got
        dev.free()


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("transcript", ["blake2b", "keccak"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_phased_proof_modes(ctx, pkg, plonk, oracle, monkeypatch, serial, transcript, multiopen):
    """Lanes and serial keys, both built-in transcripts, SHPLONK and GWC, a seed and the caller's scalars."""
    c = PC.rlc_circuit(plonk, 6, seed=4, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c, flags=plonk.KEYGEN_SERIAL if serial else 0)
    tk = (plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM) | (plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0)
    got = dev.prove(seed=8, transcript=tk)
    ch = dev.challenges()
    assert got == expected(monkeypatch, dev, dev.opk(), 8, ch, transcript=transcript, multiopen=multiopen)
    assert PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, got, ch, transcript=transcript, multiopen=multiopen)
    cnt = plonk.proof_random_count(ctx, dev.pk)
    rng = PR.ChaCha20Rng(8)
    draws = zu.ints_to_fr(oracle, [rng.fr() for _ in range(cnt)])  # upstream's (phased) draw order is the stream's order
    assert dev.prove(scalars=draws, transcript=tk) == got
    with pytest.raises(pkg.AmdzkError, match="scalars given"):
        dev.prove(scalars=draws[:-1], transcript=tk)
    dev.free()


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("transcript", ["blake2b", "keccak"])
def test_phased_proof_of_two_instances(ctx, pkg, plonk, oracle, monkeypatch, three, transcript):
    """N = 2 on a key and a workspace clone: phases outside, instances inside — commitments, draws and the callback."""
    c = PC.rlc_circuit(plonk, 5, seed=6, three_phases=three)
    dev = Device(ctx, pkg, plonk, oracle, c, N=2)
    tk = plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM
    got = dev.prove(seed=12, transcript=tk)
    ch = dev.challenges()
    assert len(got) == plonk.proof_size_multi(ctx, dev.pk, 2, tk)
    assert got == expected(monkeypatch, dev, dev.opk(), 12, ch, transcript=transcript)
    assert PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, got, ch, transcript=transcript)
    assert dev.prove(seed=12, transcript=tk) == got
    dev.free()


@pytest.mark.parametrize("three", [False, True])
def test_columns_need_not_be_ordered_by_phase(ctx, pkg, plonk, oracle, monkeypatch, three):
    """The library takes any assignment of columns to phases: with the columns declared a, r, b(, s) — phases 0, 1, 0(, 2),
    so phase 0 is two runs of columns — and every query made in the same order, the proof is byte for byte the one of the
    circuit whose columns are ordered by phase (which is the one the harness can produce)."""
    c = PC.rlc_circuit(plonk, 6, seed=7, three_phases=three, interleaved=True)
    assert c.desc["advice_column_phase"] == ([0, 1, 0, 2] if three else [0, 1, 0])
    dev = Device(ctx, pkg, plonk, oracle, c)
    got = dev.prove(seed=21)
    ch = dev.challenges()
    c0 = PC.rlc_circuit(plonk, 6, seed=7, three_phases=three)
    adv0 = [list(col) for col in c0.advice]
    for phase in range(1, 3 if three else 2):
        c0.fill(phase, dict(enumerate(ch)), adv0)
    opk0 = PR.keygen(PO.specialise(c0.desc, [0] * len(ch)), c0.fixed, c0.assembly.mapping, TAU, transcript_repr=REPR)
    assert got == PO.create_proof(monkeypatch, opk0, c0.desc, [c0.instances], [adv0], 21, ch)
    assert dev.prove(seed=21) == got
    dev.free()


def test_witness_that_ignores_the_challenge_does_not_verify(ctx, pkg, plonk, oracle, monkeypatch):
    c = PC.rlc_circuit(plonk, 6, seed=3, ignore_challenge=True)
    dev = Device(ctx, pkg, plonk, oracle, c)
    got = dev.prove(seed=5)
    ch = dev.challenges()
    with pytest.raises(AssertionError):
        PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, got, ch)
    dev.free()


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_phased_circuits(ctx, pkg, plonk, oracle, monkeypatch, seed):
    c = PC.random_phased_circuit(plonk, 5, seed=seed)
    dev = Device(ctx, pkg, plonk, oracle, c, flags=plonk.KEYGEN_SERIAL if seed % 3 == 0 else 0)
    got = dev.prove(seed=seed)
    ch = dev.challenges()
    assert got == expected(monkeypatch, dev, dev.opk(), seed, ch)
    assert PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, got, ch)
    dev.free()


def test_phase_zero_key_through_the_new_entry_points_gives_todays_bytes(ctx, pkg, plonk, oracle):
    """A phase table without later phases and challenges is amdzk_keygen_ex; amdzk_create_proof_opts on it is
    amdzk_create_proof_multi — the oracle's plain bytes."""
    c = circuits.lookup_circuit(plonk, 6, seed=9)
    desc = dict(c.desc, advice_column_phase=[0] * c.desc["num_advice"], challenge_phase=[])
    g, gl = _srs_cache.setdefault(c.k, zu.test_srs(oracle, c.k, TAU))
    params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
    want = PR.create_proof(PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR), c.instances, c.advice, seed=5)
    for d in (c.desc, desc):
        pk = plonk.ProvingKey(ctx, params, d, fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=0)
        assert plonk.create_proof(ctx, pk, inst, d_adv, seed=5) == want
        assert plonk.create_proof_opts(ctx, [pk], [inst], [d_adv], seed=5) == want
        assert len(pk.inspect(3)) == 0
        pk.free()
    d_adv.free(); params.free()


# ---- phase-table validation and refusals: each is AMDZK_E_INVALID with a message, and the ctx goes on proving ----------
def test_phase_table_validation_messages(ctx, pkg, plonk, oracle, monkeypatch):
    c = PC.rlc_circuit(plonk, 5, seed=1)
    dev = Device(ctx, pkg, plonk, oracle, c)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])

    def keygen(desc, phases=None):
        return plonk.ProvingKey(ctx, dev.params, desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=0, phases=phases)

    bad = [(dict(c.desc, advice_column_phase=[0, 0, 3]), "advice column 2 is in phase 3"),
           (dict(c.desc, advice_column_phase=[0, 0, 2]), "phase 2 has advice columns but phase 1 has none"),
           (dict(c.desc, advice_column_phase=[1, 1, 1]), "phase 1 has advice columns but phase 0 has none"),
           (dict(c.desc, challenge_phase=[2]), "challenge 0 is usable after phase 2, which has no advice column"),
           (dict(c.desc, challenge_phase=[3]), "challenge 0 is usable after phase 3"),
           (dict(c.desc, challenge_phase=[]), "challenge index 0 out of range")]
    for desc, msg in bad:
        with pytest.raises(pkg.AmdzkError, match=msg) as e:
            keygen(desc)
        assert e.value.code == -2
    # through the entry points without a phase table a CHALLENGE word stays a bad expression word
    plain = {k_: v for k_, v in c.desc.items() if k_ not in ("advice_column_phase", "challenge_phase")}
    with pytest.raises(pkg.AmdzkError, match="bad expression word 09000000") as e:
        keygen(plain)
    assert e.value.code == -2
    # the same ctx then proves correctly
    got = dev.prove(seed=3)
    assert got == expected(monkeypatch, dev, dev.opk(), 3, dev.challenges())
    dev.free()


def test_refusals_leave_the_ctx_usable(ctx, pkg, plonk, oracle, monkeypatch):
    c = PC.rlc_circuit(plonk, 5, seed=2, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c)
    want = dev.prove(seed=3)
    ch = dev.challenges()
    assert want == expected(monkeypatch, dev, dev.opk(), 3, ch)
    # a phased key proved without a callback: through the new entry point and through the old ones
    with pytest.raises(pkg.AmdzkError, match="phase callback is needed") as e:
        dev.prove(seed=3, synthesize=None)
    assert e.value.code == -2
    with pytest.raises(pkg.AmdzkError, match="phase callback is needed"):
        plonk.create_proof(ctx, dev.pk, dev.inst[0], dev.d_adv[0], seed=3)
    assert dev.prove(seed=3) == want
    # a callback that returns non-zero, in the first and in the second callback
    for fail_in in (1, 2):
        def failing(phase, challenges, stream, fail_in=fail_in):
            if phase == fail_in:
                return 7
            return dev.synthesize(phase, challenges, stream)
        with pytest.raises(pkg.AmdzkError, match="phase callback returned 7 in phase %d" % fail_in) as e:
            dev.prove(seed=3, synthesize=failing)
        assert e.value.code == -2
        assert dev.prove(seed=3) == want
    # an exception in the Python callback comes back as that exception, not as a crash
    def raising(phase, challenges, stream):
        raise KeyError("synthesize failed")
    with pytest.raises(KeyError):
        dev.prove(seed=3, synthesize=raising)
    assert dev.prove(seed=3) == want
    # an undersized amdzk_proof_opts.size
    with pytest.raises(pkg.AmdzkError, match="amdzk_proof_opts.size is 8") as e:
        dev.prove(seed=3, opts_size=8)
    assert e.value.code == -2
    assert dev.prove(seed=3) == want and dev.challenges() == ch
    dev.free()


# ---- caller-owned transcript -----------------------------------------------------------------------------------------
class ForwardedTranscript:
    """The oracle's own transcript writer, fed only through the library's callbacks (Montgomery words in, ints inside)."""

    def __init__(self, inner, multiopen=0):
        self.inner, self.multiopen, self.calls = inner, multiopen, 0

    def _pt(self, w):
        self.calls += 1
        return zu.point_to_ints(w)

    def common_point(self, w):
        self.inner.common_point(self._pt(w))

    def write_point(self, w):
        self.inner.write_point(self._pt(w))

    def common_scalar(self, w):
        self.calls += 1
        self.inner.common_scalar(zu.fr_to_int(w))

    def write_scalar(self, w):
        self.calls += 1
        self.inner.write_scalar(zu.fr_to_int(w))

    def squeeze_challenge(self):
        self.calls += 1
        return zu.fr_from_int(self.inner.squeeze_challenge())


@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_callers_blake2b_reproduces_the_builtin_transcript(ctx, pkg, plonk, oracle, monkeypatch, multiopen):
    mo = plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0
    # a phase-0 circuit ...
    c = circuits.lookup_circuit(plonk, 6, seed=9)
    g, gl = _srs_cache.setdefault(c.k, zu.test_srs(oracle, c.k, TAU))
    params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
    pk = plonk.ProvingKey(ctx, params, c.desc, np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]), c.assembly.mapping, zu.fr_from_int(REPR))
    adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
    builtin = plonk.create_proof(ctx, pk, inst, d_adv, seed=5, transcript=mo)
    t = ForwardedTranscript(PR.Blake2bWrite(), multiopen=mo)
    assert plonk.create_proof(ctx, pk, inst, d_adv, seed=5, transcript=t) == b""  # the bytes are the caller's
    assert bytes(t.inner.proof) == builtin and t.calls > 0
    assert plonk.create_proof(ctx, pk, inst, d_adv, seed=5, transcript=mo) == builtin
    d_adv.free(); pk.free(); params.free()
    # ... and a phased one, with both callbacks at once
    c = PC.rlc_circuit(plonk, 6, seed=4, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c)
    builtin = dev.prove(seed=8, transcript=mo)
    ch = dev.challenges()
    t = ForwardedTranscript(PR.Blake2bWrite())
    assert dev.prove(seed=8, transcript=mo, transcript_object=t) == b""
    assert bytes(t.inner.proof) == builtin and dev.challenges() == ch
    dev.free()


def test_callers_blake2b_on_the_benchmark_shape_at_k15(ctx, pkg, plonk, oracle):
    """141 advice columns at k = 15, device against device: the caller's Blake2b through ~500 callbacks gives the bytes
    of the built-in transcript."""
    import time
    c = circuits.full_aadhaar_shape(plonk, k=15)
    assert c.desc["num_advice"] == 141
    g, gl = _srs_cache.setdefault(c.k, zu.test_srs(oracle, c.k, TAU))
    params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
    pk = plonk.ProvingKey(ctx, params, c.desc, np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]), c.assembly.mapping, zu.fr_from_int(REPR))
    adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]
    builtin = plonk.create_proof(ctx, pk, inst, d_adv, seed=5)
    t0 = time.perf_counter()
    assert plonk.create_proof(ctx, pk, inst, d_adv, seed=5) == builtin
    t1 = time.perf_counter()
    t = ForwardedTranscript(PR.Blake2bWrite())
    assert plonk.create_proof(ctx, pk, inst, d_adv, seed=5, transcript=t) == b""
    t2 = time.perf_counter()
    print("k=15, 141 advice: built-in transcript %.1f ms, Python-callback transcript %.1f ms (%d callbacks)"
          % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, t.calls))
    assert bytes(t.inner.proof) == builtin
    d_adv.free(); pk.free(); params.free()


def test_third_transcript_sha256_verifies_under_the_matching_reader(ctx, pkg, plonk, oracle, monkeypatch):
    """A transcript the library knows nothing about (SHA-256, its own framing, 64-byte big-endian points): the proof the
    caller's object collected verifies under the oracle's verifier reading with the matching reader — for a phase-0 circuit
    and, through the phased wrapper around that reader, for a phased one."""
    c = PC.rlc_circuit(plonk, 6, seed=4, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c)
    t = ForwardedTranscript(PO.Sha256Write())
    assert dev.prove(seed=8, transcript_object=t) == b""
    ch = dev.challenges()
    proof = bytes(t.inner.proof)
    assert len(proof) > 0 and proof != dev.prove(seed=8)
    assert PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, proof, ch, transcript="sha256")
    tampered = bytearray(proof)
    tampered[-1] ^= 1
    with pytest.raises(AssertionError):
        PO.verify_proof(monkeypatch, dev.vk(), c.desc, dev.inst_ints, bytes(tampered), ch, transcript="sha256")
    # a transcript callback that fails ends the proof with AMDZK_E_INVALID, and the ctx goes on proving
    class Failing(ForwardedTranscript):
        def write_scalar(self, w):
            return 3
    with pytest.raises(pkg.AmdzkError, match="transcript reported an error") as e:
        dev.prove(seed=8, transcript_object=Failing(PO.Sha256Write()))
    assert e.value.code == -2
    t2 = ForwardedTranscript(PO.Sha256Write())
    dev.prove(seed=8, transcript_object=t2)
    assert bytes(t2.inner.proof) == proof
    dev.free()


# ---- two instances: every instance's work is enqueued before the first write, the writes keep upstream's order -----------
class TwoInstances:
    """An unphased circuit on a key and a workspace clone, instance 1's witness `adv1` (advice ints) in a buffer of its own."""

    def __init__(self, ctx, pkg, plonk, oracle, c, adv1, flags=None):
        self.ctx, self.plonk, self.oracle, self.c = ctx, plonk, oracle, c
        g, gl = _srs_cache.setdefault(c.k, zu.test_srs(oracle, c.k, TAU))
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]), c.assembly.mapping,
                                   zu.fr_from_int(REPR), flags=flags)
        self.pks = [self.pk, self.pk.clone_workspace()]
        self.inst = [[zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]] * 2
        self.inst_ints = [c.instances] * 2
        self.d_adv = [ctx.alloc(len(c.advice) * c.n * 32) for _ in range(2)]
        self.set(0, c.advice)
        self.set(1, adv1)
        self.opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)

    def set(self, ci, adv):
        self.d_adv[ci].upload(np.stack([zu.ints_to_fr(self.oracle, col) for col in adv]))

    def prove(self, seed, transcript=0, transcript_object=None):
        return self.plonk.create_proof_opts(self.ctx, self.pks, self.inst, self.d_adv, seed=seed, transcript=transcript,
                                            transcript_object=transcript_object)

    def free(self):
        for d in self.d_adv:
            d.free()
        self.pks[1].free()
        self.pk.free()
        self.params.free()


def range_lookup_variants(c):
    """Instance 1's witnesses of a circuits.lookup_circuit: one whose first range-checked cell is another value of the table
    (gates and copies are not the prover's business), one whose cell is outside it (lookup 0 fails)."""
    row = [r for r in range(c.usable) if c.fixed[2][r] == 1][0]  # fixed[2] = q_rng
    good, bad = [list(col) for col in c.advice], [list(col) for col in c.advice]
    good[0][row] = (good[0][row] + 1) % 8
    bad[0][row] = 9
    return good, bad


NOT_IN_TABLE = "create_proof: lookup 0 input not in table (ConstraintSystemFailure)"


def test_instance_one_fails_its_lookup_behind_instance_zeros_writes(ctx, pkg, plonk, oracle, monkeypatch):
    """N = 2 with a caller's transcript, instance 1's lookup input outside its table: the transcript receives exactly the
    calls the oracle's prover makes until it hits that lookup — both instances' inputs and advice, theta, instance 0's
    permuted pairs — and nothing of instance 1's; status and message are the single proof's; the handles prove on."""
    c = circuits.lookup_circuit(plonk, 5, seed=4)
    good, bad = range_lookup_variants(c)
    dev = TwoInstances(ctx, pkg, plonk, oracle, c, bad)
    want = []
    with monkeypatch.context() as m:
        m.setattr(PR, "Blake2bWrite", ST.recording(PR.Blake2bWrite, want))
        with pytest.raises(AssertionError, match="lookup input not in table"):
            PR.create_proof_multi(dev.opk, dev.inst_ints, [c.advice, bad], seed=21)
    A, L = len(c.advice), len(c.desc["lookups"])
    assert [n for n, _ in want].count("write_point") == 2 * A + 2 * L and want[-1][0] == "write_point"  # ... and ends behind instance 0's pairs
    got = []
    with pytest.raises(pkg.AmdzkError) as e:
        dev.prove(21, transcript_object=ForwardedTranscript(ST.recording(PR.Blake2bWrite, got)()))
    assert e.value.code == -2 and str(e.value) == "amdzk error -2: " + NOT_IN_TABLE
    assert got == want
    dev.set(1, good)
    assert dev.prove(21) == PR.create_proof_multi(dev.opk, dev.inst_ints, [c.advice, good], seed=21)
    dev.free()


def test_instance_one_fails_its_lookup_on_a_three_phase_key(ctx, pkg, plonk, oracle, monkeypatch):
    """The same on a key with three phases: instance 1's phase-0 column `a` leaves the table at one row (a + ch * b is looked
    up). Both callbacks have run, every phase's commitments of both instances and the phase challenges are in the
    transcript, then theta and instance 0's pair."""
    c = PC.rlc_circuit(plonk, 5, seed=6, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c, N=2)
    adv1, fill1 = dev.wit[1]
    broken = [list(col) for col in adv1]
    broken[0][3] = (broken[0][3] + 1) % zu.R  # (a + 1, b) is no pair of the table
    dev.wit[1] = (broken, fill1)
    got, want = [], []
    with pytest.raises(pkg.AmdzkError) as e:
        dev.prove(seed=12, transcript_object=ForwardedTranscript(ST.recording(PR.Blake2bWrite, got)()))
    assert e.value.code == -2 and str(e.value) == "amdzk error -2: " + NOT_IN_TABLE
    ch = dev.challenges()  # both callbacks came, with the challenges pk_inspect reports
    PO.WRITERS["recording"] = ("Keccak256Write", "Keccak256Read", ST.recording(PR.Blake2bWrite, want), PR.Blake2bRead)
    try:
        with pytest.raises(AssertionError, match="lookup input not in table"):
            PO.create_proof(monkeypatch, dev.opk(), c.desc, dev.inst_ints, dev.adv, 12, ch, transcript="recording")
    finally:
        del PO.WRITERS["recording"]
    A = len(c.advice)
    assert [n for n, _ in want].count("write_point") == 2 * A + 2 and [n for n, _ in want].count("squeeze_challenge") == len(ch) + 1
    assert got == want
    dev.wit[1] = (adv1, fill1)
    proof = dev.prove(seed=12)
    assert proof == expected(monkeypatch, dev, dev.opk(), 12, dev.challenges())
    dev.free()


@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("transcript", ["blake2b", "keccak"])
def test_two_instances_open_with_gwc(ctx, pkg, plonk, oracle, monkeypatch, serial, transcript):
    """N = 2 with ProverGWC, on a three-phase key and on an unphased one, lanes keys and serial keys, both transcripts."""
    flags = plonk.KEYGEN_SERIAL if serial else 0
    tk = (plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM) | plonk.MULTIOPEN_GWC
    c = PC.rlc_circuit(plonk, 5, seed=6, three_phases=True)
    dev = Device(ctx, pkg, plonk, oracle, c, N=2, flags=flags)
    got = dev.prove(seed=12, transcript=tk)
    assert len(got) == plonk.proof_size_multi(ctx, dev.pk, 2, tk)
    assert got == expected(monkeypatch, dev, dev.opk(), 12, dev.challenges(), transcript=transcript, multiopen="gwc")
    dev.free()
    c = circuits.lookup_circuit(plonk, 5, seed=4)
    good, _ = range_lookup_variants(c)
    two = TwoInstances(ctx, pkg, plonk, oracle, c, good, flags=flags)
    assert two.prove(17, transcript=tk) == PR.create_proof_multi(two.opk, two.inst_ints, [c.advice, good], seed=17, transcript=transcript, multiopen="gwc")
    two.free()
