"""What the amdzk_create_proof_batch_opts tests share: a batch of members — circuits of any kind on ONE ParamsKZG, each with
its own workspace, witness and device buffer — the batch-wide phase callback that fills the later phases from the circuits'
own `fill`, the expected bytes (tests/phased_oracle.py for a phased member, oracle/plonk_ref.py for the others) and the raw
ctypes call for the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import phased_oracle as PO  # noqa: E402
import plonk_ref as PR  # noqa: E402

TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
INVALID = -2
_srs_cache = {}


def srs(oracle, k):
    if k not in _srs_cache:
        _srs_cache[k] = zu.test_srs(oracle, k, TAU)
    return _srs_cache[k]


def phases_of(c):
    return max(c.desc.get("advice_column_phase", [0]) or [0]) + 1


def is_phased(c):
    return bool(c.desc.get("challenge_phase")) or phases_of(c) > 1


class Member:
    """One proof of a batch: its circuit, workspace handle, witness (advice ints, fill or None, instance ints), buffer."""

    def __init__(self, c, pk, adv, fill, inst_ints):
        self.c, self.pk, self.adv0, self.fill, self.inst_ints = c, pk, adv, fill, inst_ints
        self.adv = None


class Batch:
    """members: (circuit, witness) pairs; witness None = the circuit's own, an int = c.witness_for(seed) (phased) or
    c.witness(seed), or an explicit (advice ints, instance ints). Members of one circuit object share a key: the first gets
    the key, the others workspace clones. All keys are made on one ParamsKZG unless a member names another (c, w, params)."""

    def __init__(self, ctx, pkg, plonk, oracle, k, members):
        self.ctx, self.pkg, self.plonk, self.oracle, self.k = ctx, pkg, plonk, oracle, k
        g, gl = srs(oracle, k)
        self.params = pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)
        self.keys, self.opks, self.m, self.calls = {}, {}, [], []
        for c, w in members:
            assert c.k == k
            if id(c) not in self.keys:
                fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]) if c.fixed else np.zeros((0, c.n, 4), np.uint64)
                pk = self.keys[id(c)] = plonk.ProvingKey(ctx, self.params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR))
            else:
                pk = self.keys[id(c)].clone_workspace()
            if is_phased(c):
                adv, fill = (c.advice, c.fill) if w is None else c.witness_for(w)
                inst = c.instances
            elif w is None:
                adv, fill, inst = c.advice, None, c.instances
            elif isinstance(w, int):
                (adv, inst), fill = c.witness(w), None
            else:
                (adv, inst), fill = w, None
            self.m.append(Member(c, pk, adv, fill, inst))
        self.inst = [[zu.ints_to_fr(oracle, col) if len(col) else np.zeros((0, 4), np.uint64) for col in m.inst_ints] for m in self.m]
        self.d_adv = [ctx.alloc(max(1, len(m.adv0)) * m.c.n * 32) for m in self.m]
        self.pks = [m.pk for m in self.m]
        self.on_phase = None  # test hook: (phase, wanted, chal) -> what synthesize returns

    def reset(self, idx=None):
        """Fresh witnesses: phase-0 columns uploaded, later phases zero on the host and on the device."""
        for b in (range(len(self.m)) if idx is None else idx):
            m = self.m[b]
            m.adv = [list(col) for col in m.adv0]
            self.d_adv[b].upload(np.stack([zu.ints_to_fr(self.oracle, col) for col in m.adv]))
        self.calls = []

    def fill_and_upload(self, b, phase, known):
        m = self.m[b]
        m.fill(phase, known, m.adv)
        ap = m.c.desc["advice_column_phase"]
        for col in range(len(ap)):
            if ap[col] == phase:
                host = np.ascontiguousarray(zu.ints_to_fr(self.oracle, m.adv[col]))
                self.ctx._chk(self.ctx.L.amdzk_dev_upload(self.ctx.h, C.c_void_p(self.d_adv[b].ptr.value + col * m.c.n * 32), host.ctypes.data, host.nbytes))

    def synthesize_for(self, idx):
        """The batch callback for the members idx (batch position j = member idx[j])."""
        def synthesize(phase, wanted, chal, stream):
            self.calls.append((phase, wanted.copy(), chal.copy()))
            assert len(wanted) == len(idx) and chal.shape[0] == len(idx)
            for j, b in enumerate(idx):
                nch = len(self.m[b].c.desc.get("challenge_phase", []))
                if wanted[j]:
                    self.fill_and_upload(b, phase, {i: zu.fr_to_int(chal[j, i]) for i in range(nch)})
            return self.on_phase(phase, wanted, chal) if self.on_phase else None
        return synthesize

    def batch(self, seeds, idx=None, transcript=0, **kw):
        idx = list(range(len(self.m))) if idx is None else idx
        self.reset(idx)
        kw.setdefault("synthesize", self.synthesize_for(idx))
        return self.plonk.create_proof_batch_opts(self.ctx, [self.pks[b] for b in idx], [self.inst[b] for b in idx], [self.d_adv[b] for b in idx],
                                                  seeds=seeds, transcript=transcript, **kw)

    def single(self, b, seed, transcript=0, transcript_object=None):
        """amdzk_create_proof_opts on member b's workspace alone."""
        self.reset([b])
        m = self.m[b]

        def syn(phase, challenges, stream):
            self.fill_and_upload(b, phase, {i: zu.fr_to_int(challenges[i]) for i in range(len(challenges))})
        return self.plonk.create_proof_opts(self.ctx, [m.pk], [self.inst[b]], [self.d_adv[b]], seed=seed, transcript=transcript,
                                            synthesize=syn if m.fill else None, transcript_object=transcript_object)

    def challenges(self, b):
        return [zu.fr_to_int(x) for x in self.m[b].pk.inspect(3)]

    def check_calls(self, idx, live=None):
        """One callback per phase >= 1 that some live member has, with n_proofs = len(idx); wanted = live and has the phase; a
        wanted proof sees its finished phases' challenges (= pk_inspect's) and zero elsewhere, the others all zero."""
        live = [True] * len(idx) if live is None else live
        top = max([phases_of(self.m[b].c) for j, b in enumerate(idx) if live[j]] + [1])
        assert [p for p, _, _ in self.calls] == list(range(1, top)), "one callback per phase >= 1, in order"
        stride = max(len(self.m[b].c.desc.get("challenge_phase", [])) for b in idx)
        for phase, wanted, chal in self.calls:
            assert chal.shape == (len(idx), stride, 4)
            for j, b in enumerate(idx):
                c = self.m[b].c
                assert wanted[j] == (1 if live[j] and phases_of(c) > phase else 0), "phase %d proof %d" % (phase, j)
                got = [zu.fr_to_int(chal[j, i]) for i in range(stride)]
                if not wanted[j]:
                    assert not any(got)
                    continue
                cp, ch = c.desc["challenge_phase"], self.challenges(b)
                assert got == [ch[i] if i < len(cp) and cp[i] < phase else 0 for i in range(stride)], "phase %d proof %d" % (phase, j)

    def opk(self, b):
        c = self.m[b].c
        if id(c) not in self.opks:
            desc = PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])) if is_phased(c) else c.desc
            self.opks[id(c)] = PR.keygen(desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        return self.opks[id(c)]

    def expected(self, monkeypatch, b, seed, ch=None, transcript="blake2b", multiopen="shplonk"):
        """The oracle's bytes of member b's proof; a phased member's on the challenges `ch` (its advice filled by the callback)."""
        m = self.m[b]
        if is_phased(m.c):
            return PO.create_proof(monkeypatch, self.opk(b), m.c.desc, [m.inst_ints], [m.adv], seed, ch, transcript=transcript, multiopen=multiopen)
        return PR.create_proof(self.opk(b), m.inst_ints, m.adv0, seed=seed, transcript=transcript, multiopen=multiopen)

    def free(self):
        for d in self.d_adv:
            d.free()
        for m in self.m:
            if m.pk not in self.keys.values():
                m.pk.free()
        for pk in self.keys.values():
            pk.free()
        self.params.free()


def raw_call(ctx, pkg, keys, adv, n, seeds=(), scalars=None, scalar_count=0, kind=0, transcripts=None, phase_fn=None, opts_size=None,
             proof_stride=1 << 14, advice_stride=None, opts_null=False, keys_null=False, lens_null=False, out_null=False, strict=False):
    """amdzk_create_proof_batch_opts (strict: amdzk_create_proof_batch, whose options end behind scalar_count) through ctypes
    with every argument as given (instances NULL). Returns (rc, statuses, lengths, message); statuses and lengths start at 1
    and 7."""
    N = len(keys)
    ffi = pkg.ffi
    karr = (C.c_void_p * max(1, N))(*keys)
    aarr = (C.c_void_p * max(1, N))(*adv)
    sd = np.array(list(seeds), np.uint64) if seeds is not None else None
    S = ffi.BatchOpts if strict else ffi.BatchProofOpts
    extra = () if strict else (transcripts, phase_fn if phase_fn is not None else ffi.BATCH_PHASE_FN(), None)
    opts = S(C.sizeof(S) if opts_size is None else opts_size, kind, sd.ctypes.data if sd is not None and sd.size else None, scalars, scalar_count, *extra)
    buf = (C.c_uint8 * max(1, proof_stride * N))()
    lens_out, st = (C.c_size_t * max(1, N))(*[7] * N), (C.c_int * max(1, N))(*[1] * N)
    fn = ctx.L.amdzk_create_proof_batch if strict else ctx.L.amdzk_create_proof_batch_opts
    rc = fn(ctx.h, None if keys_null else karr, N, None, None, aarr, advice_stride if advice_stride is not None else n,
            None if opts_null else C.byref(opts), None if out_null else buf, proof_stride, None if lens_null else lens_out, st)
    return rc, list(st)[:N], list(lens_out)[:N], ctx.L.amdzk_last_error(ctx.h).decode()
