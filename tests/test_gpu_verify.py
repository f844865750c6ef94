"""GPU: amdzk_verify_proofs — plonk::verify_proof up to the pairing — on proofs the device prover made of the small circuits
of tests/verify_cases.py. The pair (L, R) must equal tests/verify_ref.py's as group elements, and tau * L == R with the tau
the test SRS was made from stands in for the caller's pairing. Decode classes at exact offsets, random single-byte mutations
against the oracle's decision, batches with caller-supplied and seeded weights, refusals, the Python mirror."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, REPR, Q, R = VC.TAU, VC.REPR, zu.Q, zu.R
_srs = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


class Rig:
    """One circuit on the device: the key, workspace clones for N instances, the witness, and the proofs made so far."""

    def __init__(self, ctx, pkg, plonk, oracle, name, N):
        self.ctx, self.plonk, self.name, self.N = ctx, plonk, name, N
        self.c, self.opk = VC.oracle_key(plonk, name)
        c = self.c
        self.phased = "challenge_phase" in c.desc
        self.proofs = {}
        if self.phased:
            from test_gpu_phased import Device
            self.dev = Device(ctx, pkg, plonk, oracle, c, N=N)
            self.pk, self.params, self.inst = self.dev.pk, self.dev.params, self.dev.inst[0]
            return
        if c.k not in _srs:
            _srs[c.k] = zu.test_srs(oracle, c.k, TAU)
        g, gl = _srs[c.k]
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR))
        self.pks = [self.pk] + [self.pk.clone_workspace() for _ in range(N - 1)]
        adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
        self.d_adv = [ctx.alloc(adv.nbytes).upload(adv) for _ in range(N)]
        self.inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]

    def case(self, transcript, multiopen, seed=5):
        """A proof by the device prover, as a verify_cases.Case (reference key: the oracle's)."""
        key = (transcript, multiopen, seed)
        if key not in self.proofs:
            flags = VC.kind_flags(self.plonk, transcript, multiopen)
            ch = None
            if self.phased:
                proof = self.dev.prove(seed=seed, transcript=flags)
                ch = self.dev.challenges()
            elif self.N == 1:
                proof = self.plonk.create_proof(self.ctx, self.pk, self.inst, self.d_adv[0], seed=seed, transcript=flags)
            else:
                proof = self.plonk.create_proof_multi(self.ctx, self.pks, [self.inst] * self.N, self.d_adv, seed=seed, transcript=flags)
            self.proofs[key] = VC.Case(self.name, self.c, self.c.desc, self.opk, [self.c.instances] * self.N, proof, transcript, multiopen, ch)
        return self.proofs[key]

    def instances_arg(self):
        return self.inst if self.N == 1 else [self.inst] * self.N

    def verify(self, case, proofs, pk=None, **kw):
        """verify_proofs on proofs of this rig's circuit made like `case`."""
        return self.plonk.verify_proofs(self.ctx, pk or self.pk, [self.instances_arg()] * len(proofs), proofs,
                                        transcript=VC.kind_flags(self.plonk, case.transcript, case.multiopen), n_circuits=self.N, **kw)

    def free(self):
        if self.phased:
            return self.dev.free()
        for d in self.d_adv:
            d.free()
        for pk in self.pks[1:]:
            pk.free()
        self.pk.free()
        self.params.free()


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


def ints(guard):
    return zu.point_to_ints(guard.lhs), zu.point_to_ints(guard.rhs)


# ------------------------------------------------------------------------------------ accepted proofs
@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_accepted_proofs_give_the_reference_pair(plonk, rigs, name, N, transcript, multiopen):
    rig = rigs(name, N)
    case = rig.case(transcript, multiopen)
    assert case.accepts(), "the device's proof is not accepted by the oracle"
    g = plonk.verify_proof(rig.ctx, rig.pk, rig.instances_arg(), case.proof, transcript=VC.kind_flags(plonk, transcript, multiopen), n_circuits=N)
    assert g.statuses == [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)] and g.well_formed
    got = ints(g)
    assert got[0] is not None and got[1] is not None
    assert got == case.pair()
    assert VR.holds(got, TAU)


def test_workspace_clones_and_keys_from_a_key_file_verify_the_same(ctx, plonk, rigs):
    rig = rigs("lookup")
    case = rig.case("blake2b", "shplonk")
    want = case.pair()
    clone = rig.pk.clone_workspace()
    loaded = plonk.ProvingKey.read(ctx, rig.params, rig.pk.write())
    try:
        for key in (clone, loaded):
            g = rig.verify(case, [case.proof], pk=key)
            assert g.well_formed and ints(g) == want
    finally:
        loaded.free()
        clone.free()


# ------------------------------------------------------------------------------------ decode classes
def nonresidue_x():
    """A small x whose cube plus 3 is a non-residue mod q: no curve point has it."""
    x = 1
    while pow((x * x * x + 3) % Q, (Q - 1) // 2, Q) == 1:
        x += 1
    return x


def positions(kinds, kind, size_p):
    """Byte offsets of the first, a middle and the last element of `kind` ('p' / 's')."""
    offs, off = [], 0
    for k in kinds:
        if k == kind:
            offs.append(off)
        off += size_p if k == "p" else 32
    return [offs[0], offs[len(offs) // 2], offs[-1]]


def put(proof, off, data):
    m = bytearray(proof)
    m[off:off + len(data)] = data
    return bytes(m)


@pytest.mark.parametrize("transcript", ["blake2b", "evm"])
def test_decode_classes_at_the_first_a_middle_and_the_last_element(plonk, rigs, transcript):
    rig = rigs("square")
    case = rig.case(transcript, "shplonk")
    evm = transcript == "evm"
    kinds = VR.element_kinds(case.desc, 1)
    psz, end = (64, "big") if evm else (32, "little")
    proof = case.proof
    malformed, false = [], []  # (bytes, expected status, expected offset) / bytes of well-formed false proofs
    for off in positions(kinds, "p", psz):
        if evm:
            x, y = int.from_bytes(proof[off:off + 32], "big"), int.from_bytes(proof[off + 32:off + 64], "big")
            xy = lambda a, b: a.to_bytes(32, "big") + b.to_bytes(32, "big")
            malformed += [(put(proof, off, xy(Q, y)), 2, off), (put(proof, off, xy(Q - 1, y)), 2, off), (put(proof, off, xy(x | 1 << 254, y)), 2, off),
                          (put(proof, off, xy(nonresidue_x(), y)), 2, off), (put(proof, off, bytes(64)), 2, off),
                          (put(proof, off, xy(x, (y + 1) % Q)), 2, off), (put(proof, off, xy(x, Q)), 2, off)]
            false.append(put(proof, off, xy(x, Q - y)))
        else:
            b = bytearray(proof[off:off + 32])
            sign = b[31] & 0x80
            le = lambda v, s=sign: bytes(v.to_bytes(32, "little")[:31]) + bytes([v.to_bytes(32, "little")[31] | s])
            assert pow(2, (Q - 1) // 2, Q) == 1  # x = q - 1 is on the curve: (-1)^3 + 3 = 2 is a square mod q (q = 7 mod 8)
            false.append(put(proof, off, le(Q - 1)))
            malformed += [(put(proof, off, le(Q)), 2, off), (put(proof, off, bytes(b[:31]) + bytes([b[31] | 0x40])), 2, off),
                          (put(proof, off, le(nonresidue_x())), 2, off), (put(proof, off, bytes(32)), 2, off)]
            false.append(put(proof, off, bytes(b[:31]) + bytes([b[31] ^ 0x80])))
    for off in positions(kinds, "s", psz):
        malformed.append((put(proof, off, R.to_bytes(32, end)), 3, off))
        malformed.append((put(proof, off, (2 ** 256 - 1).to_bytes(32, end)), 3, off))
        false.append(put(proof, off, (R - 1).to_bytes(32, end)))
    malformed += [(proof[:-1], 1, 0), (proof[:32], 1, 0), (proof + b"\0", 1, 0)]
    # two bad elements in one proof: the smaller offset is reported, whatever its class
    p_last, s_first = positions(kinds, "p", psz)[2], positions(kinds, "s", psz)[0]
    malformed.append((put(put(proof, p_last, bytes(psz)), s_first, R.to_bytes(32, end)), 3, s_first))
    for m, st, off in malformed:
        assert case.decode(m) == (st, off), "the reference decode disagrees with the expectation"
    # all malformed ones in ONE call, between two good proofs: each status is its own, the good ones are unaffected
    batch = [proof] + [m for m, _, _ in malformed] + [proof]
    rho = [zu.fr_from_int(3 + 5 * b) for b in range(len(batch))]
    g = rig.verify(case, batch, combine_scalars=np.stack(rho))
    assert [tuple(s) for s in g.statuses] == [(0, 0)] + [(st, off) for _, st, off in malformed] + [(0, 0)]
    good = case.pair()
    assert ints(g) == VR.combine([good, good], [3, 3 + 5 * (len(batch) - 1)])
    # well formed but false: the pair is the reference's and fails tau
    for m in false:
        assert case.decode(m) == (0, 0)
        one = rig.verify(case, [m])
        assert one.well_formed
        assert ints(one) == case.pair(m) and not VR.holds(ints(one), TAU)


@pytest.mark.parametrize("target", [63, 65, 67])
def test_a_bad_element_on_either_side_of_a_decode_block_in_a_single_key_batch(ctx, pkg, plonk, oracle, target):
    """The decode launch takes one block per (proof, 64 elements): proofs of E = 63 elements (one block, not full), of
    E = 65 (a second block of one element; elements 63 and 64 are the opening's two points) and of E = 67 (63 and 64 are scalars). In a batch of three, element 0, 63, 64 and E - 1 of the MIDDLE proof — those that
    exist — are corrupted one at a time, as a point or as a scalar, whichever the element is: the status names that byte offset
    and class, the neighbours stay well formed and the pair is that of the two good proofs under the same weights. Through a
    proving key and through a verifying key."""
    from test_gpu_verify_mixed import Own, padded_to  # that module imports this one
    params = pkg.kzg.ParamsKZG.setup(ctx, 4, zu.fr_from_int(TAU))
    rig = Own(ctx, pkg, plonk, oracle, "mixed_padded%d" % target, padded_to(plonk, target), params)
    vk = rig.pk.get_vk()
    try:
        cases = [rig.case("blake2b", "shplonk", seed=40 + b) for b in range(3)]
        proofs = [c.proof for c in cases]
        kinds = VR.element_kinds(cases[0].desc, 1)
        E = len(kinds)
        assert E == target == len(proofs[1]) // 32 and len(set(proofs)) == 3
        elements = sorted({e for e in (0, 63, 64, E - 1) if e < E})
        assert [(e, kinds[e]) for e in elements] == {63: [(0, "p"), (62, "p")], 65: [(0, "p"), (63, "p"), (64, "p")],
                                                     67: [(0, "p"), (63, "s"), (64, "s"), (66, "p")]}[target]
        bad = {"p": [(bytes(32), 2), (nonresidue_x().to_bytes(32, "little"), 2)], "s": [(R.to_bytes(32, "little"), 3), ((2 ** 256 - 1).to_bytes(32, "little"), 3)]}
        sc = np.stack([zu.fr_from_int(v) for v in (0x1357, R - 2, 0x2468ACE)])
        for key in (rig.pk, vk):
            want = rig.verify(cases[0], [proofs[0], proofs[2]], pk=key, combine_scalars=sc[[0, 2]])
            assert want.well_formed and VR.holds(ints(want), TAU)
            for e in elements:
                for data, cls in bad[kinds[e]]:
                    m = put(proofs[1], 32 * e, data)
                    assert cases[1].decode(m) == (cls, 32 * e), "the reference decode disagrees with the expectation"
                    g = rig.verify(cases[0], [proofs[0], m, proofs[2]], pk=key, combine_scalars=sc)
                    assert [tuple(s) for s in g.statuses] == [(0, 0), (cls, 32 * e), (0, 0)], (e, cls)
                    assert np.array_equal(g.lhs, want.lhs) and np.array_equal(g.rhs, want.rhs), (e, cls)
    finally:
        vk.free()
        rig.free()
        params.free()


# ------------------------------------------------------------------------------------ random single-byte mutations
@pytest.mark.parametrize("transcript,multiopen,seed", [("blake2b", "shplonk", 21), ("evm", "gwc", 2)])
def test_random_single_byte_mutations_agree_with_the_oracle(plonk, rigs, transcript, multiopen, seed):
    """Fixed seeds; with them the reference alone puts at least ten cases into "malformed" and ten into "rejected" per
    transcript (asserted below from the reference's verdicts, not from the device's)."""
    rig = rigs("square")
    case = rig.case(transcript, multiopen)
    rnd = random.Random(seed)
    muts = []
    for _ in range(28):
        m = bytearray(case.proof)
        m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
        muts.append(bytes(m))
    muts.append(case.proof)
    want = ["malformed" if case.decode(m)[0] else "accepted" if case.accepts(m) else "rejected" for m in muts]
    assert want.count("malformed") >= 10 and want.count("rejected") >= 10 and want[-1] == "accepted", want
    g = rig.verify(case, muts, combine_seed=99)
    got = []
    for m, s in zip(muts, g.statuses):
        assert tuple(s) == case.decode(m)
        if s.status:
            assert not case.accepts(m)
            got.append("malformed")
        else:
            got.append("accepted" if VR.holds(ints(rig.verify(case, [m])), TAU) else "rejected")
    assert got == want
    assert not VR.holds(ints(g), TAU)  # the batch holds false proofs


# ------------------------------------------------------------------------------------ batches
def test_batches_combine_with_the_callers_weights_by_position(plonk, rigs):
    rig = rigs("square")
    cases = [rig.case("blake2b", "shplonk", seed=20 + b) for b in range(7)]
    proofs = [c.proof for c in cases]
    assert len(set(proofs)) == 7
    # 7 proofs span more than two workgroups (of 64 threads) of the decode kernel
    assert 7 * len(VR.element_kinds(cases[0].desc, 1)) > 2 * 64
    singles = [ints(rig.verify(cases[b], [proofs[b]])) for b in range(7)]
    assert singles == [c.pair() for c in cases] and all(VR.holds(s, TAU) for s in singles)
    rho = [0x1234567 + 0x1F1F1F1F1F1F1F1F1F * b ** 3 for b in range(7)]
    rho[3] = R - 1
    sc = np.stack([zu.fr_from_int(v) for v in rho])
    for n in (1, 2, 7):
        g = rig.verify(cases[0], proofs[:n], combine_scalars=sc[:n])
        assert g.well_formed and len(g.statuses) == n
        assert ints(g) == VR.combine(singles[:n], rho[:n]) and VR.holds(ints(g), TAU)
    # positions 2 and 5 malformed: their statuses are set, the pair is the sum over the others, rho by POSITION
    bad = list(proofs)
    bad[2] = put(bad[2], 32, bytes(32))
    bad[5] = bad[5][:-1]
    g = rig.verify(cases[0], bad, combine_scalars=sc)
    assert [tuple(s) for s in g.statuses] == [(0, 0), (0, 0), (2, 32), (0, 0), (0, 0), (1, 0), (0, 0)]
    keep = [0, 1, 3, 4, 6]
    assert ints(g) == VR.combine([singles[b] for b in keep], [rho[b] for b in keep]) and VR.holds(ints(g), TAU)
    # one well-formed false proof among good ones: the batch fails, each good proof alone passes
    false = list(proofs)
    kinds = VR.element_kinds(cases[0].desc, 1)
    off = 32 * kinds.index("s")
    false[4] = put(false[4], off, ((int.from_bytes(false[4][off:off + 32], "little") + 1) % R).to_bytes(32, "little"))
    g = rig.verify(cases[0], false, combine_scalars=sc)
    assert g.well_formed and not VR.holds(ints(g), TAU)
    assert ints(g) == VR.combine(singles[:4] + [cases[4].pair(false[4])] + singles[5:], rho)
    # all malformed: both points are the identity
    g = rig.verify(cases[0], [p[:-1] for p in proofs[:3]], combine_scalars=sc[:3])
    assert [s.status for s in g.statuses] == [1, 1, 1] and ints(g) == (None, None)
    g = rig.verify(cases[0], [put(proofs[0], 0, bytes(32))])
    assert [tuple(s) for s in g.statuses] == [(2, 0)] and ints(g) == (None, None)


def test_seeded_weights_are_the_oracles_chacha_draws(plonk, rigs):
    rig = rigs("square")
    cases = [rig.case("evm", "shplonk", seed=30 + b) for b in range(3)]
    proofs = [c.proof for c in cases]
    singles = [c.pair() for c in cases]
    for seed in (0, 0xDEADBEEF12345):
        rng = PR.ChaCha20Rng(seed)
        rho = [rng.fr() for _ in range(3)]
        g = rig.verify(cases[0], proofs, combine_seed=seed)
        assert g.well_formed and ints(g) == VR.combine(singles, rho)
    # a single proof without weights of the caller's has weight 1, whatever the seed
    assert ints(rig.verify(cases[0], proofs[:1], combine_seed=77)) == singles[0]


def test_bad_instances_are_reported_by_column(plonk, rigs):
    rig = rigs("lookup")
    case = rig.case("blake2b", "shplonk")
    col = next(i for i, v in enumerate(rig.inst) if len(v))
    big = [v.copy() for v in rig.inst]
    big[col][0] = np.array(zu.limbs(R), dtype=np.uint64)  # the modulus itself: not a residue
    n, bf = 1 << case.desc["k"], case.desc["blinding_factors"]
    long_ = [v.copy() for v in rig.inst]
    long_[col] = np.zeros((n - bf, 4), np.uint64)  # one row more than the usable ones
    g = plonk.verify_proofs(rig.ctx, rig.pk, [rig.inst, big, long_], [case.proof] * 3, combine_scalars=np.stack([zu.fr_from_int(v) for v in (2, 3, 4)]))
    assert [tuple(s) for s in g.statuses] == [(0, 0), (4, col), (4, col)]
    assert ints(g) == VR.combine([case.pair()], [2])


# ------------------------------------------------------------------------------------ refusals, mirrors
def test_refusals_leave_the_ctx_and_the_key_usable(ctx, pkg, plonk, rigs):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk")
    L = ctx.L
    proof = (C.c_uint8 * len(case.proof)).from_buffer_copy(case.proof)
    pp = (C.c_void_p * 1)(C.addressof(proof))
    pl = (C.c_size_t * 1)(len(case.proof))
    cols = [np.ascontiguousarray(v) for v in rig.inst]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[v.ctypes.data if v.size else None for v in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[v.shape[0] for v in cols])
    ipp = (C.POINTER(C.c_void_p) * 1)(C.cast(ptrs, C.POINTER(C.c_void_p)))
    lpp = (C.POINTER(C.c_size_t) * 1)(C.cast(lens, C.POINTER(C.c_size_t)))
    st = (pkg.ffi.ProofStatus * 1)()
    pair = np.zeros(16, np.uint64)
    VO = pkg.ffi.VerifyOpts
    ok_opts = VO(C.sizeof(VO), 0, 1, 0, None)
    too_big = np.array(zu.limbs(R), dtype=np.uint64)

    def call(pk=rig.pk.h, n=1, inst=ipp, ln=lpp, proofs=pp, plens=pl, opts=ok_opts, status=st, out=pair.ctypes.data):
        return L.amdzk_verify_proofs(ctx.h, pk, n, inst, ln, proofs, plens, C.byref(opts) if opts is not None else None, status, out)

    refusals = [dict(pk=None), dict(proofs=None), dict(plens=None), dict(status=None), dict(out=None), dict(n=0),
                dict(opts=VO(C.sizeof(VO) - 1, 0, 1, 0, None)), dict(opts=VO(C.sizeof(VO), 2, 1, 0, None)),
                dict(opts=VO(C.sizeof(VO), 0x200, 1, 0, None)), dict(opts=VO(C.sizeof(VO), 0, 1, 0, too_big.ctypes.data))]
    if cols:
        refusals += [dict(inst=None), dict(ln=None)]
    want = rig.plonk.create_proof(ctx, rig.pk, rig.inst, rig.d_adv[0], seed=5)
    assert want == case.proof
    for kw in refusals:
        assert call(**kw) == -2, kw
        assert L.amdzk_last_error(ctx.h).decode().startswith("verify_proofs:"), (kw, L.amdzk_last_error(ctx.h))
        assert call() == 0 and (st[0].status, st[0].offset) == (0, 0)
        assert (zu.point_to_ints(pair[:8]), zu.point_to_ints(pair[8:])) == case.pair()
    assert call(opts=None) == 0 and (zu.point_to_ints(pair[:8]), zu.point_to_ints(pair[8:])) == case.pair()  # NULL opts: the defaults
    assert rig.plonk.create_proof(ctx, rig.pk, rig.inst, rig.d_adv[0], seed=5) == want  # a proof made afterwards has the usual bytes
    with pytest.raises(pkg.ffi.AmdzkError, match="verify_proofs:"):
        plonk.verify_proofs(ctx, rig.pk, [rig.inst], [case.proof], opts_size=8)


def test_python_mirror_names_status_and_offset_of_a_malformed_proof(plonk, rigs):
    rig = rigs("square")
    case = rig.case("blake2b", "shplonk")
    g = plonk.verify_proof(rig.ctx, rig.pk, rig.inst, case.proof)
    assert isinstance(g, plonk.Guard) and g.lhs.shape == (8,) and g.rhs.shape == (8,) and VR.holds(ints(g), TAU)
    with pytest.raises(ValueError, match=r"status 2 \(BAD_POINT\), offset 32"):
        plonk.verify_proof(rig.ctx, rig.pk, rig.inst, put(case.proof, 32, bytes(32)))
    with pytest.raises(ValueError, match=r"status 1 \(BAD_LENGTH\), offset 0"):
        plonk.verify_proof(rig.ctx, rig.pk, rig.inst, case.proof[:-1])
