"""GPU: verifying keys (amdzk_vk) — made from a proving key and by amdzk_keygen_vk alone, written, read, and verified with
after the proving key and the SRS are gone. Expected commitments and files come from the oracle's key through the
independent encoder tests/vk_blob.py; expected verdicts from the oracle side (verify_ref) and from the pk-taking calls,
which tests/test_gpu_verify*.py hold to the oracle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import pairing_ref as PRF  # noqa: E402
import plonk_ref as PR  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402
import vk_blob  # noqa: E402
from test_gpu_verify import Rig, put  # noqa: E402
from test_gpu_verify_decide import false_proof as make_false_proof  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, REPR, R = VC.TAU, VC.REPR, zu.R
G = PRF.G1_GEN  # g[0] of the test SRS: the generator
G2_WORDS = np.array(PRF.g2_words(PRF.G2_GEN), dtype=np.uint64)
S_G2_WORDS = np.array(PRF.g2_words(PRF.g2_mul(PRF.G2_GEN, TAU)), dtype=np.uint64)
NAMES = sorted({name for name, _, _ in VC.CASES})
BATCH_KINDS = [("square", "blake2b", "shplonk"), ("lookup", "evm", "gwc")]
_srs, _verdicts, _false = {}, {}, {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    """From two G2 points of the oracle side: the generator and tau times it."""
    v = pkg.kzg.ParamsVerifierKZG(ctx, G2_WORDS, S_G2_WORDS)
    yield v
    v.free()


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


def oracle_file(plonk, desc, opk, repr_=REPR, pair=False):
    return vk_blob.encode(plonk, desc, opk.fixed_commitments, opk.permutation_commitments, repr_, G, *((G2_WORDS, S_G2_WORDS) if pair else ()))


def oracle_verdict(case, proof):
    """test_gpu_verify_decide.oracle_verdict, once per distinct proof."""
    key = (case.name, case.N, case.transcript, case.multiopen, proof)
    if key not in _verdicts:
        _verdicts[key] = case.decode(proof) == (0, 0) and VR.holds(case.pair(proof), TAU)
    return _verdicts[key]


def false_proof(case):
    """test_gpu_verify_decide.false_proof (well formed and false, asserted from the oracle), once per proof."""
    key = (case.name, case.N, case.transcript, case.multiopen, case.proof)
    if key not in _false:
        _false[key] = make_false_proof(case)
    return _false[key]


def flags_of(plonk, case):
    return VC.kind_flags(plonk, case.transcript, case.multiopen)


def params_for(ctx, pkg, oracle, k, g=True):
    if k not in _srs:
        _srs[k] = zu.test_srs(oracle, k, TAU)
    return pkg.kzg.ParamsKZG(ctx, k, g=_srs[k][0] if g else None, g_lagrange=_srs[k][1])


# ------------------------------------------------------------------------------------ keys and files
@pytest.mark.parametrize("name", NAMES)
def test_vk_from_root_clone_and_file_key_is_the_oracles_and_its_file_reads_back(ctx, plonk, rigs, vparams, name):
    rig = rigs(name)
    want_f, want_p = list(rig.opk.fixed_commitments), list(rig.opk.permutation_commitments)
    clone = rig.pk.clone_workspace()
    loaded = plonk.ProvingKey.read(ctx, rig.params, rig.pk.write())
    vks = []
    try:
        vks = [key.get_vk() for key in (rig.pk, clone, loaded)]
    finally:
        loaded.free()
        clone.free()
    try:
        for vk in vks:
            f, p = vk.commitments()
            assert [zu.point_to_ints(x) for x in f] == want_f and [zu.point_to_ints(x) for x in p] == want_p
        for pair in (False, True):
            files = [vk.write(vparams if pair else None) for vk in vks]
            assert files[0] == files[1] == files[2] == oracle_file(plonk, rig.c.desc, rig.opk, pair=pair)
            assert len(files[0]) == ctx.L.amdzk_vk_serialized_size(vks[0].h, int(pair))
            assert plonk.vk_blob_info(files[0]) == vk_blob.shape(rig.c.desc, pair)
            back, g2, s_g2 = plonk.VerifyingKey.read(ctx, files[0])
            try:
                assert back.write(vparams if pair else None) == files[0]
                if pair:
                    assert np.array_equal(g2, G2_WORDS) and np.array_equal(s_g2, S_G2_WORDS)
                else:
                    assert g2 is None and s_g2 is None
                assert back.desc == plonk.blob_desc(rig.pk.write())
            finally:
                back.free()
    finally:
        for vk in vks:
            vk.free()


def no_permutation_circuit(plonk):
    """square_circuit without a single equality-enabled column: S = 0."""
    cs = plonk.ConstraintSystem()
    a, sq, s = cs.advice_column(), cs.advice_column(), cs.selector()
    cs.create_gate(lambda meta: [meta.query_selector(s) * (meta.query_advice(sq, 0) - meta.query_advice(a, 0) * meta.query_advice(a, 0))])
    c = circuits.Circuit(cs, 4)
    c.assembly = plonk.Assembly(c.n, 0)
    c.fixed[s.index][0] = 1
    c.advice[0][0], c.advice[1][0] = 5, 25
    return c


def zero_fixed_circuit(plonk):
    """square_circuit with a second fixed column that a gate queries and that is zero on every row: its commitment is the
    identity."""
    cs = plonk.ConstraintSystem()
    a, sq, inst, s, z = cs.advice_column(), cs.advice_column(), cs.instance_column(), cs.selector(), cs.fixed_column()
    for col in (a, sq, inst):
        cs.enable_equality(col)
    cs.create_gate(lambda meta: [meta.query_selector(s) * (meta.query_advice(sq, 0) - meta.query_advice(a, 0) * meta.query_advice(a, 0)),
                                 meta.query_fixed(z, 0) * meta.query_advice(a, 0)])
    c = circuits.Circuit(cs, 4)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    c.assembly.copy(0, 0, 1, 1)
    c.fixed[s.index][0] = 1
    c.advice[0][0], c.advice[1][0], c.advice[1][1] = 5, 25, 5
    c.instances[0] = []
    return c


@pytest.mark.parametrize("name", ["square", "lookup", "rlc", "random4", "random10", "random11", "no_permutation", "zero_fixed"])
def test_keygen_vk_from_the_mapping_and_from_sigma_gives_the_proving_keys_file(ctx, pkg, plonk, oracle, rigs, vparams, name):
    if name in NAMES:
        rig = rigs(name)
        c, opk, pk, params, own = rig.c, rig.opk, rig.pk, rig.params, None
    else:
        c = no_permutation_circuit(plonk) if name == "no_permutation" else zero_fixed_circuit(plonk)
        opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        own = params = params_for(ctx, pkg, oracle, c.k)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    if own is not None:
        pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR))
        assert (len(c.desc["permutation_columns"]) == 0) == (name == "no_permutation")
        assert (None in opk.fixed_commitments) == (name == "zero_fixed")
    made = []
    try:
        want = oracle_file(plonk, c.desc, opk, pair=True)
        made.append(pk.get_vk())
        made.append(plonk.keygen_vk(ctx, params, c.desc, fixed, mapping=c.assembly.mapping, transcript_repr=zu.fr_from_int(REPR)))
        if len(c.desc["permutation_columns"]):
            made.append(plonk.keygen_vk(ctx, params, c.desc, fixed, sigma_values=pk.export(1), transcript_repr=zu.fr_from_int(REPR)))
        else:
            made.append(plonk.keygen_vk(ctx, params, c.desc, fixed, transcript_repr=zu.fr_from_int(REPR)))  # S = 0: neither is wanted
        for vk in made:
            assert vk.write(vparams) == want
            f, p = vk.commitments()
            assert [zu.point_to_ints(x) for x in f] == list(opk.fixed_commitments) and [zu.point_to_ints(x) for x in p] == list(opk.permutation_commitments)
        assert plonk.proof_size(ctx, made[1]) == plonk.proof_size(ctx, pk) and plonk.proof_size_multi(ctx, made[1], 2, plonk.TRANSCRIPT_KECCAK256_EVM | plonk.MULTIOPEN_GWC) == \
            plonk.proof_size_multi(ctx, pk, 2, plonk.TRANSCRIPT_KECCAK256_EVM | plonk.MULTIOPEN_GWC)
    finally:
        for vk in made:
            vk.free()
        if own is not None:
            pk.free()
            own.free()


def test_keygen_vk_refusals_carry_a_message_and_leave_the_ctx_usable(ctx, pkg, plonk, oracle, rigs):
    rig = rigs("square")
    c = rig.c
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
    tr = zu.fr_from_int(REPR)
    want = oracle_file(plonk, c.desc, rig.opk)
    no_g = params_for(ctx, pkg, oracle, c.k, g=False)

    def good():
        vk = plonk.keygen_vk(ctx, rig.params, c.desc, fixed, mapping=c.assembly.mapping, transcript_repr=tr)
        try:
            return vk.write()
        finally:
            vk.free()
    try:
        for kw, params, why in ((dict(mapping=c.assembly.mapping, sigma_values=rig.pk.export(1)), rig.params, "keygen_vk: exactly one of .* both given"),
                                (dict(), rig.params, "keygen_vk: exactly one of .* neither given"),
                                (dict(mapping=c.assembly.mapping), no_g, "keygen_vk: the parameters need both bases")):
            with pytest.raises(pkg.AmdzkError, match=why) as e:
                plonk.keygen_vk(ctx, params, c.desc, fixed, transcript_repr=tr, **kw)
            assert e.value.code == -2
            assert good() == want
        # keygen's own checks, with keygen's own messages
        few = dict(c.desc, blinding_factors=(1 << c.k) - 2)
        with pytest.raises(pkg.AmdzkError, match="keygen: not enough rows"):
            plonk.keygen_vk(ctx, rig.params, few, fixed, mapping=c.assembly.mapping, transcript_repr=tr)
        with pytest.raises(pkg.AmdzkError, match="keygen: cs_degree 2 < 3"):
            plonk.keygen_vk(ctx, rig.params, dict(c.desc, cs_degree=2), fixed, mapping=c.assembly.mapping, transcript_repr=tr)
        assert good() == want
    finally:
        no_g.free()


def test_keygen_vk_refuses_the_circuits_keygens_compiler_refuses(ctx, pkg, plonk, oracle, rigs):
    """The verifier indexes by a key's queries and expression words unchecked, so a description with a bad one must never
    become a verifying key: an opcode outside 1 .. 9, a constant, a column or a challenge out of range, an unbalanced
    expression — each refused by amdzk_keygen_vk with keygen's "circuit:" prefix, as amdzk_keygen_ex refuses it — and a query
    that names a column out of range. Nothing is written to *out, and a following good call succeeds."""
    rig = rigs("square")
    c, L = rig.c, ctx.L
    fixed = np.ascontiguousarray(np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]))
    mp = np.ascontiguousarray(np.array(c.assembly.mapping, dtype=np.uint32).reshape(-1, c.n, 2))
    tr = zu.fr_from_int(REPR)
    want = oracle_file(plonk, c.desc, rig.opk)

    def keygen_vk(cc):
        h = C.c_void_p()
        rc = L.amdzk_keygen_vk(ctx.h, rig.params.h, C.byref(cc), None, fixed.ctypes.data, mp.ctypes.data, None, tr.ctypes.data, C.byref(h))
        return rc, h, L.amdzk_last_error(ctx.h).decode()

    def keygen_ex(cc):
        h = C.c_void_p()
        rc = L.amdzk_keygen_ex(ctx.h, rig.params.h, C.byref(cc), fixed.ctypes.data, mp.ctypes.data, tr.ctypes.data, 0, C.byref(h))
        return rc, h, L.amdzk_last_error(ctx.h).decode()

    def good():
        cc, keep = plonk.flatten_circuit(c.desc)
        rc, h, _ = keygen_vk(cc)
        assert rc == 0
        vk = plonk.VerifyingKey(ctx, h, c.desc)
        try:
            return vk.write()
        finally:
            vk.free()

    nwords = len(plonk.flatten_circuit(c.desc)[1]["words"])
    words = [(0, 10 << 24, "bad expression word 0a000000"), (0, (1 << 24) | 0xFFFF, "bad expression word|constant index"),
             (0, (3 << 24) | (200 << 8) | 128, "bad expression word|column 200 out of range"), (0, 9 << 24, "bad expression word"),
             (nwords - 1, 5 << 24, "malformed expression"), (nwords - 1, 0, "bad expression word 00000000")]
    import re
    for at, word, why in words:
        cc, a = plonk.flatten_circuit(c.desc)
        assert a["words"][at] != word
        a["words"][at] = word
        rc, h, msg = keygen_vk(cc)
        assert rc == -2 and not h.value and msg.startswith("circuit: ") and re.search(why, msg), (at, word, msg)
        rc, h, msg = keygen_ex(cc)  # keygen's own refusal of the same circuit
        assert rc == -2 and not h.value and msg.startswith("circuit: ") and re.search(why, msg), (at, word, msg)
        assert good() == want
    cc, a = plonk.flatten_circuit(c.desc)
    a["aq"][0, 0] = c.desc["num_advice"]  # one past the last advice column
    rc, h, msg = keygen_vk(cc)
    assert rc == -2 and not h.value and msg == "circuit: query 0 names a column out of range", msg
    assert good() == want


# ------------------------------------------------------------------------------------ verifying after the pk and the SRS are gone
def named_batches(cases):
    """cases: seeds 20, 21, 22 of one kind -> {name: [(case, proof)]}: the mixed batch of test_gpu_verify_decide.py, and batches
    of 1, 16, 17 and 33 proofs with one false proof at each boundary of a run of AMDZK_DECIDE_RUN = 16."""
    a, b = cases[0], cases[1]
    out = {"mixed": [(a, a.proof), (a, false_proof(a)), (a, put(a.proof, 32, bytes(32))), (b, b.proof), (b, false_proof(b))]}
    for n in (1, 16, 17, 33):
        for at in (0, 15, 16, 31, 32):
            if at < n and (at > 0 or n <= 16):
                out["n%d_false_at_%d" % (n, at)] = [(cases[i % 3], false_proof(cases[i % 3]) if i == at else cases[i % 3].proof) for i in range(n)]
    return out


class Freed:
    """What is left of a Rig once its proving key, its clones and its SRS are freed: the verifying key made before that,
    the proofs, and what the pk-taking calls said about them."""

    def __init__(self, ctx, pkg, plonk, oracle, vparams, name, N):
        rig = Rig(ctx, pkg, plonk, oracle, name, N)
        try:
            self.plonk, self.ctx, self.name, self.N, self.inst = plonk, ctx, name, N, rig.instances_arg()
            self.vk = rig.pk.get_vk()
            self.cases, self.pk_guard, self.pk_decided, self.batches, self.pk_batches = {}, {}, {}, {}, {}
            for n_, N_, tr, mo in VC.CASE_IDS:
                if (n_, N_) != (name, N):
                    continue
                case = self.cases[(tr, mo)] = rig.case(tr, mo)
                self.pk_guard[(tr, mo)] = rig.verify(case, [case.proof])
                self.pk_decided[(tr, mo)] = plonk.decide_proofs(ctx, rig.pk, vparams, [self.inst], [case.proof], transcript=flags_of(plonk, case), n_circuits=N)
                if N == 1 and (name, tr, mo) in BATCH_KINDS:
                    self.batches = named_batches([rig.case(tr, mo, seed=20 + i) for i in range(3)])
                    for bname, batch in self.batches.items():
                        proofs = [p for _, p in batch]
                        self.pk_batches[bname] = (self.decide(rig.pk, vparams, case, proofs), self.decide(rig.pk, vparams, case, proofs, combined=True, combine_seed=0xC0FFEE),
                                                  rig.verify(case, proofs, combine_seed=77))
                if N == 2 and (tr, mo) == ("blake2b", "shplonk"):
                    self.two = [case.proof, false_proof(case)]
                    self.pk_two = self.decide(rig.pk, vparams, case, self.two)
        finally:
            rig.free()

    def decide(self, key, vparams, case, proofs, **kw):
        return self.plonk.decide_proofs(self.ctx, key, vparams, [self.inst] * len(proofs), proofs, transcript=flags_of(self.plonk, case), n_circuits=self.N, **kw)

    def verify(self, case, proofs, **kw):
        return self.plonk.verify_proofs(self.ctx, self.vk, [self.inst] * len(proofs), proofs, transcript=flags_of(self.plonk, case), n_circuits=self.N, **kw)


@pytest.fixture(scope="module")
def freed(ctx, pkg, plonk, oracle, vparams):
    made = {}

    def get(name, N=1):
        if (name, N) not in made:
            made[(name, N)] = Freed(ctx, pkg, plonk, oracle, vparams, name, N)
        return made[(name, N)]
    yield get
    for f in made.values():
        f.vk.free()


def same_guard(a, b):
    return np.array_equal(a.lhs, b.lhs) and np.array_equal(a.rhs, b.rhs) and a.statuses == b.statuses


@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_every_case_verifies_the_same_without_the_proving_key_and_the_srs(plonk, freed, vparams, name, N, transcript, multiopen):
    fr = freed(name, N)
    case = fr.cases[(transcript, multiopen)]
    assert oracle_verdict(case, case.proof) is True
    g = fr.verify(case, [case.proof])
    assert same_guard(g, fr.pk_guard[(transcript, multiopen)]) and g.well_formed and g.lhs.any() and g.rhs.any()
    got = fr.decide(fr.vk, vparams, case, [case.proof])
    assert got == fr.pk_decided[(transcript, multiopen)] == ([True], [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)])
    assert plonk.decide_proof(fr.ctx, fr.vk, vparams, fr.inst, case.proof, transcript=flags_of(plonk, case), n_circuits=N) is True
    assert same_guard(plonk.verify_proof(fr.ctx, fr.vk, fr.inst, case.proof, transcript=flags_of(plonk, case), n_circuits=N), g)
    assert plonk.proof_size_multi(fr.ctx, fr.vk, N, flags_of(plonk, case)) == len(case.proof)


@pytest.mark.parametrize("name,transcript,multiopen", BATCH_KINDS)
def test_batches_get_the_oracles_and_the_pk_routes_verdicts(plonk, freed, vparams, name, transcript, multiopen):
    fr = freed(name)
    case = fr.cases[(transcript, multiopen)]
    assert sorted(fr.batches) == sorted(["mixed", "n1_false_at_0", "n16_false_at_0", "n16_false_at_15", "n17_false_at_15", "n17_false_at_16",
                                         "n33_false_at_15", "n33_false_at_16", "n33_false_at_31", "n33_false_at_32"])
    for bname, batch in fr.batches.items():
        proofs = [p for _, p in batch]
        want = [oracle_verdict(c, p) for c, p in batch]
        if bname == "mixed":
            assert want == [True, False, False, True, False] and batch[2][0].decode(proofs[2])[0] == plonk.PROOF_BAD_POINT
        else:
            at = int(bname.rsplit("_", 1)[1])
            assert want == [b != at for b in range(len(batch))]
        per_proof, combined, guard = fr.pk_batches[bname]
        verdicts, statuses = fr.decide(fr.vk, vparams, case, proofs)
        assert verdicts == want and (verdicts, statuses) == per_proof, bname
        assert [tuple(s) for s in statuses] == [c.decode(p) for c, p in batch], bname
        got = fr.decide(fr.vk, vparams, case, proofs, combined=True, combine_seed=0xC0FFEE)
        assert got == combined and got[0] == [False] * len(batch), bname  # every batch holds a false proof
        assert same_guard(fr.verify(case, proofs, combine_seed=77), guard), bname


def test_a_two_instance_proof(plonk, freed, vparams):
    fr = freed("lookup", 2)
    case = fr.cases[("blake2b", "shplonk")]
    want = [oracle_verdict(case, p) for p in fr.two]
    assert want == [True, False]
    assert fr.decide(fr.vk, vparams, case, fr.two) == fr.pk_two and fr.pk_two[0] == want


def test_a_wrong_key_decides_a_valid_proof_false_and_well_formed(ctx, pkg, plonk, oracle, rigs, freed, vparams):
    """A key of another circuit with the same proof length and instance columns, if the cases hold such a pair whose layouts
    the reference decode takes for well formed; else a key whose transcript_repr differs. The expectation is the oracle's."""
    kind = ("blake2b", "shplonk")
    names = [n for n, N, kinds in VC.CASES if N == 1 and kind in kinds]
    keys = {n: freed(n) for n in names}
    found = None
    for a in names:
        for b in names:
            ca, cb = keys[a].cases[kind], keys[b].cases[kind]
            if a != b and found is None and len(ca.proof) == len(cb.proof) and ca.desc["num_instance"] == cb.desc["num_instance"] and ca.challenges is None and \
                    cb.challenges is None:
                as_b = VC.Case(b, cb.c, cb.desc, cb.opk, ca.instances_list, ca.proof, *kind, None)
                if as_b.decode() == (0, 0):
                    found = (keys[a], keys[b].vk, as_b)
    if found is not None:
        fr, wrong, as_wrong = found
        assert not VR.holds(as_wrong.pair(), TAU)
        assert fr.decide(wrong, vparams, as_wrong, [as_wrong.proof]) == ([False], [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)])
        return
    rig = rigs("square")
    case = rig.case(*kind)
    opk2 = PR.keygen(rig.c.desc, rig.c.fixed, rig.c.assembly.mapping, TAU, transcript_repr=REPR + 1)
    as_wrong = VC.Case("square", rig.c, rig.c.desc, opk2, case.instances_list, case.proof, *kind, None)
    assert oracle_verdict(case, case.proof) and as_wrong.decode() == (0, 0) and not VR.holds(as_wrong.pair(), TAU)
    fixed = np.stack([zu.ints_to_fr(oracle, col) for col in rig.c.fixed])
    wrong = plonk.keygen_vk(ctx, rig.params, rig.c.desc, fixed, mapping=rig.c.assembly.mapping, transcript_repr=zu.fr_from_int(REPR + 1))
    try:
        assert wrong.write() == oracle_file(plonk, rig.c.desc, opk2, repr_=REPR + 1)
        got = plonk.decide_proofs(ctx, wrong, vparams, [rig.inst], [case.proof])
        assert got == ([False], [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)])
        g = plonk.verify_proof(ctx, wrong, rig.inst, case.proof)
        assert (zu.point_to_ints(g.lhs), zu.point_to_ints(g.rhs)) == as_wrong.pair()
    finally:
        wrong.free()


VERIFIER = """\
import ctypes as C, sys, numpy as np
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as ge
pkg, d = ge.load_package(), sys.argv[2]
with pkg.Context(0) as ctx:
    L, blob, cols = ctx.L, open(d + "/key.vk", "rb").read(), np.load(d + "/instances.npz")
    vk, g2, s_g2, q = C.c_void_p(), np.zeros(16, np.uint64), np.zeros(16, np.uint64), [C.c_void_p(), C.c_void_p()]
    ctx._chk(L.amdzk_vk_read(ctx.h, blob, len(blob), C.byref(vk), g2.ctypes.data, s_g2.ctypes.data, None))
    for h, w in zip(q, (g2, s_g2)):
        ctx._chk(L.amdzk_g2_prepare(ctx.h, w.ctypes.data, C.byref(h)))
    proofs = [open("%s/proof%d.bin" % (d, i), "rb").read() for i in range(3)]
    ipp, lpp, pp, pl, opts, st, keep = pkg.plonk._verify_args([[cols[k] for k in sorted(cols.files)]] * 3, proofs, 0, 1, 0, None, None)
    v = np.zeros(3, np.uint8)
    ctx._chk(L.amdzk_verify_proofs_decide_vk(ctx.h, vk, q[1], q[0], 0, 3, ipp, lpp, pp, pl, C.byref(opts), st, v.ctypes.data, None))
    print([int(x) for x in v])
"""


def test_a_fresh_process_decides_three_proofs_from_a_file(plonk, freed, vparams, tmp_path):
    """A child process that makes a ctx and calls amdzk_vk_read, amdzk_g2_prepare twice and amdzk_verify_proofs_decide_vk —
    no amdzk_srs_* and no amdzk_pk_* function: the script above is all it runs."""
    assert "amdzk_srs" not in VERIFIER and "amdzk_pk" not in VERIFIER and "keygen" not in VERIFIER
    fr = freed("lookup")
    case = fr.cases[("blake2b", "shplonk")]
    proofs = [case.proof, false_proof(case), case.proof]
    assert [oracle_verdict(case, p) for p in proofs] == [True, False, True] and any(len(col) for col in fr.inst)
    with open(tmp_path / "key.vk", "wb") as f:
        f.write(fr.vk.write(vparams))
    np.savez(tmp_path / "instances.npz", **{"col%03d" % i: col for i, col in enumerate(fr.inst)})
    for i, p in enumerate([proofs[0], proofs[2], proofs[1]]):  # two valid proofs, then the false one
        with open(tmp_path / ("proof%d.bin" % i), "wb") as f:
            f.write(p)
    with open(tmp_path / "verifier.py", "w") as f:
        f.write(VERIFIER)
    out = subprocess.run([sys.executable, str(tmp_path / "verifier.py"), ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1] == "[1, 1, 0]"


def test_refusals_of_the_two_verify_calls_carry_their_prefixes_and_leave_the_ctx_usable(ctx, pkg, plonk, freed, vparams):
    fr = freed("square")
    case = fr.cases[("blake2b", "shplonk")]
    L = ctx.L
    inst_pp, lens_pp, pp, pl, opts, st, keep = plonk._verify_args([fr.inst], [case.proof], 0, 1, 0, None, None)
    VO = pkg.ffi.VerifyOpts
    small = VO(C.sizeof(VO) - 1, 0, 1, 0, None)
    pair, verdicts, n_valid = np.zeros(16, np.uint64), np.zeros(1, np.uint8), C.c_size_t(0)
    want = fr.pk_guard[("blake2b", "shplonk")]

    def verify(vk=fr.vk.h, n=1, o=opts):
        return L.amdzk_verify_proofs_vk(ctx.h, vk, n, inst_pp, lens_pp, pp, pl, C.byref(o), st, pair.ctypes.data)

    def decide(vk=fr.vk.h, n=1, o=opts, s_g2=vparams.s_g2.h):
        return L.amdzk_verify_proofs_decide_vk(ctx.h, vk, s_g2, vparams.g2.h, 0, n, inst_pp, lens_pp, pp, pl, C.byref(o), st, verdicts.ctypes.data, C.byref(n_valid))

    for kw in (dict(vk=None), dict(n=0), dict(o=small)):
        assert verify(**kw) == -2, kw
        assert L.amdzk_last_error(ctx.h).decode().startswith("verify_proofs:"), (kw, L.amdzk_last_error(ctx.h))
        assert verify() == 0 and np.array_equal(pair[:8], want.lhs) and np.array_equal(pair[8:], want.rhs) and (st[0].status, st[0].offset) == (0, 0)
    for kw in (dict(vk=None), dict(n=0), dict(o=small), dict(s_g2=None)):
        assert decide(**kw) == -2, kw
        assert L.amdzk_last_error(ctx.h).decode().startswith("verify_proofs_decide:"), (kw, L.amdzk_last_error(ctx.h))
        assert decide() == 0 and verdicts[0] == 1 and n_valid.value == 1
    with pytest.raises(pkg.ffi.AmdzkError, match="verify_proofs:"):
        plonk.verify_proofs(ctx, fr.vk, [fr.inst], [case.proof], opts_size=8)
    with pytest.raises(pkg.ffi.AmdzkError, match="verify_proofs_decide:"):
        plonk.decide_proofs(ctx, fr.vk, vparams, [fr.inst], [case.proof], opts_size=8)
