"""GPU: keygen, proving, verifying and witness checking at the extreme circuit SHAPES of tests/shape_circuits.py — no advice
column, no fixed column, no gate, n = 8 with 2 usable rows, ten permutation sets of one column, eight lookups, a lookup six
pairs wide, rotations of n - 1 and n + 1, unqueried columns, witness tables beside a constant one: the counts that are 0 or 1
where every other fixture has a few.

Everything is compared exactly — commitments, key files, proof bytes, the verifier's pair, statuses, verdicts, failure
tuples — with the CPU side: the pure-Python oracle (oracle/plonk_ref.py; tests/test_shape_circuits.py holds the C++-backed
prover to the same bytes), tests/verify_ref.py, tests/witness_check_ref.py and the independent file encoders. There is no
tolerance anywhere. One SRS per k, made on the device; one key per shape, shared by the module's tests."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pk_blob  # noqa: E402
import plonk_ref as PR  # noqa: E402
import shape_circuits as S  # noqa: E402
import verify_ref as VR  # noqa: E402
import witness_check_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, REPR, SEED, R = S.TAU, S.REPR, S.SEED, zu.R
EMPTY_SECTIONS = {"perm_only-k3": "F", "perm_only-k4": "F", "perm_ten_sets": "F", "lookup_only-k3": "S", "lookup_only-k4": "S", "no_advice": "S"}
INVALID = -2  # AMDZK_E_INVALID


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


@pytest.fixture(scope="module")
def srs(ctx, pkg):
    """k -> ParamsKZG made on the device (amdzk_srs_setup), shared by the module's tests."""
    made = {}

    def get(k):
        if k not in made:
            made[k] = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(TAU))
        return made[k]
    yield get
    for p in made.values():
        p.free()


@pytest.fixture(scope="module")
def vparams(ctx, pkg):
    v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
    yield v
    v.free()


def fr_cols(oracle, cols, n):
    return np.stack([zu.ints_to_fr(oracle, col) for col in cols]) if cols else np.zeros((0, n, 4), np.uint64)


def fr_inst(oracle, instances):
    return [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in instances]


def flags_of(plonk, transcript, multiopen):
    return (plonk.TRANSCRIPT_BLAKE2B if transcript == "blake2b" else plonk.TRANSCRIPT_KECCAK256_EVM) | (plonk.MULTIOPEN_GWC if multiopen == "gwc" else 0)


class Rig:
    """One shape on the device: its key and its own witness. A shape without an advice column has no advice buffer at all:
    every call gets d_advice = NULL."""

    def __init__(self, ctx, plonk, oracle, srs, name):
        self.ctx, self.plonk, self.oracle, self.name = ctx, plonk, oracle, name
        self.c = c = S.shape(plonk, name)
        self.opk = S.oracle_key(plonk, name)
        self.params = srs(c.k)
        self.fixed = fr_cols(oracle, c.fixed, c.n)
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, self.fixed, c.assembly.mapping, zu.fr_from_int(REPR))
        self.inst = fr_inst(oracle, c.instances)
        self.d_adv = self.device_advice(c.advice)

    def device_advice(self, advice):
        if not advice:
            return None
        arr = fr_cols(self.oracle, advice, self.c.n)
        return self.ctx.alloc(arr.nbytes).upload(arr)

    def prove(self, transcript, multiopen, pk=None, seed=SEED):
        return self.plonk.create_proof(self.ctx, pk or self.pk, self.inst, self.d_adv, seed=seed, transcript=flags_of(self.plonk, transcript, multiopen))

    def report(self, advice=None, instances=None):
        d = self.d_adv if advice is None else self.device_advice(advice)
        try:
            rep = self.plonk.check_witness(self.ctx, self.pk, self.inst if instances is None else fr_inst(self.oracle, instances), d)
        finally:
            if d is not None and d is not self.d_adv:
                d.free()
        assert rep.ok == (not rep.failures)
        return [tuple(f) for f in rep.failures]

    def free(self):
        if self.d_adv is not None:
            self.d_adv.free()
        self.pk.free()


@pytest.fixture(scope="module")
def rigs(ctx, plonk, oracle, srs):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Rig(ctx, plonk, oracle, srs, name)
        return made[name]
    yield get
    for r in made.values():
        r.free()


def ints(guard):
    return zu.point_to_ints(guard.lhs), zu.point_to_ints(guard.rhs)


# ------------------------------------------------------------------------------------ key
@pytest.mark.parametrize("name", S.NAMES)
def test_key_commitments_and_file_are_the_oracles(ctx, plonk, oracle, rigs, name):
    """ProvingKey(...) succeeds; its commitments are the oracle key's — empty lists where F or S is 0 — and its file is the
    independent encoder's, byte for byte, with zero-length sections where a count is 0; the host-only checks accept the file
    and report the shape's counts."""
    rig = rigs(name)
    c, opk = rig.c, rig.opk
    f, p = rig.pk.commitments()
    assert f.shape == (c.desc["num_fixed"], 8) and p.shape == (len(c.desc["permutation_columns"]), 8)
    assert [zu.point_to_ints(x) for x in f] == opk.fixed_commitments and [zu.point_to_ints(x) for x in p] == opk.permutation_commitments
    blob = rig.pk.write()
    assert len(blob) == ctx.L.amdzk_pk_serialized_size(rig.pk.h)
    assert blob == pk_blob.encode(plonk, oracle, c.desc, opk, REPR)
    F, Sn = c.desc["num_fixed"], len(c.desc["permutation_columns"])
    assert len(blob) == len(pk_blob.header(plonk, c.desc)) + 32 + (F + Sn) * (64 + 32 * c.n) + 64
    if name in EMPTY_SECTIONS:
        assert {"F": F, "S": Sn}[EMPTY_SECTIONS[name]] == 0
    buf = np.frombuffer(blob, dtype=np.uint8)
    msg = C.create_string_buffer(256)
    assert ctx.L.amdzk_pk_blob_check(buf.ctypes.data, buf.size, msg, len(msg)) == 0, msg.value
    assert plonk.blob_info(blob) == dict(k=c.k, num_fixed=F, num_advice=c.desc["num_advice"], num_perm_columns=Sn, num_challenges=0)
    for what, want in enumerate((c.fixed, opk.permutations, opk.fixed_polys, opk.permutation_polys)):
        got = rig.pk.export(what)
        assert got.shape == (len(want), c.n, 4) and np.array_equal(got, fr_cols(oracle, want, c.n)), "export(%d)" % what


# ------------------------------------------------------------------------------------ proof
@pytest.mark.parametrize("name", S.NAMES)
def test_proof_bytes_are_the_oracles(ctx, plonk, rigs, name):
    rig = rigs(name)
    for tr, mo in S.KINDS:
        want = S.oracle_proof(plonk, name, tr, mo)
        got = rig.prove(tr, mo)
        assert got == want, (tr, mo)
        assert plonk.proof_size(ctx, rig.pk, flags_of(plonk, tr, mo)) == len(got)
        assert rig.prove(tr, mo) == want  # the workspace is clean afterwards


@pytest.mark.parametrize("name", S.NAMES)
def test_keys_of_every_origin_prove_the_same_bytes(ctx, plonk, rigs, name):
    """A key read back from its file, a key made from the exported sigma columns (none where S = 0) and a workspace clone."""
    rig = rigs(name)
    c = rig.c
    blob = rig.pk.write()
    keys = {"read": plonk.ProvingKey.read(ctx, rig.params, blob),
            "sigma": plonk.ProvingKey.from_sigma(ctx, rig.params, c.desc, rig.fixed, rig.pk.export(1), zu.fr_from_int(REPR)),
            "clone": rig.pk.clone_workspace()}
    try:
        for origin, key in keys.items():
            assert key.write() == blob, origin
            for tr, mo in S.KINDS:
                assert rig.prove(tr, mo, pk=key) == S.oracle_proof(plonk, name, tr, mo), (origin, tr, mo)
    finally:
        for key in keys.values():
            key.free()


# ------------------------------------------------------------------------------------ verify
def oracle_verdict(c, opk, instances, proof, tr, mo):
    """(status, verdict, pair or None) from the CPU side alone: the reference decode, then tau * L == R for the reference pair."""
    status = VR.decode(c.desc, 1, [instances], proof, transcript=tr, multiopen=mo)
    if status != (VR.WELL_FORMED, 0):
        return status, False, None
    pair = VR.pair(opk, [instances], proof, transcript=tr, multiopen=mo)
    return status, VR.holds(pair, TAU), pair


@pytest.mark.parametrize("name", S.NAMES)
def test_verify_and_decide_with_every_key(ctx, plonk, oracle, rigs, vparams, name):
    """The device's own proofs of both kinds: WELL_FORMED and the reference pair from the proving key, from vk_from_pk,
    from keygen_vk and from a verifying key read back from its file; decided true. The proof with its last byte flipped and
    the proof under a wrong instance value get the reference's status and the verdict false, and nothing else is refused.
    The two kinds in one mixed batch give the same statuses and verdicts."""
    rig = rigs(name)
    c, opk = rig.c, rig.opk
    S_ = len(c.desc["permutation_columns"])
    vks = [rig.pk.get_vk(),
           plonk.keygen_vk(ctx, rig.params, c.desc, rig.fixed, mapping=c.assembly.mapping if S_ else None, transcript_repr=zu.fr_from_int(REPR))]
    try:
        file = vks[0].write(vparams)
        assert vks[1].write(vparams) == file
        back, g2, s_g2 = plonk.VerifyingKey.read(ctx, file)
        vks.append(back)
        assert g2 is not None and back.write(vparams) == file
        keys = [rig.pk] + vks
        bad_inst = S.wrong_instances(c)
        members = []  # (key, instances words, proof, flags, expected status, expected verdict) of the mixed batch
        for tr, mo in S.KINDS:
            flags = flags_of(plonk, tr, mo)
            proof = rig.prove(tr, mo)
            status, verdict, pair = oracle_verdict(c, opk, c.instances, proof, tr, mo)
            assert status == (0, 0) and verdict and pair[0] is not None and pair[1] is not None
            for key in keys:
                assert plonk.proof_size(ctx, key, flags) == len(proof)
                g = plonk.verify_proofs(ctx, key, [rig.inst], [proof], transcript=flags)
                assert g.statuses == [plonk.ProofStatus(plonk.PROOF_WELL_FORMED, 0)] and ints(g) == pair
                assert plonk.decide_proofs(ctx, key, vparams, [rig.inst], [proof], transcript=flags) == ([True], [plonk.ProofStatus(0, 0)])
            members.append((vks[0], rig.inst, proof, flags, (0, 0), True))
            # one byte of the proof, one public input: the reference's status, the verdict false, no other refusal
            cases = [(c.instances, S.flipped(proof))] + ([(bad_inst, proof)] if bad_inst is not None else [])
            for instances, bytes_ in cases:
                status, verdict, pair = oracle_verdict(c, opk, instances, bytes_, tr, mo)
                assert not verdict
                words = fr_inst(oracle, instances)
                for key in (rig.pk, vks[-1]):
                    g = plonk.verify_proofs(ctx, key, [words], [bytes_], transcript=flags)
                    assert [tuple(s) for s in g.statuses] == [status]
                    if pair is not None:
                        assert ints(g) == pair
                    verdicts, statuses = plonk.decide_proofs(ctx, key, vparams, [words], [bytes_], transcript=flags)
                    assert verdicts == [False] and [tuple(s) for s in statuses] == [status]
                members.append((vks[1], words, bytes_, flags, status, False))
        # a good proof decides true right after the false ones, and the whole lot in one mixed call
        items = [plonk.VerifyItem(key, words, proof, transcript=flags) for key, words, proof, flags, _, _ in members]
        verdicts, statuses = plonk.decide_proofs_mixed(ctx, vparams, items)
        assert verdicts == [m[5] for m in members] and [tuple(s) for s in statuses] == [m[4] for m in members]
        both = [plonk.VerifyItem(rig.pk, rig.inst, rig.prove(tr, mo), transcript=flags_of(plonk, tr, mo)) for tr, mo in S.KINDS]
        rho = [3, R - 2]
        g = plonk.verify_proofs_mixed(ctx, both, combine_scalars=np.stack([zu.fr_from_int(v) for v in rho]))
        pairs = [VR.pair(opk, [c.instances], it.proof, transcript=tr, multiopen=mo) for it, (tr, mo) in zip(both, S.KINDS)]
        assert g.well_formed and ints(g) == VR.combine(pairs, rho)
        assert plonk.decide_proofs_mixed(ctx, vparams, both, combined=True, combine_seed=77)[0] == [True, True]
    finally:
        for vk in vks:
            vk.free()


# ------------------------------------------------------------------------------------ check
@pytest.mark.parametrize("name", S.NAMES)
def test_check_witness_reports_the_references_tuples(plonk, rigs, name):
    """Nothing for the witness; for each constraint kind the shape has, one corrupted cell — a gate input, a lookup input, one
    end of a copy — gives exactly the reference's tuples, and the good witness is accepted again afterwards."""
    rig = rigs(name)
    c = rig.c
    assert (rig.d_adv is None) == (name == "no_advice")
    assert rig.report() == [] == W.report(c)
    for way in sorted(S.SHAPES[name][1]):
        adv, inst, want = S.corrupt(c, way)
        assert any(e[0] == S.KIND[way] for e in want)
        assert rig.report(advice=adv, instances=inst) == want, way
        assert rig.report() == []


# ------------------------------------------------------------------------------------ batch and instances
@pytest.mark.parametrize("name", ["perm_ten_sets", "unused_columns"])
def test_batches_and_two_instances_under_gwc(ctx, plonk, oracle, rigs, vparams, name):
    """create_proof_batch of three witnesses under (blake2b, gwc) equals three single proofs and the oracle's; one proof of
    N = 2 circuit instances through create_proof_multi under GWC, for both transcripts, equals the oracle's, gives the
    reference pair and is decided true."""
    rig = rigs(name)
    c, opk = rig.c, rig.opk
    wit = [(c.advice, c.instances)] + [c.witness(j) for j in (1, 2)]
    pks = [rig.pk, rig.pk.clone_workspace(), rig.pk.clone_workspace()]
    d_adv = [rig.device_advice(a) for a, _ in wit]
    inst = [fr_inst(oracle, i) for _, i in wit]
    try:
        flags = flags_of(plonk, "blake2b", "gwc")
        seeds = [SEED, SEED + 1, SEED + 2]
        singles = [plonk.create_proof(ctx, rig.pk, inst[b], d_adv[b], seed=seeds[b], transcript=flags) for b in range(3)]
        want = [PR.create_proof(opk, wit[b][1], wit[b][0], seed=seeds[b], multiopen="gwc") for b in range(3)]
        assert singles == want
        assert plonk.create_proof_batch(ctx, pks, inst, d_adv, seeds, transcript=flags) == singles
        for tr in ("blake2b", "evm"):
            flags = flags_of(plonk, tr, "gwc")
            want = PR.create_proof_multi(opk, [i for _, i in wit[:2]], [a for a, _ in wit[:2]], seed=SEED, transcript=tr, multiopen="gwc")
            got = plonk.create_proof_multi(ctx, pks[:2], inst[:2], d_adv[:2], seed=SEED, transcript=flags)
            assert got == want, tr
            assert plonk.proof_size_multi(ctx, rig.pk, 2, flags) == len(got)
            assert PR.verify_proof_multi(opk, [i for _, i in wit[:2]], got, transcript=tr, multiopen="gwc")
            pair = VR.pair(opk, [i for _, i in wit[:2]], got, transcript=tr, multiopen="gwc")
            g = plonk.verify_proofs(ctx, rig.pk, [inst[:2]], [got], transcript=flags, n_circuits=2)
            assert g.well_formed and ints(g) == pair and VR.holds(pair, TAU)
            assert plonk.decide_proofs(ctx, rig.pk, vparams, [inst[:2]], [got], transcript=flags, n_circuits=2)[0] == [True]
            assert plonk.decide_proofs(ctx, rig.pk, vparams, [inst[:2][::-1]], [got], transcript=flags, n_circuits=2)[0] == [False]
    finally:
        for d in d_adv:
            d.free()
        for pk in pks[1:]:
            pk.free()


def test_a_batch_without_an_advice_column(ctx, plonk, rigs):
    """create_proof_batch with d_advice[b] = NULL for a key that has no advice column: two seeds, the oracle's bytes."""
    rig = rigs("no_advice")
    clone = rig.pk.clone_workspace()
    try:
        flags = flags_of(plonk, "blake2b", "gwc")
        want = [PR.create_proof(rig.opk, rig.c.instances, rig.c.advice, seed=s, multiopen="gwc") for s in (SEED, SEED + 1)]
        assert plonk.create_proof_batch(ctx, [rig.pk, clone], [rig.inst, rig.inst], [None, None], [SEED, SEED + 1], transcript=flags) == want
        assert [plonk.create_proof(ctx, rig.pk, rig.inst, None, seed=s, transcript=flags) for s in (SEED, SEED + 1)] == want
    finally:
        clone.free()


# ------------------------------------------------------------------------------------ refusals
def proves_square_min_rows(plonk, rigs):
    rig = rigs("square_min_rows")
    return all(rig.prove(tr, mo) == S.oracle_proof(plonk, "square_min_rows", tr, mo) for tr, mo in S.KINDS)


def test_nothing_constrained_is_refused_for_its_identity_commitment(ctx, pkg, plonk, oracle, srs, rigs):
    """h(X) is zero, a piece of it commits to the identity: the refusal a random circuit with a zero piece gets
    (tests/test_random_circuits.py, seed (6, 23)) — the same code, the same message. Keygen, the witness check and the key
    file are not affected. The context proves the smallest shape to the oracle's bytes afterwards."""
    c = S.shape(plonk, "nothing_constrained")
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    with pytest.raises(AssertionError, match="cannot write points at infinity"):
        PR.create_proof(opk, c.instances, c.advice, seed=SEED)
    pk = plonk.ProvingKey(ctx, srs(c.k), c.desc, fr_cols(oracle, c.fixed, c.n), c.assembly.mapping, zu.fr_from_int(REPR))
    adv = fr_cols(oracle, c.advice, c.n)
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    try:
        assert pk.write() == pk_blob.encode(plonk, oracle, c.desc, opk, REPR)
        assert plonk.check_witness(ctx, pk, [], d_adv).ok
        for flags in (0, plonk.TRANSCRIPT_KECCAK256_EVM | plonk.MULTIOPEN_GWC):
            with pytest.raises(pkg.AmdzkError, match=r"^amdzk error -2: create_proof: h_piece commitment is the identity \(cannot write points at infinity to the transcript\)$") as e:
                plonk.create_proof(ctx, pk, [], d_adv, seed=SEED, transcript=flags)
            assert e.value.code == INVALID
            assert proves_square_min_rows(plonk, rigs)
    finally:
        d_adv.free()
        pk.free()


def test_too_few_rows_is_refused_at_keygen(ctx, pkg, plonk, oracle, srs, rigs):
    """n = 4 with five blinding factors: no usable row. Keygen refuses before it makes anything, from the mapping, from
    sigma columns and for a verifying key alone; the context proves the smallest shape afterwards."""
    c = S.shape(plonk, "too_few_rows")
    with pytest.raises(AssertionError, match="not enough rows"):
        PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    fixed, tr = fr_cols(oracle, c.fixed, c.n), zu.fr_from_int(REPR)
    sigma = np.zeros((2, c.n, 4), np.uint64)
    makers = (lambda: plonk.ProvingKey(ctx, srs(c.k), c.desc, fixed, c.assembly.mapping, tr),
              lambda: plonk.ProvingKey.from_sigma(ctx, srs(c.k), c.desc, fixed, sigma, tr),
              lambda: plonk.keygen_vk(ctx, srs(c.k), c.desc, fixed, mapping=c.assembly.mapping, transcript_repr=tr))
    for make in makers:
        with pytest.raises(pkg.AmdzkError, match=r"^amdzk error -2: keygen: not enough rows \(n = 4, blinding factors = 5\)$") as e:
            make()
        assert e.value.code == INVALID
        assert proves_square_min_rows(plonk, rigs)
