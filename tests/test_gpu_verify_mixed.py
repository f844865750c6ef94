"""GPU: amdzk_verify_proofs_mixed / amdzk_verify_proofs_decide_mixed — proofs of DIFFERENT circuits under different keys in one
call. The yardstick is the single-key calls: a batch over one key must give their words; a mixed batch must give, item by item,
the status, offset and verdict the single-key call gives that proof under that key, and a pair that equals — as a group
element, in Python integers — the sum of the pairs the single-key calls return for each key's members with the same weights.
Verdicts are also held against the oracle's verifier. Keys are proving keys and verifying keys (one read from a key file after
its SRS and proving key are gone), at k = 4, 5 and 6, two of them over one setup and its downsize; Blake2b/SHPLONK and EVM/GWC
sit in one batch; some items come through the caller's read transcript. Element counts of 63, 64 and 65 (computed and asserted)
sit on the edges of the decode launch's block -> item table. All comparisons are exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402
from test_gpu_verify import Rig, ints, nonresidue_x, positions, put  # noqa: E402
from test_gpu_verify_read import _Refuse, bump_scalar, reader_of  # noqa: E402

pytestmark = pytest.mark.gpu
TAU, REPR, Q, R = VC.TAU, VC.REPR, zu.Q, zu.R
OTHER_TAU = TAU + 1
WELL, BAD_LENGTH, BAD_POINT, BAD_SCALAR, BAD_INSTANCE, BAD_TRANSCRIPT = 0, 1, 2, 3, 4, 5
B2, EVM = ("blake2b", "shplonk"), ("evm", "gwc")


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def padded_circuit(plonk, extra_adv, extra_fix, k=4):
    """A SquareCircuit-like gate with extra_adv more advice columns queried at rotation 0 (one point and one scalar each) and
    extra_fix more queried fixed columns (one scalar each): the proof's element count in steps of one."""
    cs = plonk.ConstraintSystem()
    a, sq = cs.advice_column(), cs.advice_column()
    xs = [cs.advice_column() for _ in range(extra_adv)]
    sel = cs.selector()
    fs = [cs.fixed_column() for _ in range(extra_fix)]
    cs.enable_equality(a)

    def gate(m):
        s = m.query_selector(sel)
        return ([s * (m.query_advice(sq, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))] + [s * m.query_advice(x, 0) for x in xs] +
                [s * m.query_fixed(f, 0) for f in fs])

    cs.create_gate(gate)
    c = circuits.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    c.fixed[sel.index][0] = 1
    c.advice[a.index][0], c.advice[sq.index][0] = 7, 49
    c.instances = []
    circuits.check_satisfied(c)
    return c


def count_elements(c):
    return len(VR.element_kinds(c.desc, 1, "shplonk"))


def padded_to(plonk, target):
    """The padded circuit whose Blake2b/SHPLONK proof has `target` elements."""
    need = target - count_elements(padded_circuit(plonk, 0, 0))
    assert need >= 0
    c = padded_circuit(plonk, need // 2, need % 2)
    assert count_elements(c) == target
    return c


class Own(Rig):
    """A Rig over a circuit and params of the test's own (the params stay the caller's)."""

    def __init__(self, ctx, pkg, plonk, oracle, name, c, params):
        if name not in VC._keys:  # the oracle's key, made once per process like verify_cases' own
            VC._keys[name] = (c, PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR))
        self.ctx, self.plonk, self.name, self.N = ctx, plonk, name, 1
        self.c, self.opk = VC._keys[name]
        self.phased, self.proofs, self.params = False, {}, params
        c = self.c
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed])
        self.pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR))
        self.pks = [self.pk]
        adv = np.stack([zu.ints_to_fr(oracle, col) for col in c.advice])
        self.d_adv = [ctx.alloc(adv.nbytes).upload(adv)]
        self.inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]

    def free(self):
        for d in self.d_adv:
            d.free()
        self.pk.free()


class Member:
    """One item of a batch: the rig that knows the circuit, the key handle to verify under (proving or verifying), the proof."""

    def __init__(self, rig, key, kind, proof=None, inst=None, seed=5, reader=None):
        self.rig, self.key, self.kind = rig, key, kind
        self.case = rig.case(kind[0], kind[1], seed=seed)
        self.proof = self.case.proof if proof is None else proof
        self.inst = rig.instances_arg() if inst is None else inst
        self.reader_kw = reader  # None: bytes; else the Reader's hooks
        self.flags = VC.kind_flags(rig.plonk, *kind)

    def group(self):
        return (id(self.key), self.rig.N, self.flags)

    def reader(self):
        return None if self.reader_kw is None else reader_of(self.case, self.proof, **self.reader_kw)

    def item(self):
        plonk = self.rig.plonk
        if self.reader_kw is None:
            return plonk.VerifyItem(self.key, self.inst, self.proof, transcript=self.flags, n_circuits=self.rig.N)
        # of the kind only the opening scheme counts; the bytes are not read
        return plonk.VerifyItem(self.key, self.inst, None, transcript=self.flags & plonk.MULTIOPEN_GWC, n_circuits=self.rig.N, reader=self.reader())

    def with_(self, **kw):
        m = Member.__new__(Member)
        m.__dict__.update(self.__dict__)
        m.__dict__.update(kw)
        return m


def by_group(members):
    groups = {}
    for b, m in enumerate(members):
        groups.setdefault(m.group(), []).append(b)
    return list(groups.values())


def single_key_pairs(ctx, plonk, members, weights):
    """Per group ONE single-key verify_proofs call over its members with their weights: (statuses by position, the sum of the
    calls' pairs as integers)."""
    statuses, L, Rr = [None] * len(members), None, None
    for idx in by_group(members):
        ms = [members[b] for b in idx]
        trs = [m.reader() for m in ms]
        g = plonk.verify_proofs(ctx, ms[0].key, [m.inst for m in ms], [m.proof for m in ms], transcript=ms[0].flags, n_circuits=ms[0].rig.N,
                                combine_scalars=np.stack([weights[b] for b in idx]), transcripts=trs if any(t is not None for t in trs) else None)
        for b, s in zip(idx, g.statuses):
            statuses[b] = s
        l, r = ints(g)
        L, Rr = P.g1_add(L, l), P.g1_add(Rr, r)
    return statuses, (L, Rr)


def single_key_verdicts(ctx, plonk, vparams, members):
    verdicts, statuses = [None] * len(members), [None] * len(members)
    for idx in by_group(members):
        ms = [members[b] for b in idx]
        trs = [m.reader() for m in ms]
        v, s = plonk.decide_proofs(ctx, ms[0].key, vparams, [m.inst for m in ms], [m.proof for m in ms], transcript=ms[0].flags, n_circuits=ms[0].rig.N,
                                   transcripts=trs if any(t is not None for t in trs) else None)
        for b, vb, sb in zip(idx, v, s):
            verdicts[b], statuses[b] = vb, sb
    return verdicts, statuses


def weights_for(n, seed=1):
    rnd = np.random.RandomState(seed)
    return [zu.fr_from_int(int.from_bytes(rnd.bytes(31), "little") + 1) for _ in range(n)]


def check_against_single_key(ctx, plonk, vparams, members, want_statuses=None):
    """The whole contract for one batch: statuses, the pair, per-proof verdicts and the combined verdict. Returns
    (statuses, verdicts)."""
    w = weights_for(len(members), seed=len(members))
    statuses, pair = single_key_pairs(ctx, plonk, members, w)
    g = plonk.verify_proofs_mixed(ctx, [m.item() for m in members], combine_scalars=np.stack(w))
    assert g.statuses == statuses
    if want_statuses is not None:
        assert [tuple(s) for s in g.statuses] == want_statuses
    assert ints(g) == pair
    verdicts, st = single_key_verdicts(ctx, plonk, vparams, members)
    got_v, got_s = plonk.decide_proofs_mixed(ctx, vparams, [m.item() for m in members])
    assert got_s == st == statuses and got_v == verdicts
    comb_v, comb_s = plonk.decide_proofs_mixed(ctx, vparams, [m.item() for m in members], combined=True, combine_scalars=np.stack(w))
    live = [s.status == WELL for s in statuses]
    all_true = all(v for v, l in zip(verdicts, live) if l) and any(live)
    assert comb_s == statuses and comb_v == [l and all_true for l in live]
    return statuses, verdicts


class World:
    """Every key of this file, made once: see the module's docstring."""

    def __init__(self, ctx, pkg, plonk, oracle):
        self.ctx, self.pkg, self.plonk, self.oracle = ctx, pkg, plonk, oracle
        self.vparams = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(TAU))
        self.rigs, self.vks, self.params = {}, [], []
        # one setup at k = 6 and its downsize to k = 4: a lookup-and-permutation circuit and a gate circuit over them
        # (amdzk_srs_downsize itself: ParamsKZG.downsize would free the setup it shrinks; the downsized SRS is another handle)
        p6 = pkg.kzg.ParamsKZG.setup(ctx, 6, zu.fr_from_int(TAU))
        h4 = C.c_void_p()
        ctx._chk(ctx.L.amdzk_srs_downsize(ctx.h, p6.h, 4, C.byref(h4)))
        p4 = pkg.kzg.ParamsKZG.__new__(pkg.kzg.ParamsKZG)
        p4.ctx, p4.k, p4.n, p4._g, p4._gl, p4.h = ctx, 4, 16, None, None, h4
        assert np.array_equal(p4.get_g()[0], p6.get_g()[0])
        self.params += [p4]
        lk6 = Own(ctx, pkg, plonk, oracle, "mixed_lookup6", circuits.lookup_circuit(plonk, 6, seed=3), p6)
        assert lk6.c.k == 6 and lk6.c.desc["lookups"] and lk6.c.desc["permutation_columns"]
        for kind in (B2, EVM):
            lk6.case(*kind)
            lk6.case(*kind, seed=6)
        # ... verified with a verifying key read from a key file, after the SRS and the proving key are freed
        vk = lk6.pk.get_vk()
        blob = vk.write()
        vk.free()
        lk6.free()
        p6.free()
        self.lk6, self.lk6_vk = lk6, plonk.VerifyingKey.read(ctx, blob)[0]
        self.vks.append(self.lk6_vk)
        self.sq_ds = Own(ctx, pkg, plonk, oracle, "square", VC.oracle_key(plonk, "square")[0], p4)
        self.rigs["sq_ds"] = self.sq_ds
        for name, N in (("square", 1), ("rlc", 1), ("lookup", 2)):
            self.rigs[(name, N)] = Rig(ctx, pkg, plonk, oracle, name, N)
        self.lookup2_vk = self.rigs[("lookup", 2)].pk.get_vk()
        self.vks.append(self.lookup2_vk)
        self._padded = {}

    def rig(self, name, N=1):
        return self.rigs[(name, N)]

    def padded(self, target):
        """The k = 4 key whose Blake2b proof has `target` elements, over the downsized setup."""
        if target not in self._padded:
            self._padded[target] = Own(self.ctx, self.pkg, self.plonk, self.oracle, "mixed_padded%d" % target, padded_to(self.plonk, target), self.params[0])
        return self._padded[target]

    def members(self):
        """The mixed batch of the module's docstring: six keys, four circuits and more, both transcript kinds."""
        sq, rlc, lk2 = self.rig("square"), self.rig("rlc"), self.rig("lookup", 2)
        return [Member(sq, sq.pk, B2), Member(self.lk6, self.lk6_vk, EVM), Member(rlc, rlc.pk, B2), Member(lk2, self.lookup2_vk, EVM),
                Member(self.sq_ds, self.sq_ds.pk, B2), Member(self.lk6, self.lk6_vk, B2), Member(sq, sq.pk, EVM), Member(lk2, lk2.pk, B2)]

    def free(self):
        for vk in self.vks:
            vk.free()
        for r in list(self.rigs.values()) + list(self._padded.values()):
            r.free()
        for p in self.params:
            p.free()
        self.vparams.free()


@pytest.fixture(scope="module")
def world(ctx, pkg, plonk, oracle):
    w = World(ctx, pkg, plonk, oracle)
    yield w
    w.free()


# ------------------------------------------------------------------------------------ 1. the same key everywhere
@pytest.mark.parametrize("kind", [B2, EVM], ids=["blake2b_shplonk", "evm_gwc"])
@pytest.mark.parametrize("which", ["pk", "vk"])
def test_one_key_everywhere_gives_the_single_key_calls_words(ctx, plonk, world, kind, which):
    rig = world.rig("lookup", 2)
    key = rig.pk if which == "pk" else world.lookup2_vk
    flags = VC.kind_flags(plonk, *kind)
    a, b = rig.case(*kind), rig.case(*kind, seed=6)
    false = bump_scalar(a)
    for proofs in ([a.proof], [a.proof, false, b.proof], [b.proof] * 17 + [false]):  # one item, several, and across a decide run
        n = len(proofs)
        inst = [rig.instances_arg()] * n
        items = [plonk.VerifyItem(key, rig.instances_arg(), p, transcript=flags, n_circuits=2) for p in proofs]
        w = np.stack(weights_for(n, seed=9))
        for kw in (dict(combine_seed=77), dict(combine_scalars=w), dict()):
            want = plonk.verify_proofs(ctx, key, inst, proofs, transcript=flags, n_circuits=2, **kw)
            got = plonk.verify_proofs_mixed(ctx, items, **kw)
            assert got.statuses == want.statuses and np.array_equal(got.lhs, want.lhs) and np.array_equal(got.rhs, want.rhs)
            assert want.lhs.any() and want.rhs.any()
        for combined in (False, True):
            want = plonk.decide_proofs(ctx, key, world.vparams, inst, proofs, transcript=flags, n_circuits=2, combined=combined, combine_seed=5)
            assert plonk.decide_proofs_mixed(ctx, world.vparams, items, combined=combined, combine_seed=5) == want
            assert want[0] == ([p != false for p in proofs] if not combined else [false not in proofs] * n)


# ------------------------------------------------------------------------------------ 2. mixed batches
def test_mixed_batches_in_several_orders(ctx, plonk, world):
    ms = world.members()
    assert len({m.group() for m in ms}) == 8 and len({id(m.key) for m in ms}) == 6
    assert {m.rig.c.k for m in ms} == {4, 5, 6} and any(m.rig.phased for m in ms) and any(m.rig.N == 2 for m in ms)
    assert all(m.case.accepts() for m in ms), "the device's proofs are not accepted by the oracle"
    rnd = np.random.RandomState(4)
    orders = [list(range(8)), list(range(7, -1, -1)), [0, 1, 0, 2, 1, 3, 4, 0, 5, 6, 7, 5, 1], list(rnd.permutation(8)) + list(rnd.permutation(8))]
    for order in orders:
        batch = [ms[i] for i in order]
        statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch, want_statuses=[(0, 0)] * len(batch))
        assert verdicts == [True] * len(batch)  # the oracle's decisions, asserted above
    # seeded weights belong to positions: the b-th draw, whichever key sits there
    batch = [ms[i] for i in orders[2]]
    seeded = plonk.verify_proofs_mixed(ctx, [m.item() for m in batch], combine_seed=12345)
    rng = PR.ChaCha20Rng(12345)
    given = plonk.verify_proofs_mixed(ctx, [m.item() for m in batch], combine_scalars=np.stack([zu.fr_from_int(rng.fr()) for _ in batch]))
    assert np.array_equal(seeded.lhs, given.lhs) and np.array_equal(seeded.rhs, given.rhs)
    assert VR.holds(ints(seeded), TAU)
    # one item without weights has weight 1, as one proof has
    one = plonk.verify_proofs_mixed(ctx, [ms[1].item()])
    assert ints(one) == ms[1].case.pair() and VR.holds(ints(one), TAU)


# ------------------------------------------------------------------------------------ 3. malformed and false proofs
def first_of(case, kind):
    kinds = VR.element_kinds(case.desc, case.N, case.multiopen)
    return positions(kinds, kind, 64 if case.transcript == "evm" else 32)[0]


def test_malformed_and_false_proofs_in_mixed_positions(ctx, plonk, world):
    ms = world.members()
    big = np.array([zu.limbs(R)], dtype=np.uint64)  # the modulus itself in an instance column
    # a bad point (no curve point has this x) under Blake2b, a bad scalar under EVM, a length, another key's proof, an instance
    p_off, s_off = first_of(ms[0].case, "p"), first_of(ms[1].case, "s")
    bad = {0: (ms[0].with_(proof=put(ms[0].proof, p_off, nonresidue_x().to_bytes(32, "little"))), (BAD_POINT, p_off)),
           1: (ms[1].with_(proof=put(ms[1].proof, s_off, R.to_bytes(32, "big"))), (BAD_SCALAR, s_off)),
           2: (ms[2].with_(proof=ms[2].proof[:-32]), (BAD_LENGTH, 0)),
           4: (ms[4].with_(proof=ms[5].proof), (BAD_LENGTH, 0)),
           7: (ms[7].with_(inst=[[big if i == 0 else col for i, col in enumerate(ms[7].rig.inst)], ms[7].rig.inst]), (BAD_INSTANCE, 0))}
    assert len(ms[5].proof) != len(ms[4].proof)
    clean_status, clean_verdicts = check_against_single_key(ctx, plonk, world.vparams, ms)
    for at, (mutant, want) in bad.items():
        batch = list(ms)
        batch[at] = mutant
        statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch)
        assert [tuple(s) for s in statuses] == [want if b == at else (0, 0) for b in range(8)], at
        assert verdicts == [b != at for b in range(8)]
    # all five at once, and a false proof beside them: per proof it alone is 0 among the live ones, combined everything is
    batch = [bad[b][0] if b in bad else ms[b] for b in range(8)]
    batch[3] = ms[3].with_(proof=bump_scalar(ms[3].case))
    assert not ms[3].case.accepts(batch[3].proof)
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch)
    assert [tuple(s) for s in statuses] == [bad[b][1] if b in bad else (0, 0) for b in range(8)]
    assert verdicts == [False, False, False, False, False, True, True, False]
    false_only = list(ms)
    false_only[3] = batch[3]
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, false_only, want_statuses=[(0, 0)] * 8)
    assert verdicts == [b != 3 for b in range(8)]
    comb, _ = plonk.decide_proofs_mixed(ctx, world.vparams, [m.item() for m in false_only], combined=True, combine_seed=3)
    assert comb == [False] * 8
    # a group whose members are all malformed, between live groups
    sq = world.rig("square")
    dead = Member(sq, sq.pk, B2).with_(proof=put(ms[0].proof, p_off, bytes(32)))  # the identity's encoding
    batch = [ms[1], dead, ms[2], dead.with_(proof=ms[0].proof + bytes(32)), ms[5]]
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch,
                                                  want_statuses=[(0, 0), (BAD_POINT, p_off), (0, 0), (BAD_LENGTH, 0), (0, 0)])
    assert verdicts == [True, False, True, False, True]
    # no well-formed item at all: identities, n_valid = 0, the call ran
    batch = [bad[0][0], bad[1][0], bad[2][0], bad[7][0]]
    g = plonk.verify_proofs_mixed(ctx, [m.item() for m in batch], combine_seed=1)
    assert [tuple(s) for s in g.statuses] == [bad[0][1], bad[1][1], bad[2][1], bad[7][1]] and not g.lhs.any() and not g.rhs.any()
    for combined in (False, True):
        v, s = plonk.decide_proofs_mixed(ctx, world.vparams, [m.item() for m in batch], combined=combined)
        assert v == [False] * 4 and s == g.statuses


# ------------------------------------------------------------------------------------ 4. the mapping's edges
def test_element_counts_on_the_block_edges(ctx, plonk, world):
    sq, lk5 = world.rig("square"), world.rig("lookup", 2)
    edge = {t: world.padded(t) for t in (63, 64, 65)}
    em = {t: Member(r, r.pk, B2) for t, r in edge.items()}
    # with Blake2b every element is 32 bytes: the element count is the proof's length / 32 — computed, not assumed
    counts = {t: len(m.proof) // 32 for t, m in em.items()}
    assert all(len(m.proof) % 32 == 0 for m in em.values()) and counts == {63: 63, 64: 64, 65: 65}
    assert {c % 64 for c in counts.values()} == {63, 0, 1}
    assert all(m.case.accepts() for m in em.values())
    small, large = Member(sq, sq.pk, B2), Member(world.lk6, world.lk6_vk, B2)
    assert len({len(m.proof) for m in (small, large, *em.values())}) == 5  # neighbours of unequal size
    for t, m in em.items():
        check_against_single_key(ctx, plonk, world.vparams, [m], want_statuses=[(0, 0)])  # a one-item batch
        # bad in turn: the last element (with 65 the only one of its block) and the last element of the first block
        kinds = VR.element_kinds(m.case.desc, 1, "shplonk")
        for e in (t - 1, min(t - 1, 63) - (t == 64)):
            data, cls = (nonresidue_x().to_bytes(32, "little"), BAD_POINT) if kinds[e] == "p" else (R.to_bytes(32, "little"), BAD_SCALAR)
            mutant = m.with_(proof=put(m.proof, 32 * e, data))
            check_against_single_key(ctx, plonk, world.vparams, [small, mutant, large], want_statuses=[(0, 0), (cls, 32 * e), (0, 0)])
    # neighbours of unequal size on both sides of each
    batch = [small, em[63], large, em[64], small, em[65], large, em[65], em[64], em[63], Member(lk5, lk5.pk, EVM)]
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch, want_statuses=[(0, 0)] * len(batch))
    assert verdicts == [True] * len(batch)


def test_forty_items_of_four_groups_and_a_run_without_a_live_item(ctx, plonk, world):
    sq = world.rig("square")
    four = [Member(sq, sq.pk, B2), Member(world.padded(64), world.padded(64).pk, B2), Member(world.lk6, world.lk6_vk, EVM),
            Member(world.padded(65), world.padded(65).pk, B2)]
    batch = [four[b % 4] for b in range(40)]
    assert plonk.DECIDE_RUN == 16 and all(len({m.group() for m in batch[r:r + 16]}) == 4 for r in (0, 16, 32))
    batch[5] = four[1].with_(proof=bump_scalar(four[1].case))  # a false proof in the first run
    batch[37] = four[1].with_(proof=four[1].proof[:-32])
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch)
    assert verdicts == [b not in (5, 37) for b in range(40)] and statuses[37].status == BAD_LENGTH
    # positions 16 .. 31 all malformed: that run launches nothing, the runs around it are unaffected
    for b in range(16, 32):
        batch[b] = batch[b].with_(proof=batch[b].proof + bytes(32)) if b % 2 else batch[b].with_(proof=put(batch[b].proof, 0, bytes(64)))
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch)
    assert all(statuses[b].status in (BAD_LENGTH, BAD_POINT) for b in range(16, 32))
    assert verdicts == [b not in (5, 37) and not 16 <= b < 32 for b in range(40)]


# ------------------------------------------------------------------------------------ 5. caller-owned read transcripts
def test_read_transcripts_beside_bytes_items_of_other_keys(ctx, plonk, world):
    ms = world.members()
    batch = [ms[0].with_(reader_kw={}), ms[1], ms[3].with_(reader_kw={}), ms[5], ms[4].with_(reader_kw={}), ms[6].with_(reader_kw={}), ms[7],
             world_padded_member(world, 65).with_(reader_kw={})]
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, batch, want_statuses=[(0, 0)] * len(batch))
    assert verdicts == [True] * len(batch)
    # every element was read once, in the proof's order, proof after proof in ascending position
    readers = [m.reader() for m in batch]
    items = []
    for m, rd in zip(batch, readers):
        it = m.item()
        if rd is not None:
            it.reader = rd
        items.append(it)
    g = plonk.verify_proofs_mixed(ctx, items, combine_seed=8)
    assert g.errors == [] and g.well_formed
    for m, rd in zip(batch, readers):
        if rd is not None:
            assert "".join(k for k in rd.order if k != "c") == VR.element_kinds(m.case.desc, m.rig.N, m.kind[1]) and rd.inner.pos == len(rd.inner.data)
    # the same items through bytes: the same words
    same = plonk.verify_proofs_mixed(ctx, [m.with_(reader_kw=None).item() for m in batch], combine_seed=8)
    assert np.array_equal(g.lhs, same.lhs) and np.array_equal(g.rhs, same.rhs)
    # a callback failure: its status and its read count, the others untouched; bad words get the element's index
    pts, _ = VC.decoded_elements(ms[0].case)
    off_curve = zu.point_from_ints((pts[1][0], (pts[1][1] + 1) % Q))
    failing = list(batch)
    failing[2] = batch[2].with_(reader_kw=dict(fail=("read", 5)))
    failing[0] = batch[0].with_(reader_kw=dict(replace={1: off_curve}))
    it = [m.item() for m in failing]
    g = plonk.verify_proofs_mixed(ctx, it, combine_seed=8)
    assert [tuple(s) for s in g.statuses] == [(BAD_POINT, 1), (0, 0), (BAD_TRANSCRIPT, 5)] + [(0, 0)] * 5
    assert len(g.errors) == 1 and isinstance(g.errors[0], _Refuse) and it[2].reader.reads == 5
    statuses, verdicts = check_against_single_key(ctx, plonk, world.vparams, failing)
    assert statuses == g.statuses and verdicts == [False, True, False] + [True] * 5


def world_padded_member(world, target):
    r = world.padded(target)
    return Member(r, r.pk, B2)


# ------------------------------------------------------------------------------------ 6. refusals
def test_every_refusal_names_its_item_and_leaves_the_ctx_usable(ctx, pkg, plonk, oracle, world):
    ms = world.members()
    L, ffi = ctx.L, pkg.ffi
    good = [ms[0].item(), ms[1].item(), ms[4].item()]
    arr, opts, st, keep = plonk._mixed_args(good, 0, None, None, [])
    pair = np.zeros(16, np.uint64)
    verdicts, n_valid = np.zeros(3, np.uint8), C.c_size_t(0)
    sg2, g2 = world.vparams.s_g2.h, world.vparams.g2.h

    def refused(rc, needle):
        msg = L.amdzk_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("verify_proofs_mixed: ") and needle in msg, (rc, msg)
        assert L.amdzk_sync(ctx.h) == 0

    def both(needle, items=arr, n=3, o=C.byref(opts), status=st):
        refused(L.amdzk_verify_proofs_mixed(ctx.h, items, n, o, status, pair.ctypes.data), needle)
        refused(L.amdzk_verify_proofs_decide_mixed(ctx.h, sg2, g2, 0, items, n, o, status, verdicts.ctypes.data, C.byref(n_valid)), needle)

    assert L.amdzk_verify_proofs_mixed(None, arr, 3, C.byref(opts), st, pair.ctypes.data) == -2
    both("null argument", items=None)
    both("null argument", status=None)
    refused(L.amdzk_verify_proofs_mixed(ctx.h, arr, 3, C.byref(opts), st, None), "null argument")
    for a in (dict(s=None), dict(g=None), dict(v=None)):
        refused(L.amdzk_verify_proofs_decide_mixed(ctx.h, a.get("s", sg2), a.get("g", g2), 0, arr, 3, C.byref(opts), st,
                                                   a.get("v", verdicts.ctypes.data), C.byref(n_valid)), "null argument")
    refused(L.amdzk_verify_proofs_decide_mixed(ctx.h, sg2, g2, 2, arr, 3, C.byref(opts), st, verdicts.ctypes.data, C.byref(n_valid)), "unknown flags")
    both("n_items is 0", n=0)
    both("2^20", n=(1 << 20) + 1)
    small = ffi.VerifyMixedOpts(C.sizeof(ffi.VerifyMixedOpts) - 1, 0, None)
    both("amdzk_verify_mixed_opts.size", o=C.byref(small))

    def edited(b, **fields):
        out = (ffi.VerifyItem * 3)()
        for i in range(3):
            out[i] = arr[i]
        for k, v in fields.items():
            setattr(out[b], k, v)
        return out

    both("item 1: exactly one of pk and vk", items=edited(1, pk=ms[0].key.h))  # both set
    both("item 2: exactly one of pk and vk", items=edited(2, pk=None))         # neither
    both("item 1: unknown transcript kind", items=edited(1, transcript_kind=7))
    both("item 2: unknown transcript kind", items=edited(2, transcript_kind=0x200))
    both("item 0: null argument (proof)", items=edited(0, proof=None))
    both("item 1: n_circuits out of range", items=edited(1, n_circuits=(1 << 16) + 1))
    both("item 1: null argument (instances)", items=edited(1, instances=None))
    sc = np.stack([zu.fr_from_int(3), np.array(zu.limbs(R), dtype=np.uint64), zu.fr_from_int(5)])
    bad_w = ffi.VerifyMixedOpts(C.sizeof(ffi.VerifyMixedOpts), 0, sc.ctypes.data)
    refused(L.amdzk_verify_proofs_mixed(ctx.h, arr, 3, C.byref(bad_w), st, pair.ctypes.data), "combine_scalars[1]")
    # the one rule: a key made over a setup with another G. (Another TRAPDOOR alone does not make one: g[0] = s^0 G is the
    # generator for every s — test_a_key_over_another_trapdoor... below — so the other setup starts from H = 7 G.)
    other = OtherSetup(ctx, pkg, plonk, oracle)
    try:
        wrong = other.member()
        for items, at in (([ms[0], ms[1], wrong, ms[4]], 2), ([ms[1], wrong], 1), ([wrong, wrong, ms[0]], 2)):
            with pytest.raises(pkg.ffi.AmdzkError, match=r"verify_proofs_mixed: item %d: its key was made over another G" % at) as e:
                plonk.verify_proofs_mixed(ctx, [m.item() for m in items], combine_seed=1)
            assert e.value.code == -2 and L.amdzk_sync(ctx.h) == 0
            with pytest.raises(pkg.ffi.AmdzkError, match=r"verify_proofs_mixed: item %d: " % at):
                plonk.decide_proofs_mixed(ctx, world.vparams, [m.item() for m in items])
        # alone, or among keys of its own setup, it is fine
        assert plonk.verify_proofs_mixed(ctx, [wrong.item(), wrong.item()], combine_seed=1).well_formed
    finally:
        other.free()
    # the ctx proves and verifies afterwards
    sq = world.rig("square")
    fresh = sq.case("blake2b", "shplonk", seed=1234)
    assert fresh.accepts()
    assert L.amdzk_verify_proofs_mixed(ctx.h, arr, 3, C.byref(opts), st, pair.ctypes.data) == 0
    assert [(s.status, s.offset) for s in st] == [(0, 0)] * 3
    v, s = plonk.decide_proofs_mixed(ctx, world.vparams, good + [plonk.VerifyItem(sq.pk, sq.inst, fresh.proof)])
    assert v == [True] * 4
    # a wrong [s]_2: verdict 0 everywhere, in both modes
    wrong_v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(OTHER_TAU))
    try:
        for combined in (False, True):
            v, s = plonk.decide_proofs_mixed(ctx, wrong_v, good, combined=combined, combine_seed=2)
            assert v == [False] * 3 and [tuple(x) for x in s] == [(0, 0)] * 3
    finally:
        wrong_v.free()
    del keep


def test_a_key_over_another_trapdoor_shares_g_and_fails_its_pairing(ctx, pkg, plonk, oracle, world):
    """Two setups with different trapdoors have the SAME G (g[0] is the generator), so the rule cannot tell them apart and
    does not refuse: the foreign item is well formed and its own pairing under the batch's [s]_2 fails, as the single-key call
    decides it."""
    ms = world.members()
    other = OtherSetup(ctx, pkg, plonk, oracle, scale=1, tau=OTHER_TAU)
    try:
        foreign = other.member()
        batch = [ms[0], foreign, ms[1]]
        v, s = plonk.decide_proofs_mixed(ctx, world.vparams, [m.item() for m in batch])
        assert [tuple(x) for x in s] == [(0, 0)] * 3 and v == [True, False, True]
        assert plonk.decide_proofs(ctx, foreign.key, world.vparams, [foreign.inst], [foreign.proof]) == ([False], [s[1]])
        v, _ = plonk.decide_proofs_mixed(ctx, world.vparams, [m.item() for m in batch], combined=True, combine_seed=4)
        assert v == [False] * 3
        own_v = pkg.kzg.ParamsVerifierKZG.setup(ctx, zu.fr_from_int(OTHER_TAU))
        try:
            assert plonk.decide_proofs_mixed(ctx, own_v, [m.item() for m in batch])[0] == [False, True, False]
        finally:
            own_v.free()
    finally:
        other.free()


class OtherSetup:
    """A square-circuit key over another setup: the bases [tau^i] H with H = scale * G, uploaded as an SRS (scale = 1 with
    another tau: another trapdoor over the same G)."""

    def __init__(self, ctx, pkg, plonk, oracle, scale=7, tau=TAU):
        c = VC.oracle_key(plonk, "square")[0]
        g, gl = zu.test_srs(oracle, c.k, tau)
        if scale != 1:
            g, gl = (np.ascontiguousarray(np.stack([zu.point_from_ints(P.g1_mul(zu.point_to_ints(p), scale)) for p in b])) for b in (g, gl))
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        self.rig = Own(ctx, pkg, plonk, oracle, "square", c, self.params)

    def member(self):
        rig = self.rig
        proof = rig.plonk.create_proof(rig.ctx, rig.pk, rig.inst, rig.d_adv[0], seed=5)
        m = Member.__new__(Member)
        m.rig, m.key, m.kind, m.proof, m.inst, m.reader_kw, m.flags = rig, rig.pk, B2, proof, rig.instances_arg(), None, 0
        m.case = None
        return m

    def free(self):
        self.rig.free()
        self.params.free()
