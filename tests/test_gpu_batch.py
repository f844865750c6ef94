"""GPU: amdzk_create_proof_batch — B independent proofs of one circuit advanced in lock-step on one stream, every step's
commitments of all proofs in ONE pointer-table MSM (amdzk_msm_g1_cols_dev) — and that MSM on its own.

The oracle of a batch is the single-proof path: proof b's bytes are those of create_proof on the same workspace with the
same seed (and, for proof 0 of the shape test, those of the pure-Python protocol oracle)."""
import os
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import phased_circuits as PC  # noqa: E402
import plonk_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
SMALL = dict(k=7, num_advice=5, num_lookup_advice=2, lookup_bits=5, num_spread=2, spread_bits=3)
_srs_cache = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


class Batch:
    """One circuit on the device with B workspaces (the key and B - 1 clones) and B witnesses (advice ints, instance ints)."""

    def __init__(self, ctx, pkg, plonk, oracle, c, witnesses, flags=None):
        self.ctx, self.plonk, self.c = ctx, plonk, c
        if c.k not in _srs_cache:
            _srs_cache[c.k] = zu.test_srs(oracle, c.k, TAU)
        g, gl = _srs_cache[c.k]
        self.params = pkg.kzg.ParamsKZG(ctx, c.k, g=g, g_lagrange=gl)
        fixed = np.stack([zu.ints_to_fr(oracle, col) for col in c.fixed]) if c.fixed else np.zeros((0, c.n, 4), np.uint64)
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=flags)
        self.pks = [self.pk] + [self.pk.clone_workspace() for _ in witnesses[1:]]
        self.d_adv, self.inst = [], []
        for adv, inst in witnesses:
            arr = np.stack([zu.ints_to_fr(oracle, col) for col in adv])
            self.d_adv.append(ctx.alloc(arr.nbytes).upload(arr))
            self.inst.append([zu.ints_to_fr(oracle, col) if len(col) else np.zeros((0, 4), np.uint64) for col in inst])

    def batch(self, seeds, transcript=0, idx=None, **kw):
        idx = list(range(len(self.pks))) if idx is None else idx
        return self.plonk.create_proof_batch(self.ctx, [self.pks[i] for i in idx], [self.inst[i] for i in idx],
                                             [self.d_adv[i] for i in idx], seeds, transcript=transcript, **kw)

    def single(self, b, seed, transcript=0):
        return self.plonk.create_proof(self.ctx, self.pks[b], self.inst[b], self.d_adv[b], seed=seed, transcript=transcript)

    def vk(self):
        f, p = self.pk.commitments()
        return PR.VerifyingKey(self.c.desc, [zu.point_to_ints(x) for x in f], [zu.point_to_ints(x) for x in p], TAU, REPR)

    def free(self):
        for d in self.d_adv:
            d.free()
        for pk in self.pks[1:]:
            pk.free()
        self.pk.free()
        self.params.free()


def small_shape(plonk, seeds=(0, 301, 302)):
    c = circuits.rsa_sha256_shape(plonk, **SMALL)
    wit = [(c.advice, c.instances) if s == 0 else c.witness(s) for s in seeds]
    return c, wit


@pytest.mark.parametrize("transcript", ["blake2b", "evm", "blake2b+gwc"])
def test_three_witnesses_of_one_layout(ctx, pkg, plonk, oracle, transcript):
    """B = 3 (odd, > 2) on the smallest RSA-SHA256 shape (gates, both lookup kinds, a permutation over every column, two
    instance columns): three witnesses, the key and two clones, distinct seeds. Every batch proof equals create_proof on
    the same workspace with the same seed; proof 0 equals the protocol oracle's bytes and verifies."""
    c, wit = small_shape(plonk)
    assert wit[1][0] != wit[0][0] and wit[2][0] != wit[1][0]
    tk = {"blake2b": plonk.TRANSCRIPT_BLAKE2B, "evm": plonk.TRANSCRIPT_KECCAK256_EVM, "blake2b+gwc": plonk.TRANSCRIPT_BLAKE2B | plonk.MULTIOPEN_GWC}[transcript]
    okw = dict(transcript="evm" if transcript == "evm" else "blake2b", multiopen="gwc" if transcript.endswith("gwc") else "shplonk")
    B = Batch(ctx, pkg, plonk, oracle, c, wit)
    seeds = [7, 8, 9]
    got = B.batch(seeds, transcript=tk)
    assert all(isinstance(p, bytes) for p in got) and len(set(got)) == 3
    for b in range(3):
        assert got[b] == B.single(b, seeds[b], tk), "proof %d" % b
        assert len(got[b]) == plonk.proof_size(ctx, B.pk, tk)
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    assert got[0] == PR.create_proof(opk, c.instances, c.advice, seed=7, **okw)
    assert PR.verify_proof(B.vk(), c.instances, got[0], **okw)
    assert B.batch(seeds, transcript=tk) == got  # the workspaces are reused cleanly
    B.free()


def test_batch_of_one_and_the_same_witness_twice(ctx, pkg, plonk, oracle):
    """B = 1 is the single call. B = 2 with the same witness and two seeds: two different proofs, each its single twin's."""
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    B = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances)] * 2)
    assert B.batch([3], idx=[0]) == [B.single(0, 3)]
    assert B.batch([3], idx=[1]) == [B.single(1, 3)]  # a clone alone
    got = B.batch([3, 4])
    assert got[0] != got[1]
    assert got == [B.single(0, 3), B.single(1, 4)]
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    assert got[1] == PR.create_proof(opk, c.instances, c.advice, seed=4)
    B.free()


def test_instance_lengths_differ_between_proofs(ctx, pkg, plonk, oracle):
    """B = 2 on SquareCircuit (its one instance column is absorbed by the transcript and not constrained): proof 0 has one
    public input, proof 1 three, and different signals. Each proof equals its single twin and the oracle's bytes."""
    c0 = circuits.square_circuit(plonk, 4, signal=5)
    c1 = circuits.square_circuit(plonk, 4, signal=11)
    wit = [(c0.advice, [[25]]), (c1.advice, [[121, 0, 7]])]
    B = Batch(ctx, pkg, plonk, oracle, c0, wit)
    got = B.batch([21, 22])
    assert got == [B.single(0, 21), B.single(1, 22)] and got[0] != got[1]
    opk = PR.keygen(c0.desc, c0.fixed, c0.assembly.mapping, TAU, transcript_repr=REPR)
    for b in range(2):
        assert got[b] == PR.create_proof(opk, wit[b][1], wit[b][0], seed=21 + b)
    B.free()


def test_caller_scalars_equal_the_seeded_streams(ctx, pkg, plonk, oracle):
    """amdzk_batch_opts.scalars with the draws ChaCha20Rng::seed_from_u64(seed_b) would have made: the seeded batch's bytes
    (and amdzk_create_proof_scalars' per proof). Too few scalars are refused."""
    c, wit = small_shape(plonk, seeds=(0, 301))
    B = Batch(ctx, pkg, plonk, oracle, c, wit)
    cnt = plonk.proof_random_count(ctx, B.pk)
    draws = []
    for seed in (77, 78):
        rng = PR.ChaCha20Rng(seed)
        draws.append(zu.ints_to_fr(oracle, [rng.fr() for _ in range(cnt)]))
    want = B.batch([77, 78])
    assert B.batch(None, scalars=draws) == want
    for b in range(2):
        assert plonk.create_proof_with_scalars(ctx, B.pks[b], B.inst[b], B.d_adv[b], draws[b]) == want[b]
    with pytest.raises(pkg.AmdzkError, match="scalars"):
        B.batch(None, scalars=[draws[0], draws[1][:-1]])
    assert B.batch([77, 78]) == want
    B.free()


def test_default_and_serial_keys_give_the_same_bytes(ctx, pkg, plonk, oracle):
    c, wit = small_shape(plonk, seeds=(0, 301))
    out = []
    for flags in (None, plonk.KEYGEN_SERIAL):
        B = Batch(ctx, pkg, plonk, oracle, c, wit, flags=flags)
        out.append(B.batch([5, 6]))
        assert out[-1] == [B.single(0, 5), B.single(1, 6)]
        B.free()
    assert out[0] == out[1]


def test_several_permutation_sets_and_lookups(ctx, pkg, plonk, oracle):
    """B = 2 on the composite Aadhaar shape at the small k where test_full_aadhaar_shape_equals_oracle compares it with the
    pure-Python oracle: bytes equal the single path for both transcripts."""
    c = circuits.full_aadhaar_shape(plonk, **SMALL)
    assert len(c.desc["permutation_columns"]) > c.desc["cs_degree"] - 2 and len(c.desc["lookups"]) > 1
    B = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances), c.witness(41)])
    for tk in (plonk.TRANSCRIPT_BLAKE2B, plonk.TRANSCRIPT_KECCAK256_EVM):
        got = B.batch([9, 10], transcript=tk)
        assert got == [B.single(0, 9, tk), B.single(1, 10, tk)]
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    assert B.batch([9, 10])[0] == PR.create_proof(opk, c.instances, c.advice, seed=9)
    B.free()


def test_the_commitments_really_are_merged(ctx, pkg, plonk, oracle):
    """Per-kernel profiling (a supported mode of the ctx): a B = 3 batch launches the level-1 accumulation exactly as often
    as a B = 1 batch — one MSM submission per commitment step, whatever B — and fewer than three times the kernels of a
    B = 1 batch in all."""
    c, wit = small_shape(plonk)
    B = Batch(ctx, pkg, plonk, oracle, c, wit)
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


def test_one_bad_witness_does_not_cost_the_batch(ctx, pkg, plonk, oracle):
    """B = 3 on lookup_circuit(k = 5), proof 1's advice broken as test_lookup_failure_is_reported breaks it: its status is
    AMDZK_E_INVALID, the message names the proof and the lookup, its length is 0; proofs 0 and 2 are their single twins';
    all three workspaces then prove the right bytes alone."""
    import ctypes as C
    c = circuits.lookup_circuit(plonk, 5, seed=4)
    bad = [list(col) for col in c.advice]
    rows = [r for r in range(c.usable) if c.fixed[2][r] == 1]
    bad[0][rows[0]] = 9  # not in the 0..7 range table
    B = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances), (bad, c.instances), (c.advice, c.instances)])
    got = B.batch([5, 6, 7])
    assert isinstance(got[1], pkg.AmdzkError) and got[1].code == -2
    assert "proof 1" in str(got[1]) and "lookup 0 input not in table" in str(got[1])
    assert got[0] == B.single(0, 5) and got[2] == B.single(2, 7)
    # the raw call: return value = the first failing proof's status, proof_lens[1] = 0, statuses = NULL changes nothing else
    N, n = 3, c.n
    keep = []
    inst_pp, lens_pp = (C.POINTER(C.c_void_p) * N)(), (C.POINTER(C.c_size_t) * N)()
    for b in range(N):
        cols = [np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4) for x in B.inst[b]]
        ptrs = (C.c_void_p * len(cols))(*[x.ctypes.data if x.size else None for x in cols])
        lens = (C.c_size_t * len(cols))(*[x.shape[0] for x in cols])
        keep += [cols, ptrs, lens]
        inst_pp[b], lens_pp[b] = C.cast(ptrs, C.POINTER(C.c_void_p)), C.cast(lens, C.POINTER(C.c_size_t))
    keys = (C.c_void_p * N)(*[pk.h for pk in B.pks])
    adv = (C.c_void_p * N)(*[d.ptr for d in B.d_adv])
    seeds = np.array([5, 6, 7], np.uint64)
    opts = pkg.ffi.BatchOpts(C.sizeof(pkg.ffi.BatchOpts), 0, seeds.ctypes.data, None, 0)
    stride = plonk.proof_size(ctx, B.pk)
    for with_statuses in (True, False):
        buf, lens_out, st = (C.c_uint8 * (stride * N))(), (C.c_size_t * N)(7, 7, 7), (C.c_int * N)(1, 1, 1)
        rc = ctx.L.amdzk_create_proof_batch(ctx.h, keys, N, inst_pp, lens_pp, adv, n, C.byref(opts), buf, stride, lens_out,
                                            st if with_statuses else None)
        assert rc == -2 and ctx.L.amdzk_last_error(ctx.h).decode().startswith("proof 1: ")
        assert list(lens_out) == [stride, 0, stride]
        if with_statuses:
            assert list(st) == [0, -2, 0]
        assert bytes(buf[:stride]) == got[0] and bytes(buf[2 * stride: 3 * stride]) == got[2]
    # every workspace is quiet and proves alone
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    want = PR.create_proof(opk, c.instances, c.advice, seed=11)
    assert B.single(0, 11) == want and B.single(2, 11) == want
    B.d_adv[1].upload(np.stack([zu.ints_to_fr(oracle, col) for col in c.advice]))
    assert B.single(1, 11) == want
    assert B.batch([11, 11, 11]) == [want] * 3
    B.free()


def test_refusals_leave_the_ctx_usable(ctx, pkg, plonk, oracle):
    """Every refused batch gives the documented status and a message, and a good batch succeeds right after it."""
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    B = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances)] * 2)
    other = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances)] * 2)  # the same circuit, another key
    want = [B.single(0, 3), B.single(1, 4)]
    INVALID, UNSUPPORTED = -2, -5

    def refused(code, match, fn):
        with pytest.raises(pkg.AmdzkError, match=match) as e:
            fn()
        assert e.value.code == code
        assert B.batch([3, 4]) == want

    pc = PC.rlc_circuit(plonk, 5, seed=2)
    P = Batch(ctx, pkg, plonk, oracle, pc, [(pc.advice, pc.instances)])
    refused(UNSUPPORTED, "amdzk_create_proof_opts", lambda: P.batch([1]))
    P.free()
    refused(INVALID, "no proofs", lambda: plonk.create_proof_batch(ctx, [], [], [], []))
    refused(INVALID, "share one workspace", lambda: plonk.create_proof_batch(ctx, [B.pk, B.pk], B.inst, B.d_adv, [3, 4]))
    refused(INVALID, "not the first key or a workspace clone",
            lambda: plonk.create_proof_batch(ctx, [B.pk, other.pks[1]], B.inst, B.d_adv, [3, 4]))
    refused(INVALID, "create_proof_batch: proof 1's key is not the first key or a workspace clone of it",  # a clone of one key, the other key
            lambda: plonk.create_proof_batch(ctx, [B.pks[1], other.pk], B.inst, B.d_adv, [3, 4]))
    refused(INVALID, "proof_stride", lambda: B.batch([3, 4], proof_stride=plonk.proof_size(ctx, B.pk) - 1))
    refused(INVALID, "amdzk_batch_opts.size", lambda: B.batch([3, 4], opts_size=8))
    refused(INVALID, "neither rng_seeds nor scalars", lambda: B.batch(None))
    refused(INVALID, "null advice", lambda: plonk.create_proof_batch(ctx, B.pks, B.inst, [B.d_adv[0], None], [3, 4]))
    # the raw call: a refusal writes its status and a length of 0 for every proof, whatever the arrays held
    import ctypes as C
    keys = (C.c_void_p * 2)(B.pk.h, B.pk.h)
    adv = (C.c_void_p * 2)(*[d.ptr for d in B.d_adv])
    seeds = np.array([3, 4], np.uint64)
    opts = pkg.ffi.BatchOpts(C.sizeof(pkg.ffi.BatchOpts), 0, seeds.ctypes.data, None, 0)
    stride = plonk.proof_size(ctx, B.pk)
    buf, lens_out, st = (C.c_uint8 * (2 * stride))(), (C.c_size_t * 2)(7, 7), (C.c_int * 2)(1, 1)
    rc = ctx.L.amdzk_create_proof_batch(ctx.h, keys, 2, None, None, adv, c.n, C.byref(opts), buf, stride, lens_out, st)
    assert rc == INVALID and list(st) == [INVALID, INVALID] and list(lens_out) == [0, 0]
    assert ctx.L.amdzk_last_error(ctx.h).decode().startswith("create_proof_batch:")
    assert B.batch([3, 4]) == want
    other.free()
    B.free()


def test_a_batch_on_two_clones_after_the_first_handle_is_freed(ctx, pkg, plonk, oracle):
    """The handles of a key are equals: a batch of two proofs on two clones, with the handle keygen returned already freed,
    gives the oracle's bytes (k = 5: a constant table, a permutation and both lookup kinds)."""
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    B = Batch(ctx, pkg, plonk, oracle, c, [(c.advice, c.instances)] * 3)
    B.pk.free()
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    assert B.batch([3, 4], idx=[1, 2]) == [PR.create_proof(opk, c.instances, c.advice, seed=s) for s in (3, 4)]
    B.free()


@pytest.mark.parametrize("k", [6, 12])
def test_pointer_table_msm_equals_the_strided_msm(ctx, pkg, oracle, k):
    """amdzk_msm_g1_cols_dev against amdzk_msm_g1_dev on the same columns, word for word: 5 columns scattered over three
    separately allocated buffers (not in address order), one all zero, and a ragged length (len < n) — for both bases, in
    one submission and cut into runs of columns by ever smaller max_scratch_bytes."""
    A = pkg.arithmetic
    n = 1 << k
    params = pkg.kzg.ParamsKZG.setup(ctx, k, zu.fr_from_int(TAU))
    cols = [zu.random_fr(n, seed=100 * k + j) for j in range(5)]
    cols[1] = zu.skewed_fr(n, 100 * k + 1, oracle)
    cols[3] = np.zeros((n, 4), np.uint64)
    cols = [np.ascontiguousarray(col, dtype=np.uint64) for col in cols]
    packed = ctx.alloc(5 * n * 32).upload(np.stack(cols))  # the strided twin
    bufs = [ctx.alloc(2 * n * 32 + 64), ctx.alloc(n * 32), ctx.alloc(2 * n * 32)]
    place = [(2, 0), (0, 48), (1, 0), (2, n * 32), (0, 48 + n * 32)]  # column -> (buffer, byte offset): 16-byte aligned, not 32
    ptrs = []
    for col, (b, off) in zip(cols, place):
        ctx._chk(ctx.L.amdzk_dev_upload(ctx.h, bufs[b].ptr.value + off, col.ctypes.data, col.nbytes))
        ptrs.append(bufs[b].ptr.value + off)
    for basis in (0, 1):
        for length in (n, n - 5):
            want = A.best_multiexp_dev(ctx, params.h, basis, packed, 5, length, col_stride=n)
            got = A.best_multiexp_cols_dev(ctx, params.h, basis, ptrs, length)
            assert np.array_equal(got, want), "basis %d len %d" % (basis, length)
            assert not got[3][8:].any()  # the all-zero column: the identity, z = 0
    # cut into runs: ever smaller scratch bounds (steps of sqrt 2: finer than the 5 : 3 between the geometries of 5 and 3
    # columns) go from one run to five runs of one column. A run is one level-1 launch (per-kernel profiling), so the
    # count says which cut a bound gave: 1 = 5 columns, 2 = 3 + 2, 3 = 2 + 2 + 1 (both with a shorter last run), 5 = 1 each.
    want = A.best_multiexp_dev(ctx, params.h, 1, packed, 5, n, col_stride=n)
    runs = []
    ctx.prof_enable(True)
    try:
        for cap in [int(2 ** (s / 2)) for s in range(60, 19, -1)] + [1]:
            ctx.prof_reset()
            assert np.array_equal(A.best_multiexp_cols_dev(ctx, params.h, 1, ptrs, n, max_scratch_bytes=cap), want), "cap %d" % cap
            runs.append(ctx.prof_dump()["msm_accum_l1"][0])
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()
    print("k=%d runs per bound: %s" % (k, runs))
    assert runs[0] == 1 and runs[-1] == 5 and runs == sorted(runs) and set(runs) <= {1, 2, 3, 5}
    assert set(runs) & {2, 3}, "no bound cut the columns into runs with a shorter last run"
    with pytest.raises(pkg.AmdzkError, match="null"):
        A.best_multiexp_cols_dev(ctx, params.h, 1, ptrs[:2] + [0], n)
    assert np.array_equal(A.best_multiexp_cols_dev(ctx, params.h, 1, ptrs, n), want)
    for b in bufs + [packed]:
        b.free()
    params.free()
