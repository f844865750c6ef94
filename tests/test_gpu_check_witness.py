"""GPU: amdzk_check_witness — failing gates, lookups and copy constraints of a witness, found on the device.

The device's full report equals the reference's (tests/witness_check_ref.py: Python integers, exact tuples), entry for
entry, in every case: satisfied fixtures, random circuits with one corrupted cell, the row and lookup edge cases, keys
of every origin, phased keys. At the metric shape (k = 15), where the Python walk is too slow to run in full, every
reported entry is confirmed by the reference at its first_row."""
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
import witness_check_cases as K  # noqa: E402
import witness_check_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
R = zu.R


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


def fr_cols(oracle, cols, n):
    return np.stack([zu.ints_to_fr(oracle, col) for col in cols]) if cols else np.zeros((0, n, 4), np.uint64)


def fr_inst(oracle, instances):
    return [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in instances]


class Dev:
    """One circuit's key on the device and the check of any witness of it."""

    def __init__(self, ctx, plonk, oracle, srs, c):
        self.ctx, self.plonk, self.oracle, self.c = ctx, plonk, oracle, c
        self.params = srs(c.k)
        self.fixed = fr_cols(oracle, c.fixed, c.n)
        self.pk = plonk.ProvingKey(ctx, self.params, c.desc, self.fixed, c.assembly.mapping, zu.fr_from_int(REPR))
        self.d_adv = ctx.alloc(max(32, len(c.advice) * c.n * 32))

    def upload(self, advice=None):
        self.d_adv.upload(fr_cols(self.oracle, self.c.advice if advice is None else advice, self.c.n))
        return self.d_adv

    def report(self, advice=None, instances=None, pk=None, **kw):
        inst = fr_inst(self.oracle, self.c.instances if instances is None else instances)
        rep = self.plonk.check_witness(self.ctx, pk or self.pk, inst, self.upload(advice), **kw)
        assert rep.ok == (not rep.failures)
        return [tuple(f) for f in rep.failures]

    def free(self):
        self.d_adv.free()
        self.pk.free()


def check_equal(dev, advice=None, instances=None, **kw):
    want = W.report(dev.c, advice=advice, instances=instances)
    got = dev.report(advice=advice, instances=instances, **kw)
    assert got == want
    return got


# ---------------------------------------------------------------------------------------------- satisfied fixtures
@pytest.mark.parametrize("name", ["square-k4", "high-degree", "lookup-range-first", "lookup-pair-first"])
def test_satisfied_fixtures_give_an_empty_report(ctx, plonk, oracle, srs, name):
    c = {"square-k4": lambda: circuits.square_circuit(plonk, 4), "high-degree": lambda: circuits.high_degree_circuit(plonk),
         "lookup-range-first": lambda: circuits.lookup_circuit(plonk, 5, seed=2),
         "lookup-pair-first": lambda: circuits.lookup_circuit(plonk, 5, seed=2, tables="pair_first")}[name]()
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert dev.report() == [] == W.report(c)
    assert dev.report(theta_seed=99) == []
    dev.free()


@pytest.mark.parametrize("seed", K.RANDOM_SEEDS)
def test_random_circuits_satisfied(ctx, plonk, oracle, srs, seed):
    c = K.random_circuit(plonk, seed)
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert dev.report() == [] == W.report(c)
    dev.free()


@pytest.mark.parametrize("seed,way", K.CORRUPTED_CASES)
def test_random_circuits_with_one_corrupted_cell(ctx, plonk, oracle, srs, seed, way):
    """One advice cell changed — a cell an enabled gate reads, a lookup input cell, a cell of a copy cycle of length >= 3
    across column kinds: the device's report is the reference's, and the good witness is accepted again afterwards on the
    workspace the bad one left. Every case exists (witness_check_cases.WAY_SEEDS): none is skipped."""
    c = K.random_circuit(plonk, seed)
    made = K.corrupt(c, way)
    assert made is not None, "seed %d has no cell to corrupt by way of %s" % (seed, way)
    adv, want = made
    assert any(e[0] == {"gate": W.GATE, "lookup": W.LOOKUP, "copy": W.COPY}[way] for e in want)
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert dev.report(advice=adv) == want
    assert dev.report() == []
    dev.free()


def test_the_corrupted_random_circuits_cover_every_kind(plonk):
    """At least 40 random circuits, and per way of corrupting at least 10 CASES, each with a reference entry of the way's
    kind (so at least 10 gate, 10 lookup and 10 copy failures in the reference's reports)."""
    t = K.tallies(plonk)
    assert len(K.RANDOM_SEEDS) >= 40
    for way in K.WAYS:
        cases, entries = t[way]
        assert cases >= 10 and entries >= cases, (way, t)


# ---------------------------------------------------------------------------------------------- row edges
def test_row_edges_and_rotations_that_wrap(ctx, plonk, oracle, srs):
    """q * (b - (a(-1) + a(+1))): row 0 reads row n - 1 and row u - 1 reads row u, which hold non-zero junk. The gate is
    violated at every row >= u of the fixture and that is not reported; a failing row u - 1 is, a failing row 0 is."""
    c = K.edge_circuit(plonk, 5)
    n, u = c.n, c.usable
    assert all(W.Walk(c).gate_fails_at(0, row) for row in range(u, n)) and c.advice[c.a][n - 1] and c.advice[c.a][u]
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert check_equal(dev) == []
    assert check_equal(dev, advice=K.with_cell(c, c.b, u - 1, 5)) == [(W.GATE, 0, u - 1, 1)]
    assert check_equal(dev, advice=K.with_cell(c, c.b, u, 5)) == []
    # the junk cells matter: row n - 1 is read by row 0 alone (and row n - 2, not usable), row u by row u - 1 (and u + 1)
    assert check_equal(dev, advice=K.with_cell(c, c.a, n - 1, 5)) == [(W.GATE, 0, 0, 1)]
    assert check_equal(dev, advice=K.with_cell(c, c.a, u, 5)) == [(W.GATE, 0, u - 1, 1)]
    dev.free()


@pytest.mark.parametrize("k", [7, 8])
def test_failures_on_both_sides_of_a_block_boundary(ctx, plonk, oracle, srs, k):
    """Rows 127 and 128: the last row of the interpreter's first 128-thread block and the first of its second. k = 8: the
    gate fails at both and both are counted; column d's copies fail at both. k = 7: row 128 does not exist and row 127 is
    not usable — the violated gate there is not reported, the broken copy constraint is (copies run over all n rows)."""
    c = K.edge_circuit(plonk, k, seed=k)
    a_col, d_col = (W.COPY, 0), (W.COPY, 1)  # positions of a and d among the permutation's columns
    adv = K.with_cell(c, c.b, 127, 5)
    adv[c.d][127] = 7
    if k == 8:
        adv[c.b][128] = 6
        adv[c.d][128] = 8
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert check_equal(dev) == []
    got = check_equal(dev, advice=adv)
    if k == 8:
        assert got == [(W.GATE, 0, 127, 2), a_col + (3, 2), d_col + (127, 2)]
        assert check_equal(dev, advice=K.with_cell(c, c.b, 128, 6)) == [(W.GATE, 0, 128, 1)]
        assert check_equal(dev, advice=K.with_cell(c, c.d, 128, 6)) == [a_col + (4, 1), d_col + (128, 1)]
    else:
        assert got == [a_col + (3, 1), d_col + (127, 1)]
        assert check_equal(dev, advice=K.with_cell(c, c.b, c.usable - 1, 6)) == [(W.GATE, 0, c.usable - 1, 1)]
    dev.free()


# ---------------------------------------------------------------------------------------------- lookup semantics
@pytest.mark.parametrize("k", [5, 12])
def test_lookup_semantics(ctx, plonk, oracle, srs, k):
    """Lookup 0 has a constant table (sorted at keygen), lookup 1 two expressions (theta), lookup 2 a table that is part
    of the witness. k = 12: the tables' sort takes its global passes (4096 keys, tiles of 2048)."""
    c = K.lookup_edge_circuit(plonk, k)
    u = c.usable
    dev = Dev(ctx, plonk, oracle, srs, c)
    assert check_equal(dev) == []
    # 777 is in t1 (and w) only at rows >= u: not a table value
    assert check_equal(dev, advice=K.with_cell(c, c.x, 3, 777)) == [(W.LOOKUP, 0, 3, 1), (W.LOOKUP, 1, 3, 1), (W.LOOKUP, 2, 3, 1)]
    # each component occurs in its table column, the pair never does
    adv = K.with_cell(c, c.x, 4, c.fixed[0][1])
    adv[c.y][4] = c.fixed[1][2]
    assert check_equal(dev, advice=adv) == [(W.LOOKUP, 1, 4, 1)]
    assert check_equal(dev, advice=adv, theta_seed=12345) == [(W.LOOKUP, 1, 4, 1)]
    # the witness-dependent table: take value 5 out of w everywhere, every x = 5 row fails lookup 2 alone
    adv = [list(a) for a in c.advice]
    adv[c.w] = [6 if v == 5 else v for v in adv[c.w]]
    got = check_equal(dev, advice=adv)
    assert [e[:2] for e in got] == [(W.LOOKUP, 2)] and got[0][3] == sum(1 for r in range(u) if c.advice[c.x][r] == 5) > 0
    # the last usable row and the row behind it
    assert check_equal(dev, advice=K.with_cell(c, c.x, u - 1, R - 1)) == [(W.LOOKUP, l, u - 1, 1) for l in range(3)]
    assert check_equal(dev, advice=K.with_cell(c, c.x, u, R - 1)) == []
    dev.free()


# ---------------------------------------------------------------------------------------------- key origins
def bad_lookup_circuit_witness(c):
    """One cell of each kind of trouble: a mul gate's output, a range-lookup input, a copied cell."""
    adv = K.with_cell(c, 2, 0, c.advice[2][0] + 1)
    q_rng = c.desc["lookups"][0]["inputs"][0][1]
    row = next(r for r in range(3, c.usable) if c.fixed[q_rng[1]][r] == 1)
    adv[0][row] = 1000
    adv[2][1] = (adv[2][1] + 1) % R  # c(1) is copied to the instance column
    return adv


def test_keys_of_every_origin_give_the_same_reports(ctx, pkg, plonk, oracle, srs):
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    dev = Dev(ctx, plonk, oracle, srs, c)
    bad = bad_lookup_circuit_witness(c)
    want = W.report(c, advice=bad)
    assert {e[0] for e in want} == {W.GATE, W.LOOKUP, W.COPY}
    sigma = dev.pk.export(1)
    keys = {"keygen": dev.pk,
            "sigma": plonk.ProvingKey.from_sigma(ctx, dev.params, c.desc, dev.fixed, sigma, zu.fr_from_int(REPR)),
            "read": plonk.ProvingKey.read(ctx, dev.params, dev.pk.write())}
    keys["clone"] = keys["read"].clone_workspace()  # the clone checks first: it decodes its root's sigma columns
    for name in ("clone", "read", "sigma", "keygen"):
        assert dev.report(pk=keys[name]) == [], name
        assert dev.report(pk=keys[name], advice=bad) == want, name
    # one junk sigma value: the key is made (keygen_sigma takes its input on trust), the check names the cell
    junk = sigma.copy()
    junk[1, 3] = zu.fr_from_int(0xDEADBEEF12345)
    jk = plonk.ProvingKey.from_sigma(ctx, dev.params, c.desc, dev.fixed, junk, zu.fr_from_int(REPR))
    for _ in range(2):
        with pytest.raises(pkg.AmdzkError, match=r"check_witness: sigma column 1 row 3 ") as e:
            dev.report(pk=jk)
        assert e.value.code == -2
    assert dev.report(advice=bad) == want  # the ctx is usable
    jk.free()
    keys["clone"].free(); keys["read"].free(); keys["sigma"].free()
    dev.free()


def test_clones_outlive_the_handle_keygen_returned(ctx, pkg, plonk, oracle, srs):
    """Keygen, two clones, and the handle keygen returned is freed first: each clone proves the oracle's bytes for its seed
    (k = 5 with a constant table, whose compressed column a clone copies, a permutation and both lookup kinds), and a
    clone's check of the witness — the first check on any handle of this key, so the sigma columns are decoded after the
    original handle is gone — reports nothing."""
    import plonk_ref as PR

    c = circuits.lookup_circuit(plonk, 5, seed=2)
    dev = Dev(ctx, plonk, oracle, srs, c)
    clones = [dev.pk.clone_workspace(), dev.pk.clone_workspace()]
    dev.pk.free()
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    d_adv, inst = dev.upload(), fr_inst(oracle, c.instances)
    for clone, seed in zip(clones, (41, 42)):
        assert plonk.create_proof(ctx, clone, inst, d_adv, seed=seed) == PR.create_proof(opk, c.instances, c.advice, seed=seed)
    assert dev.report(pk=clones[1]) == []
    for clone in clones:
        clone.free()
    dev.free()


# ---------------------------------------------------------------------------------------------- phased keys
@pytest.mark.parametrize("name", ["rlc", "rlc-three", "random-0", "random-1"])
def test_phased_keys_take_the_callers_challenges(ctx, pkg, plonk, oracle, name):
    from test_gpu_phased import Device

    c = {"rlc": lambda: PC.rlc_circuit(plonk, 5, seed=5), "rlc-three": lambda: PC.rlc_circuit(plonk, 5, seed=5, three_phases=True),
         "random-0": lambda: PC.random_phased_circuit(plonk, 5, seed=0), "random-1": lambda: PC.random_phased_circuit(plonk, 5, seed=1)}[name]()
    dev = Device(ctx, pkg, plonk, oracle, c)
    try:
        dev.prove(seed=11)
        ch = dev.challenges()
        assert ch and len(ch) == len(c.desc["challenge_phase"])
        adv, inst = dev.adv[0], dev.inst[0]
        check = lambda vals, **kw: [tuple(f) for f in plonk.check_witness(ctx, dev.pk, inst, dev.d_adv[0], challenges=None if vals is None else
                                                                             np.stack([zu.fr_from_int(v) for v in vals]), **kw).failures]
        assert check(ch) == [] == W.report(c, advice=adv, challenges=ch)
        other = [(v + 1) % R for v in ch]
        want = W.report(c, advice=adv, challenges=other)
        assert want and check(other) == want
        for vals in (None, ch + [1], ch[:-1] if len(ch) > 1 else ch + [1, 2]):
            with pytest.raises(pkg.AmdzkError, match="check_witness: .*challenges") as e:
                check(vals)
            assert e.value.code == -2
        assert check(ch) == []
    finally:
        dev.free()


# ---------------------------------------------------------------------------------------------- interface
def raw_call(ctx, pk, inst, d_adv, n, out, cap, total, opts=None):
    cols = [np.ascontiguousarray(col, dtype=np.uint64).reshape(-1, 4) for col in inst]
    ptrs = (C.c_void_p * max(1, len(cols)))(*[col.ctypes.data if col.size else None for col in cols])
    lens = (C.c_size_t * max(1, len(cols)))(*[col.shape[0] for col in cols])
    return ctx.L.amdzk_check_witness(ctx.h, pk, ptrs, lens, d_adv, n, opts, out, cap, total)


def test_count_query_cap_and_refusals(ctx, pkg, plonk, oracle, srs):
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    dev = Dev(ctx, plonk, oracle, srs, c)
    bad = bad_lookup_circuit_witness(c)
    want = W.report(c, advice=bad)
    assert len(want) >= 4
    inst = fr_inst(oracle, c.instances)
    d_adv = dev.upload(bad)
    total = C.c_size_t(77)
    # out = NULL: the count alone; opts = NULL: the defaults
    assert raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, None, 0, C.byref(total)) == 0 and total.value == len(want)
    assert raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, None, 5, C.byref(total)) == 0 and total.value == len(want)
    # cap below the count: cap entries (the first ones), the full count, nothing written behind them
    buf = (pkg.ffi.CheckFailure * len(want))()
    for f in buf:
        f.kind = f.reserved = 0xAAAA
    assert raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, buf, 2, C.byref(total)) == 0 and total.value == len(want)
    assert [(f.kind, f.index, f.first_row, f.count) for f in buf[:2]] == want[:2] and all(f.reserved == 0 for f in buf[:2])
    assert all(f.kind == 0xAAAA and f.reserved == 0xAAAA for f in buf[2:])
    assert raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, buf, len(want), C.byref(total)) == 0
    assert [(f.kind, f.index, f.first_row, f.count) for f in buf] == want

    def refused(rc, pattern):
        msg = ctx.L.amdzk_last_error(ctx.h).decode()
        assert rc == -2 and msg.startswith("check_witness:") and pattern in msg, (rc, msg)
        assert dev.report(advice=bad) == want  # the ctx and the key stay usable
        dev.upload(bad)

    refused(raw_call(ctx, None, inst, d_adv.ptr, c.n, None, 0, C.byref(total)), "null argument")
    refused(raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, None, 0, None), "null argument")
    refused(raw_call(ctx, dev.pk.h, inst, None, c.n, None, 0, C.byref(total)), "null argument")
    long_inst = [zu.ints_to_fr(oracle, [1] * (c.usable + 1))]
    refused(raw_call(ctx, dev.pk.h, long_inst, d_adv.ptr, c.n, None, 0, C.byref(total)), "instance column 0 too long (InstanceTooLarge)")
    lens_only = (C.c_size_t * 1)(2)
    assert ctx.L.amdzk_check_witness(ctx.h, dev.pk.h, None, lens_only, d_adv.ptr, c.n, None, None, 0, C.byref(total)) == -2
    refused(-2, "null argument")
    small = pkg.ffi.CheckOpts(C.sizeof(pkg.ffi.CheckOpts) - 8, 0, None, 0)
    refused(raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, None, 0, C.byref(total), C.byref(small)), "amdzk_check_opts.size")
    one = zu.fr_from_int(5).reshape(1, 4)
    extra = pkg.ffi.CheckOpts(C.sizeof(pkg.ffi.CheckOpts), 0, one.ctypes.data, 1)
    refused(raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n, None, 0, C.byref(total), C.byref(extra)), "challenges")
    # an instance column of exactly u values is accepted, and a shorter stride than n is not
    full = [zu.ints_to_fr(oracle, list(c.instances[0]) + [0] * (c.usable - len(c.instances[0])))]
    assert raw_call(ctx, dev.pk.h, full, d_adv.ptr, c.n, None, 0, C.byref(total)) == 0 and total.value == len(want)
    refused(raw_call(ctx, dev.pk.h, inst, d_adv.ptr, c.n - 1, None, 0, C.byref(total)), "stride")
    dev.free()


def test_advice_stride(ctx, plonk, oracle, srs):
    """Columns n + 5 apart, junk between them."""
    c = circuits.lookup_circuit(plonk, 5, seed=2)
    dev = Dev(ctx, plonk, oracle, srs, c)
    bad = bad_lookup_circuit_witness(c)
    stride = c.n + 5
    host = np.full((len(bad), stride, 4), 0x1234, np.uint64)
    host[:, :c.n] = fr_cols(oracle, bad, c.n)
    d = ctx.alloc(host.nbytes).upload(host)
    rep = plonk.check_witness(ctx, dev.pk, fr_inst(oracle, c.instances), d, advice_stride=stride)
    assert [tuple(f) for f in rep.failures] == W.report(c, advice=bad)
    d.free()
    dev.free()


# ---------------------------------------------------------------------------------------------- non-interference
def test_checks_between_proofs_change_no_proof(ctx, plonk, oracle, srs):
    import plonk_ref as PR

    c = circuits.lookup_circuit(plonk, 5, seed=2)
    dev = Dev(ctx, plonk, oracle, srs, c)
    inst = fr_inst(oracle, c.instances)
    good = ctx.alloc(len(c.advice) * c.n * 32).upload(fr_cols(oracle, c.advice, c.n))
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
    want = PR.create_proof(opk, c.instances, c.advice, seed=3)
    first = plonk.create_proof(ctx, dev.pk, inst, good, seed=3)
    assert plonk.check_witness(ctx, dev.pk, inst, good).ok
    second = plonk.create_proof(ctx, dev.pk, inst, good, seed=3)
    bad = bad_lookup_circuit_witness(c)
    assert dev.report(advice=bad) == W.report(c, advice=bad) != []
    third = plonk.create_proof(ctx, dev.pk, inst, good, seed=3)
    assert first == second == third == want
    good.free()
    dev.free()


# ---------------------------------------------------------------------------------------------- the metric shape
def test_metric_shape_k15(ctx, pkg, plonk, oracle, srs):
    """full_aadhaar_shape at k = 15 (141 advice columns, 24 lookups, 118 permutation columns): the satisfied witness
    gives an empty report; with one advice cell corrupted the report is not empty, and the reference evaluator confirms
    every reported gate and lookup at its first_row and every reported copy entry's cell against its sigma-image. (The
    full Python walk is too slow at this size: the reason the check exists.)"""
    c = circuits.full_aadhaar_shape(plonk, k=15)
    n = c.n
    wl = pkg.workloads
    fixed = oracle.fr_from_raw(np.ascontiguousarray(wl.canon_limbs(c.fixed)).reshape(-1, 4)).reshape(len(c.fixed), n, 4)
    pk = plonk.ProvingKey(ctx, srs(15), c.desc, fixed, c.assembly.mapping, zu.fr_from_int(REPR))
    adv = np.ascontiguousarray(wl.canon_limbs(c.advice))
    d_adv = ctx.alloc(adv.nbytes).upload(adv)
    ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, d_adv.ptr, len(c.advice) * n))
    inst = fr_inst(oracle, c.instances)
    assert plonk.check_witness(ctx, pk, inst, d_adv).ok

    def poke(col, row, value):
        v = np.ascontiguousarray(zu.fr_from_int(value % R))
        ctx._chk(ctx.L.amdzk_dev_upload(ctx.h, C.c_void_p(d_adv.ptr.value + (col * n + row) * 32), v.ctypes.data, 32))

    def confirmed(advice, rep):
        walk = W.Walk(c, advice=advice)
        for f in rep.failures:
            assert f.count >= 1 and f.first_row < (n if f.kind == W.COPY else c.usable)
            if f.kind == W.GATE:
                assert walk.gate_fails_at(f.index, f.first_row), f
            elif f.kind == W.LOOKUP:
                assert walk.lookup_fails_at(f.index, f.first_row), f
            else:
                assert walk.copy_fails_at(f.index, f.first_row), f

    # an input cell of a gate that is also one end of a copy constraint: the first advice <-> advice copy of the layout
    i1, r1, i2, r2 = c.copies[0]
    pcols = W.Walk(c).perm_columns()
    assert pcols[i2][0] == 0 and pcols[i1][0] == 0
    col = pcols[i2][1]
    advice = [a if j != col else list(a) for j, a in enumerate(c.advice)]
    advice[col][r2] = (advice[col][r2] + 1) % R
    poke(col, r2, advice[col][r2])
    rep = plonk.check_witness(ctx, pk, inst, d_adv)
    kinds = {f.kind for f in rep.failures}
    assert not rep.ok and W.GATE in kinds and W.COPY in kinds
    assert {(f.index, f.first_row) for f in rep.failures if f.kind == W.COPY} >= {(i2, r2)} or i1 == i2
    confirmed(advice, rep)
    poke(col, r2, c.advice[col][r2])
    # ... and a range-checked cell pushed out of its table
    lcol = next(e for e in c.desc["lookups"][0]["inputs"])[1]
    advice = [a if j != lcol else list(a) for j, a in enumerate(c.advice)]
    advice[lcol][100] = 1 << 20
    poke(lcol, 100, advice[lcol][100])
    rep = plonk.check_witness(ctx, pk, inst, d_adv)
    assert (W.LOOKUP, 0, 100, 1) in [tuple(f) for f in rep.failures]
    confirmed(advice, rep)
    poke(lcol, 100, c.advice[lcol][100])
    assert plonk.check_witness(ctx, pk, inst, d_adv).ok
    d_adv.free()
    pk.free()
