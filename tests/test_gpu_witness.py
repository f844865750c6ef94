"""GPU: witness programs on the device (amdzk_witness_compile / _run / _run_dev) against tests/witness_ref.py. In every
program here every node is also a public, so every node of every proof is compared — exact equality of canonical values.
Groups: the op edges; the launch geometry (level widths around the fused width, batch sizes around the wavefront, a
3000-level chain in one fused launch, fused and per-level launches alternating, operands 1, 2 and many levels back); runs
(a bounded workspace cuts the batch, results equal word for word); cells (scatter, stride, sentinel, zero fill); the _dev
form and the refusals of a run."""
import ctypes as C
import random

import numpy as np
import pytest

import witness_cases as WC
import witness_ref as WR

pytestmark = pytest.mark.gpu
E_INVALID = -2
R = WR.R
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def W(pkg):
    return pkg.witness.WitnessProgram


class Bufs:
    """One d_advice buffer per proof, num_advice x stride Fr, filled with the sentinel byte."""

    def __init__(self, ctx, n_proofs, num_advice, stride):
        self.ctx, self.shape = ctx, (num_advice, stride, 4)
        self.nbytes = max(32, num_advice * stride * 32)
        self.d = [ctx.alloc(self.nbytes) for _ in range(n_proofs)]
        self.fill()

    def fill(self):
        for d in self.d:
            self.ctx._chk(self.ctx.L.amdzk_dev_memset(self.ctx.h, d.ptr, SENTINEL, self.nbytes))

    def get(self, b):
        return self.d[b].download(self.shape)

    def free(self):
        for d in self.d:
            d.free()


def sentinel_words(shape):
    return np.full(shape, int.from_bytes(bytes([SENTINEL]) * 8, "little"), dtype=np.uint64)


def run_host(ctx, cw, prog, inputs, bufs=None, **kw):
    own = bufs is None
    if own:
        bufs = Bufs(ctx, len(inputs), prog.num_advice, 1 << prog.k)
    try:
        return cw.run([WR.to_words(row) for row in inputs], bufs.d[:len(inputs)], **kw)
    finally:
        if own:
            bufs.free()


def reference_words(prog, inputs):
    """(n_proofs, n_nodes, 4) Montgomery words of every node."""
    return np.stack([WR.to_words(WR.evaluate(prog, row)) for row in inputs])


def check_all_nodes(ctx, prog, inputs, want=None, **kw):
    """Compile prog with every node exposed, run it, compare every node of every proof. Returns the publics."""
    assert len(prog.publics) == len(prog.nodes)
    cw = prog.compile(ctx)
    try:
        got = run_host(ctx, cw, prog, inputs, **kw)
    finally:
        cw.free()
    want = reference_words(prog, inputs) if want is None else want
    if not np.array_equal(got, want):
        b, i = np.argwhere((got != want).any(axis=2))[0]
        raise AssertionError("proof %d node %d %s%r: got %r, want %r" % (b, i, WR.OP_NAMES[prog.nodes[i][0]], prog.nodes[i][1:], got[b, i], want[b, i]))
    return got


# ---- op edges
def test_op_edges_across_a_batch_of_edge_operands(ctx, W):
    prog, pairs = WC.edge_program(W)
    WC.expose_all(prog)
    check_all_nodes(ctx, prog, pairs)


@pytest.mark.parametrize("seed", [0, 1])
def test_random_programs_over_all_ops(ctx, W, seed):
    rng = random.Random(4200 + seed)
    prog = WC.expose_all(WC.random_program(W, rng, n_nodes=500, n_inputs=8, near=(0.8, 0.3)[seed], recent=0.2))
    assert {n[0] for n in prog.nodes} == set(range(14))
    check_all_nodes(ctx, prog, WC.random_inputs(rng, 13, 8))


def test_bits_every_shift_and_every_mask(ctx, W):
    prog = W(3, 1)
    a = prog.input()
    for lo in range(256):
        prog.bits(a, lo, 256 - lo)
        prog.bits(a, lo, 1)
    for ln in range(1, 257):
        prog.bits(a, 0, ln)
    WC.expose_all(prog)
    check_all_nodes(ctx, prog, [[R - 1], [R - 2], [0x2AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA], [1]])


# ---- geometry
@pytest.fixture(scope="module")
def fused_width(W):
    return W(4, 1).plan(1)["fused_width"]


@pytest.mark.parametrize("n_proofs", [1, 3])
def test_level_widths_around_the_fused_width(ctx, W, fused_width, n_proofs):
    fw = fused_width
    widths = [1, 63, 64, 65, fw - 1, fw, fw + 1, 4 * fw + 3]
    prog = WC.expose_all(WC.widths_program(W, widths))
    assert WR.level_widths(prog.nodes)[1:1 + len(widths)] == widths
    rng = random.Random(5)
    assert prog.plan(n_proofs)["launches"] == WR.launches(prog, [n_proofs], fw)
    check_all_nodes(ctx, prog, WC.random_inputs(rng, n_proofs, 2))


@pytest.fixture(scope="module")
def batch_case(W):
    prog = WC.expose_all(WC.widths_program(W, [1, 7, 63, 64, 65, 16, 1, 1, 200, 2]))
    inputs = WC.random_inputs(random.Random(6), 65, 2)
    return prog, inputs, reference_words(prog, inputs)


@pytest.mark.parametrize("n_proofs", [1, 2, 3, 64, 65])
def test_batch_sizes_around_the_wavefront(ctx, batch_case, n_proofs):
    prog, inputs, want = batch_case
    check_all_nodes(ctx, prog, inputs[:n_proofs], want=want[:n_proofs])


def test_a_3000_level_chain_is_one_fused_launch(ctx, W):
    prog = WC.expose_all(WC.chain_program(W, 3000))
    pl = prog.plan(3)
    assert pl["levels"] == 3001 and pl["launches"] == 2, "one single-workgroup launch for all levels, and the gather"
    check_all_nodes(ctx, prog, [[3, 5], [R - 1, R - 2], [0x123456789ABCDEF, 1 << 200]])


def test_fused_and_per_level_launches_alternate_twenty_times(ctx, W, fused_width):
    widths = [1, fused_width + 1] * 20
    prog = WC.expose_all(WC.widths_program(W, widths))
    assert prog.plan(1)["launches"] == 1 + 2 * 20 + 1  # the leaves fuse with the first narrow level; the last stretch; the gather
    check_all_nodes(ctx, prog, [[7, 11]])
    # and with the narrow levels two wide: at 3 proofs a narrow level is 6 items, a wide one 3 * (fw + 1)
    check_all_nodes(ctx, prog, WC.random_inputs(random.Random(8), 3, 2))


def test_operands_one_two_and_many_levels_back(ctx, W):
    prog = W(4, 1)
    x = prog.input()
    chain = [x]
    for i in range(40):
        chain.append(prog.add(chain[-1], x))
    prog.select(chain[-1], chain[-2], chain[1])
    prog.add(prog.mul(chain[-1], chain[-3]), chain[0])
    WC.expose_all(prog)
    check_all_nodes(ctx, prog, [[1], [0], [R - 1]])


# ---- runs
def test_a_bounded_workspace_cuts_the_batch_and_changes_nothing(ctx, W, pkg):
    rng = random.Random(9)
    prog = WC.expose_all(WC.random_program(W, rng, n_nodes=300, n_inputs=4))
    for j, i in enumerate(rng.sample(range(len(prog.nodes)), 10)):
        prog.assign(i, j % 3, j)
    inputs = WC.random_inputs(rng, 5, 4)
    per_proof = (len(prog.nodes) + len(prog.publics)) * 32
    cw = prog.compile(ctx)
    results, runs = [], []
    for bound in (0, 2 * per_proof + 256, 3 * per_proof + 255, per_proof + 256):  # one run; 2 + 2 + 1 twice; each proof its own
        bufs = Bufs(ctx, 5, prog.num_advice, 1 << prog.k)
        ctx.prof_enable(True)
        ctx.prof_reset()
        pub = run_host(ctx, cw, prog, inputs, bufs=bufs, max_scratch_bytes=bound)
        runs.append(ctx.prof_dump()["wit_gather"][0])  # one gather per run
        ctx.prof_enable(False)
        results.append((pub, [bufs.get(b) for b in range(5)]))
        bufs.free()
    assert runs == [1, 3, 3, 5]
    assert WR.run_cut(5, 2) == [2, 2, 1] and WR.run_cut(5, 1) == [1] * 5
    assert np.array_equal(results[0][0], reference_words(prog, inputs))
    for pub, adv in results[1:]:
        assert np.array_equal(pub, results[0][0])
        for b in range(5):
            assert np.array_equal(adv[b], results[0][1][b])
    # a bound below one proof's workspace is refused
    bufs = Bufs(ctx, 5, prog.num_advice, 1 << prog.k)
    with pytest.raises(pkg.AmdzkError) as e:
        run_host(ctx, cw, prog, inputs, bufs=bufs, max_scratch_bytes=per_proof + 255)
    assert e.value.code == E_INVALID and "witness:" in str(e.value)
    assert all(np.array_equal(bufs.get(b), sentinel_words(bufs.shape)) for b in range(5))
    bufs.free()
    cw.free()


# ---- cells
def test_cells_stride_sentinel_and_zero_fill(ctx, W, pkg):
    k, ncol, stride = 4, 3, 20
    n = 1 << k
    prog = W(k, ncol)
    a, b = prog.input(), prog.input()
    s, m, d = prog.add(a, b), prog.mul(a, b), prog.sub(a, b)
    placed = {(0, 0): s, (0, n - 1): m, (ncol - 1, 0): d, (ncol - 1, n - 1): a, (1, 7): m}
    for (col, row), node in placed.items():
        prog.assign(node, col, row)
    WC.expose_all(prog)
    inputs = [[3, 4], [R - 1, 2], [0, 0]]
    want = reference_words(prog, inputs)
    cw = prog.compile(ctx)
    bufs = Bufs(ctx, 3, ncol, stride)
    sent = sentinel_words((4,))
    for flags in (0, pkg.witness.ZERO_FILL):
        bufs.fill()
        cw.run([WR.to_words(row) for row in inputs], bufs.d, advice_stride=stride, flags=flags)
        for p in range(3):
            adv = bufs.get(p)
            for col in range(ncol):
                for row in range(stride):
                    if (col, row) in placed:
                        assert np.array_equal(adv[col, row], want[p, placed[(col, row)]]), (flags, p, col, row)
                    elif row < n and flags:
                        assert not adv[col, row].any(), "zero-filled"
                    else:
                        assert np.array_equal(adv[col, row], sent), "an unnamed cell without ZERO_FILL, or the padding between columns"
    bufs.free()
    cw.free()


# ---- the _dev form and the refusals of a run
def test_dev_form_equals_host_form_and_refuses_a_resident_input_above_the_modulus(ctx, W, pkg):
    rng = random.Random(10)
    prog = WC.expose_all(WC.random_program(W, rng, n_nodes=200, n_inputs=5))
    prog.assign(len(prog.nodes) - 1, 2, 3)
    inputs = WC.random_inputs(rng, 4, 5)
    cw = prog.compile(ctx)
    bufs = Bufs(ctx, 4, prog.num_advice, 1 << prog.k)
    host = run_host(ctx, cw, prog, inputs, bufs=bufs)
    host_adv = [bufs.get(b) for b in range(4)]
    in_stride = 7  # > n_inputs
    words = np.zeros((4, in_stride, 4), dtype=np.uint64)
    for b, row in enumerate(inputs):
        words[b, :5] = WR.to_words(row)
    d_in = ctx.alloc(words.nbytes).upload(words)
    bufs.fill()
    dev = cw.run_dev(d_in, in_stride, bufs.d)
    assert np.array_equal(dev, host) and np.array_equal(host, reference_words(prog, inputs))
    assert all(np.array_equal(bufs.get(b), host_adv[b]) for b in range(4))
    # one resident input >= r: refused by the check launch, nothing written anywhere
    for bad in (R, (1 << 256) - 1):
        words2 = words.copy()
        words2[2, 3] = WR.raw_words([bad])[0]
        d_in.upload(words2)
        bufs.fill()
        with pytest.raises(pkg.AmdzkError) as e:
            cw.run_dev(d_in, in_stride, bufs.d, flags=pkg.witness.ZERO_FILL)
        assert e.value.code == E_INVALID and "witness: input 3 of proof 2" in str(e.value)
        assert all(np.array_equal(bufs.get(b), sentinel_words(bufs.shape)) for b in range(4))
    # the padding of the input rows is not checked: it is not an input
    words2 = words.copy()
    words2[1, 6] = WR.raw_words([(1 << 256) - 1])[0]
    d_in.upload(words2)
    assert np.array_equal(cw.run_dev(d_in, in_stride, bufs.d), host)
    d_in.free()
    bufs.free()
    cw.free()


def test_refusals_of_a_run_leave_the_buffers_and_the_ctx_alone(ctx, W, pkg):
    prog = W(4, 2)
    a, b = prog.input(), prog.input()
    s = prog.add(a, b)
    prog.assign(s, 0, 0)
    prog.expose(s)
    cw = prog.compile(ctx)
    bufs = Bufs(ctx, 3, 2, 16)
    good = [WR.to_words([1, 2])] * 3
    L = ctx.L

    def refused(call, code=E_INVALID):
        with pytest.raises(pkg.AmdzkError) as e:
            call()
        assert e.value.code == code and "witness:" in str(e.value), str(e.value)
        assert all(np.array_equal(bufs.get(i), sentinel_words(bufs.shape)) for i in range(3))

    refused(lambda: cw.run([WR.to_words([1, 2]), WR.raw_words([R, 2]), WR.to_words([1, 2])], bufs.d, flags=1))  # an input >= r, host form
    refused(lambda: cw.run(good, [bufs.d[0], bufs.d[1], bufs.d[0]]))  # the same buffer twice
    refused(lambda: cw.run(good, [bufs.d[0], None, bufs.d[2]]))
    refused(lambda: cw.run([], []))  # n_proofs = 0
    refused(lambda: cw.run(good, bufs.d, advice_stride=15))
    refused(lambda: cw.run(good, bufs.d, flags=2))
    adv = (C.c_void_p * 3)(*[d.ptr for d in bufs.d])
    ins = (C.c_void_p * 3)(*[g.ctypes.data for g in good])
    # null program, null inputs (the program has inputs), a null inputs[b], null d_advice
    for w, i, ad in ((None, ins, adv), (cw.h, None, adv), (cw.h, (C.c_void_p * 3)(), adv), (cw.h, ins, None)):
        assert L.amdzk_witness_run(ctx.h, w, 3, i, ad, 16, 0, 0, None) == E_INVALID and L.amdzk_last_error(ctx.h).startswith(b"witness:")
    assert L.amdzk_witness_run_dev(ctx.h, cw.h, 3, None, 2, adv, 16, 0, 0, None) == E_INVALID
    assert L.amdzk_witness_compile(ctx.h, None, None) == E_INVALID and L.amdzk_last_error(ctx.h).startswith(b"witness:")
    assert L.amdzk_witness_run(None, cw.h, 3, None, adv, 16, 0, 0, None) == E_INVALID
    h = C.c_void_p()
    d, keep = prog.desc(size=8)
    assert L.amdzk_witness_compile(ctx.h, C.byref(d), C.byref(h)) == E_INVALID and not h.value
    # the ctx and the program are still usable
    out = cw.run(good, bufs.d)
    assert WR.from_words(out) == [3, 3, 3]
    assert WR.from_words(bufs.get(1)[0, 0]) == [3]
    bufs.free()
    cw.free()
