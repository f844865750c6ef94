"""GPU: Poseidon over Fr (csrc/poseidon.hip; include/amdzk.h "Poseidon over Fr") against tests/poseidon_ref.py, exactly.
Permutations: every t and round shape on every kind of constants, batches at the group, wavefront and block boundaries, a
stride with gaps. Sponges: rates, lengths at every chunk boundary, uniform and ragged, both initial states, the host form
against the resident form, digests into a larger buffer, the reference's own shape. permute_dev composed into a sponge.
Every refusal: status, message, buffers unchanged, the ctx usable."""
import ctypes as C

import numpy as np
import pytest

import poseidon_cases as PC
import poseidon_ref as PR

pytestmark = pytest.mark.gpu
R = PR.R
TS = (2, 3, 5, 6, 7, 8)
ROUNDS = ((2, 0), (2, 1), (8, 57))
BATCHES = (1, 7, 8, 9, 31, 32, 33, 65)  # a group is 8 lanes, a wavefront 8 groups, a block 32
SENTINEL = 0xA5A5A5A5A5A5A5A5


def rates(t):
    return sorted({1, t // 2, t - 1})


def lengths(rate):
    return sorted({0, 1, rate - 1, rate, rate + 1, 2 * rate, 37})


@pytest.fixture()
def compiled(pkg, ctx):
    made = []

    def make(spec):
        made.append(pkg.poseidon.Poseidon(ctx, PC.pkg_spec(pkg, spec)))
        return made[-1]
    yield make
    for p in made:
        p.free()


@pytest.fixture()
def dev(ctx):
    bufs = []

    def make(arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        bufs.append(ctx.alloc(max(arr.nbytes, 32)).upload(arr))
        return bufs[-1]
    yield make
    for b in bufs:
        b.free()


# ---------------------------------------------------------------------------------------------- permutation
@pytest.mark.parametrize("r_f,r_p", ROUNDS)
@pytest.mark.parametrize("t", TS)
def test_permutation_every_kind_of_constants_and_batch_size(compiled, dev, t, r_f, r_p):
    states = PC.states(t, max(BATCHES))  # words 0, 1, r - 1 and random
    words = np.stack([PC.to_words(s) for s in states])
    for kind in PC.KINDS:
        spec = PC.spec(t, 1, r_f, r_p, kind)
        want = np.stack([PC.to_words(PR.permute(spec, s)) for s in states])
        P = compiled(spec)
        for n in BATCHES:
            d = dev(words[:n])
            P.permute_many_dev(d, n)
            got = d.download((n, t, 4))
            assert np.array_equal(got, want[:n]), "t=%d (%d, %d) %s, %d states: first difference at state %d" % (
                t, r_f, r_p, kind, n, int(np.argmax((got != want[:n]).any(axis=(1, 2)))))


@pytest.mark.parametrize("t", (2, 5, 8))
def test_permutation_with_a_stride_leaves_the_gaps(compiled, dev, t):
    spec, n, stride = PC.spec(t, 1, 2, 1), 33, t + 3
    states = PC.states(t, n)
    buf = np.full((n + 2, stride, 4), SENTINEL, dtype=np.uint64)  # one stride of margin before and after
    for b, s in enumerate(states):
        buf[1 + b, :t] = PC.to_words(s)
    d = dev(buf)
    compiled(spec).permute_many_dev(d, n, stride, offset=stride)
    got = d.download(buf.shape)
    want = buf.copy()
    for b, s in enumerate(states):
        want[1 + b, :t] = PC.to_words(PR.permute(spec, s))
    assert np.array_equal(got, want)


def test_the_largest_spec_fills_the_round_constants_budget(compiled, dev):
    """(r_f + r_p) * t = 1536, the most a block's LDS is asked to hold; 33 states, so a second block reads them too."""
    t, n = 8, 33
    spec = PC.spec(t, 7, 2, 190, "cauchy")
    states = PC.states(t, n)
    d = dev(np.stack([PC.to_words(s) for s in states]))
    compiled(spec).permute_many_dev(d, n)
    assert np.array_equal(d.download((n, t, 4)), np.stack([PC.to_words(PR.permute(spec, s)) for s in states]))


def test_permute_many_over_numpy(compiled):
    spec = PC.spec(3, 2, 8, 57, "cauchy")
    states = PC.states(3, 10)
    got = compiled(spec).permute_many(np.stack([PC.to_words(s) for s in states]))
    assert [PC.from_words(g) for g in got] == [PR.permute(spec, s) for s in states]


# ---------------------------------------------------------------------------------------------- sponge
@pytest.mark.parametrize("init", (False, True), ids=("default-init", "given-init"))
@pytest.mark.parametrize("t", TS)
def test_sponge_rates_and_lengths_uniform_ragged_host_and_resident(compiled, dev, t, init):
    for rate in rates(t):
        spec = PC.spec(t, rate, 2, 1, "cauchy" if init else "random", init)
        P = compiled(spec)
        ls = lengths(rate)
        # ragged: every length five times over, rotated, so that 35 sponges of different lengths share wavefronts and blocks
        ragged = [ls[(i + i // len(ls)) % len(ls)] for i in range(5 * len(ls))]
        data = [PC.inputs(n, "gpu%d" % i, edge=True) for i, n in enumerate(ragged)]
        want = PC.to_words([PR.sponge(spec, x) for x in data])
        host = P.hash_many([PC.to_words(x) for x in data])
        assert np.array_equal(host, want), "host form, t=%d rate=%d" % (t, rate)
        stride = max(ragged) + 2
        table = np.full((len(data), stride, 4), SENTINEL, dtype=np.uint64)
        for b, x in enumerate(data):
            table[b, :len(x)] = PC.to_words(x)
        d_in, d_out = dev(table), dev(np.full((len(data), 4), SENTINEL, dtype=np.uint64))
        P.hash_many_dev(d_in, stride, len(data), d_out, lens=ragged)
        assert np.array_equal(d_out.download((len(data), 4)), host), "resident form against the host form, t=%d rate=%d" % (t, rate)
        assert np.array_equal(d_in.download(table.shape), table)
        # uniform: the sponges of one length in one call with lens = NULL
        for n in ls:
            rows = [b for b, x in enumerate(ragged) if x == n]
            uni = np.zeros((len(rows), max(n, 1), 4), dtype=np.uint64)
            for i, b in enumerate(rows):
                uni[i, :n] = PC.to_words(data[b])
            d_u, d_o = dev(uni), dev(np.zeros((len(rows), 4), dtype=np.uint64))
            P.hash_many_dev(d_u, max(n, 1), len(rows), d_o, length=n)
            assert np.array_equal(d_o.download((len(rows), 4)), want[rows]), "uniform length %d, t=%d rate=%d" % (n, t, rate)


def test_sponge_of_no_input_needs_no_input_buffer(compiled, dev):
    spec = PC.spec(3, 2, 2, 1)
    d_out = dev(np.zeros((9, 4), dtype=np.uint64))
    compiled(spec).hash_many_dev(None, 0, 9, d_out, length=0)
    assert np.array_equal(d_out.download((9, 4)), PC.to_words([PR.sponge(spec, [])] * 9))


def test_digests_with_an_output_stride_into_a_larger_buffer(compiled, dev):
    spec = PC.spec(5, 4, 2, 1)
    n, out_stride, at = 33, 3, 2
    data = [PC.inputs(6, "stride%d" % b) for b in range(n)]
    d_in = dev(np.stack([PC.to_words(x) for x in data]))
    out = np.full((at + n * out_stride + 5, 4), SENTINEL, dtype=np.uint64)
    d_out = dev(out)
    compiled(spec).hash_many_dev(d_in, 6, n, d_out, out_stride=out_stride, length=6, out_offset=at)
    want = out.copy()
    want[at:at + n * out_stride:out_stride] = PC.to_words([PR.sponge(spec, x) for x in data])
    assert np.array_equal(d_out.download(out.shape), want)


def test_the_reference_shape_and_update_squeeze(compiled, dev):
    """t = 5, rate = 4, (8, 57), 950 inputs below 256, two sponges: Poseidon::<Fr, 5, 4>::new(8, 57) over the nullifier's input."""
    spec = PC.spec(5, 4, 8, 57, "cauchy")
    data = [[v % 256 for v in PC.inputs(950, "bytes%d" % b)] for b in range(2)]
    want = [PR.sponge(spec, x) for x in data]
    P = compiled(spec)
    assert PC.from_words(P.hash_many([PC.to_words(x) for x in data])) == want
    d_in, d_out = dev(np.stack([PC.to_words(x) for x in data])), dev(np.zeros((2, 4), dtype=np.uint64))
    P.hash_many_dev(d_in, 950, 2, d_out, length=950)
    assert PC.from_words(d_out.download((2, 4))) == want
    assert P.update(data[0][:400]).update(data[0][400:]).squeeze() == want[0]
    assert P.update(data[1]).squeeze() == want[1], "squeeze starts the sponge afresh"


# ---------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("t,rate", [(3, 2), (5, 4), (8, 3)])
def test_permute_dev_driven_as_a_sponge_gives_hash_devs_digest(compiled, dev, t, rate):
    spec = PC.spec(t, rate, 8, 5, "cauchy", init=True)
    P = compiled(spec)
    data = [PC.inputs(n, "compose%d" % n) for n in (0, rate, 2 * rate + 1, 11)]
    digests = PC.from_words(P.hash_many([PC.to_words(x) for x in data]))
    for x, digest in zip(data, digests):
        d = dev(PC.to_words(spec.initial_state()))
        for chunk in PR.chunks(x, rate):
            s = PC.from_words(d.download((t, 4)))
            for i, v in enumerate(chunk):
                s[1 + i] = (s[1 + i] + v) % R
            d.upload(PC.to_words(s))
            P.permute_many_dev(d, 1)
        assert PC.from_words(d.download((t, 4)))[1] == digest


# ---------------------------------------------------------------------------------------------- refusals
def test_compile_refuses_every_bad_description(pkg, ctx, compiled):
    L = ctx.L
    for name, kw, code, needle in PC.DESC_REFUSALS:
        d, keep = PC.raw_desc(pkg, **kw)
        h = C.c_void_p(1)
        assert L.amdzk_poseidon_compile(ctx.h, C.byref(d), C.byref(h)) == code, name
        msg = L.amdzk_last_error(ctx.h).decode()
        assert msg.startswith("poseidon: ") and needle in msg and not h.value, (name, msg)
        del keep
    d, keep = PC.raw_desc(pkg)
    h = C.c_void_p()
    assert L.amdzk_poseidon_compile(ctx.h, None, C.byref(h)) == -2 and L.amdzk_last_error(ctx.h).decode().startswith("poseidon: null")
    assert L.amdzk_poseidon_compile(ctx.h, C.byref(d), None) == -2 and L.amdzk_last_error(ctx.h).decode().startswith("poseidon: null")
    L.amdzk_poseidon_free(ctx.h, None)  # a no-op
    spec = PC.spec(3, 2, 2, 1)
    assert PC.from_words(compiled(spec).hash_many([PC.to_words([5, 6, 7])])) == [PR.sponge(spec, [5, 6, 7])]


def test_calls_refuse_bad_arguments_and_leave_everything_as_it_was(pkg, ctx, compiled, dev):
    L = ctx.L
    t, rate, n = 5, 4, 6
    spec = PC.spec(t, rate, 2, 1)
    P = compiled(spec)
    states = np.stack([PC.to_words(s) for s in PC.states(t, n)])
    table = np.stack([PC.to_words(PC.inputs(9, "refuse%d" % b)) for b in range(n)])
    outs = np.full((n, 4), SENTINEL, dtype=np.uint64)
    d_states, d_in, d_out = dev(states), dev(table), dev(outs)
    host = np.zeros((64, 4), dtype=np.uint64)  # not device memory
    lens9 = (C.c_size_t * n)(*([9] * n))
    lens10 = (C.c_size_t * n)(*([9] * (n - 1) + [10]))
    big = 1 << 31
    in_ptrs = (C.c_void_p * n)(*[table[b].ctypes.data for b in range(n)])
    null_row = (C.c_void_p * n)(*([table[0].ctypes.data] * (n - 1) + [None]))
    bad = table.copy()
    bad[3, 4] = [(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    bad_ptrs = (C.c_void_p * n)(*[bad[b].ctypes.data for b in range(n)])
    host_out = np.full((n, 4), SENTINEL, dtype=np.uint64)
    sp, ip, op, hp = d_states.ptr, d_in.ptr, d_out.ptr, C.c_void_p(host.ctypes.data)
    INVALID, UNSUPPORTED = -2, -5
    cases = [
        ("permute: null handle", L.amdzk_poseidon_permute_dev, (ctx.h, None, sp, n, t), INVALID),
        ("permute: null states", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, None, n, t), INVALID),
        ("permute: n = 0", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, sp, 0, t), INVALID),
        ("permute: stride < t", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, sp, n, t - 1), INVALID),
        ("permute: host memory", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, hp, n, t), INVALID),
        ("permute: 2^31 states", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, sp, big, t), UNSUPPORTED),
        ("permute: bytes overflow", L.amdzk_poseidon_permute_dev, (ctx.h, P.h, sp, n, 1 << 60), UNSUPPORTED),
        ("hash_dev: null handle", L.amdzk_poseidon_hash_dev, (ctx.h, None, ip, 9, None, 9, n, op, 1), INVALID),
        ("hash_dev: null out", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, None, 9, n, None, 1), INVALID),
        ("hash_dev: null inputs", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, None, 9, None, 9, n, op, 1), INVALID),
        ("hash_dev: n = 0", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, None, 9, 0, op, 1), INVALID),
        ("hash_dev: stride < len", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 8, None, 9, n, op, 1), INVALID),
        ("hash_dev: stride < longest of lens", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, lens10, 0, n, op, 1), INVALID),
        ("hash_dev: out_stride = 0", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, None, 9, n, op, 0), INVALID),
        ("hash_dev: inputs in host memory", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, hp, 9, None, 9, n, op, 1), INVALID),
        ("hash_dev: out in host memory", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, None, 9, n, hp, 1), INVALID),
        ("hash_dev: 2^31 sponges", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 9, None, 9, big, op, 1), UNSUPPORTED),
        ("hash_dev: a length of 2^31", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, big, None, big, n, op, 1), UNSUPPORTED),
        ("hash_dev: bytes overflow", L.amdzk_poseidon_hash_dev, (ctx.h, P.h, ip, 1 << 60, None, 9, n, op, 1), UNSUPPORTED),
        ("hash: null handle", L.amdzk_poseidon_hash, (ctx.h, None, in_ptrs, lens9, n, host_out.ctypes.data), INVALID),
        ("hash: null inputs", L.amdzk_poseidon_hash, (ctx.h, P.h, None, lens9, n, host_out.ctypes.data), INVALID),
        ("hash: null lens", L.amdzk_poseidon_hash, (ctx.h, P.h, in_ptrs, None, n, host_out.ctypes.data), INVALID),
        ("hash: null out", L.amdzk_poseidon_hash, (ctx.h, P.h, in_ptrs, lens9, n, None), INVALID),
        ("hash: n = 0", L.amdzk_poseidon_hash, (ctx.h, P.h, in_ptrs, lens9, 0, host_out.ctypes.data), INVALID),
        ("hash: a null row", L.amdzk_poseidon_hash, (ctx.h, P.h, null_row, lens9, n, host_out.ctypes.data), INVALID),
        ("hash: an input >= r", L.amdzk_poseidon_hash, (ctx.h, P.h, bad_ptrs, lens9, n, host_out.ctypes.data), INVALID),
    ]
    want_states = np.stack([PC.to_words(PR.permute(spec, s)) for s in PC.states(t, n)])
    want_digests = PC.to_words([PR.sponge(spec, PC.inputs(9, "refuse%d" % b)) for b in range(n)])
    for name, fn, args, code in cases:
        assert fn(*args) == code, name
        msg = L.amdzk_last_error(ctx.h).decode()
        assert msg.startswith("poseidon:"), (name, msg)
        assert np.array_equal(d_states.download(states.shape), states), name
        assert np.array_equal(d_in.download(table.shape), table), name
        assert np.array_equal(d_out.download(outs.shape), outs) and (host_out == SENTINEL).all() and not host.any(), name
        # ... and a successful call on the same ctx
        P.hash_many_dev(d_in, 9, n, d_out, lens=[9] * n)
        assert np.array_equal(d_out.download(outs.shape), want_digests), name
        d_out.upload(outs)
    assert "input 4 of sponge 3" in msg
    P.permute_many_dev(d_states, n)
    assert np.array_equal(d_states.download(states.shape), want_states)
    assert np.array_equal(P.hash_many(list(table)), want_digests)
