"""GPU: the lookup argument's permutation (amdzk_permute_expression_pair_dev -> zk_sort_keys2 and zk_lookup_permute,
csrc/plonk_kernels.hip: bitonic_lds_kernel, bitonic_global_kernel, lookup_mark_kernel, flag_scan_kernel,
lookup_compact_kernel, lookup_assign_kernel) at edge keys, sizes and usable rows.

The cases, the orders of the input column and the reference are tests/lookup_permute_cases.py; its CPU test shows that
the reference agrees with the definition on every case run here. The calls go through the C entry point with buffers of
this file's own, so that the table buffer can be read back: inputs, tables and a poisoned output go up, A', S' and the
table come down, and everything is compared exactly (a mismatch names the first differing row). Rows at or beyond
`usable` hold r - 1 in the input and a value found nowhere else in the table: they must not matter and come back zero.

A Python copy of the launch rule (lookup_permute_cases.launch_plan) is asserted against the library's own launch counters
(Context.prof_dump) around every call: when the rule changes, a case fails instead of quietly testing something else."""
import contextlib
import functools
import re

import numpy as np
import pytest
import zkutil as zu

import lookup_permute_cases as LC

pytestmark = pytest.mark.gpu
R = zu.R
E_INVALID = -2  # AMDZK_E_INVALID
POISON = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # not below r: a value no kernel writes


# ------------------------------------------------------------------------------ device plumbing
@contextlib.contextmanager
def launches(ctx):
    """{kernel name: launches} of the sort's and the permutation's kernels launched inside the block."""
    got = {}
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        yield got
        got.update({name: cnt for name, (cnt, _) in ctx.prof_dump().items() if name.startswith(("sort_", "lookup_"))})
    finally:
        ctx.prof_enable(False)


class Buffers:
    """Input, table and output columns for up to `ncols` lookups of n rows."""

    def __init__(self, ctx, ncols, n):
        self.ctx, self.ncols, self.n = ctx, ncols, n
        self.inp, self.tab, self.out = (ctx.alloc(max(32, ncols * n * 32)) for _ in range(3))

    def free(self):
        self.inp.free(); self.tab.free(); self.out.free()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def call(ctx, bufs, inputs, tables, usable, n=None, nlookups=None):
    """One amdzk_permute_expression_pair_dev over the (L, n, 4) arrays `inputs` and `tables`; the output starts poisoned.
    Returns (A', S', the table buffer afterwards), raises AmdzkError on a refusal."""
    L, rows = inputs.shape[0], inputs.shape[1]
    assert tables.shape == inputs.shape and L <= bufs.ncols and rows == bufs.n
    bufs.inp.upload(inputs)
    bufs.tab.upload(tables)
    bufs.out.upload(np.tile(POISON, (L * rows, 1)))
    ctx._chk(ctx.L.amdzk_permute_expression_pair_dev(ctx.h, bufs.inp.ptr, bufs.tab.ptr, bufs.out.ptr, L if nlookups is None else nlookups,
                                                     rows if n is None else n, usable))
    return bufs.inp.download(inputs.shape), bufs.out.download(inputs.shape), bufs.tab.download(inputs.shape)


def same(got, want, what):
    if np.array_equal(got, want):
        return
    g, w = got.reshape(-1, 4), want.reshape(-1, 4)
    row = int(np.nonzero((g != w).any(axis=1))[0][0])
    word = lambda a: "%#x" % zu.from_limbs(a)  # the Montgomery word: a poisoned or unreduced row has no canonical value
    pytest.fail("%s: first mismatch at row %d of %d: got the word %s (canonical %#x), want %s (canonical %#x)"
                % (what, row, g.shape[0], word(g[row]), zu.fr_to_int(g[row]), word(w[row]), zu.fr_to_int(w[row])))


def column(oracle, vals, n, pad):
    return zu.ints_to_fr(oracle, list(vals) + [pad] * (n - len(vals)))


_prepared = {}


def prepared(oracle, n, u):
    """{case name: (input column in ascending order, table column, expected A', expected S')} as (n, 4) Montgomery arrays,
    for the cases over u usable rows of n. Made once per (n, u), shared by the tests below and never written to."""
    if (n, u) not in _prepared:
        out = {}
        for name, inp, tab in LC.cases(u):
            a_want, s_want = LC.reference(inp, tab, u)
            out[name] = (column(oracle, inp, n, LC.INPUT_PAD), column(oracle, tab, n, LC.TABLE_PAD), column(oracle, a_want, n, 0),
                         column(oracle, s_want, n, 0))
        _prepared[(n, u)] = out
    return _prepared[(n, u)]


@functools.lru_cache(maxsize=None)
def order_index(order, u):
    return np.array(LC.ORDERS[order](u), dtype=np.int64)


def in_order(inp_arr, u, order):
    out = inp_arr.copy()
    out[:u] = inp_arr[:u][order_index(order, u)]
    return out


def distinct_orders(u):
    """The orders that differ as permutations of u rows (at u = 1 they are all the same)."""
    seen, out = set(), []
    for name in LC.ORDERS:
        key = order_index(name, u).tobytes()
        if key not in seen:
            seen.add(key)
            out.append(name)
    return out


def run_columns(ctx, bufs, cols, n, u, what):
    """One call over the columns [(input, table, A', S')]; asserts the launch rule, both outputs and the table buffer."""
    inputs, tables = np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols])
    with launches(ctx) as got:
        a, s, t = call(ctx, bufs, inputs, tables, u)
    assert got == LC.launch_plan(n, u, len(cols)), (what, got)
    same(a, np.stack([c[2] for c in cols]), "%s: A'" % (what,))
    same(s, np.stack([c[3] for c in cols]), "%s: S'" % (what,))
    same(t, tables, "%s: the table buffer after the call" % (what,))


# ------------------------------------------------------------------------------ sizes, key sets, orders
@pytest.mark.parametrize("n", LC.SIZES)
def test_key_sets_in_every_order(ctx, oracle, n):
    """Every key set and multiset of lookup_permute_cases in every order of the input column, one lookup per call, from two
    rows (one compare-exchange by thread 0 of 64) through n = 32 (tile / 2 below the 64 threads launched), 256 and 512
    (128 and 256 threads), one tile, to two tiles with one global pass and eight tiles with six.

    What fails on which defect: key_less reading a limb as a signed number orders each `sign_bits` pair the wrong way
    round (test_lookup_permute_cases shows it on a model of that compare), so A' differs at the pair's rows — or
    lookup_mark's binary search walks away from a value that is there and the call is refused. A comparator that ranks
    the limbs in another order than 7...0 misorders the `limb_ladder` pair of the two limbs it swaps. A stage of the
    network with wrong index arithmetic leaves some 0-1 sequence unsorted (the 0-1 principle) — `zero_one` at the splits
    0, 1, u / 2, u - 1 and u in five orders; a barrier dropped where one is needed shows in the tiles of 256 keys and more,
    where a stage with j >= 128 hands data between wavefronts. The scans walk four tiles of 4096 flags at n = 16384
    (three carries, each of the two buffers of wavefront totals written twice) with every flag set (`all_equal`)."""
    with Buffers(ctx, 1, n) as bufs:
        for u in LC.default_usable(n):
            for name, (inp, tab, a_want, s_want) in prepared(oracle, n, u).items():
                for order in distinct_orders(u):
                    run_columns(ctx, bufs, [(in_order(inp, u, order), tab, a_want, s_want)], n, u, (n, u, name, order))


# ------------------------------------------------------------------------------ usable rows
@pytest.mark.parametrize("n,usable", [(64, u) for u in (0, 1, 63, 64)] + [(8192, u) for u in (1, 2, 4095, 4096, 4097, 8191, 8192)])
def test_usable_rows(ctx, oracle, n, usable):
    """`usable` from 0 to n, around the scans' tile of 4096 flags. `all_equal` sets every rep flag but the first and clears
    every used flag but one, so each scan's carry into the second tile is the largest there can be: 4095 of the 4096 flags
    before it. At usable = 4097 the second tile holds the one row 4096, whose rank is that carry and nothing else, and the
    total rank[usable] behind it; a carry that is dropped, doubled or taken from the other buffer of wavefront totals
    gives row 4096 another leftover (they are all distinct), and S' differs there.
    `many_leftovers` sets most flags with runs that straddle the tile edge.

    usable = 0: zk_lookup_permute used to launch lookup_mark with a grid of (0, L), which the runtime refuses — the call
    returned a HIP error. Nothing is launched now, and both outputs are all zero. usable = n: no row is zeroed (the
    three tail memsets would be zero bytes wide and are not issued), the answer is the permutation of all n rows."""
    with Buffers(ctx, 1, n) as bufs:
        if usable == 0:
            pad_in, pad_tab = column(oracle, [], n, LC.INPUT_PAD), column(oracle, [], n, LC.TABLE_PAD)
            zero = np.zeros((n, 4), np.uint64)
            run_columns(ctx, bufs, [(pad_in, pad_tab, zero, zero)], n, 0, (n, 0))
            return
        for name in ("all_equal", "many_leftovers"):
            _, inp, tab = LC.multiset_case(name, usable)
            a_want, s_want = LC.reference(inp, tab, usable)
            cols = (column(oracle, inp, n, LC.INPUT_PAD), column(oracle, tab, n, LC.TABLE_PAD), column(oracle, a_want, n, 0),
                    column(oracle, s_want, n, 0))
            for order in ("descending", "shuffle"):
                run_columns(ctx, bufs, [(in_order(cols[0], usable, order),) + cols[1:]], n, usable, (n, usable, name, order))


# ------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("n,L", [(4096, 3), (4096, 5), (16384, 3), (16384, 5)])
def test_batches_across_tiles(ctx, oracle, n, L):
    """L lookups in one call, every column with another key set and order, one of them with all inputs equal. The launches
    pick the column by blockIdx.y: the inputs are columns 0...L-1 of the first batch, the tables columns L...2L-1 and come
    from the second pointer (data_b + (blockIdx.y - ncols_a) * col_stride). A wrong column offset in the global pass —
    taken from `data` for a table, or off by one column — compare-exchanges across the tile boundary in the wrong column:
    that column comes out unsorted between its tiles (A' differs, or a table value is not found and the call is refused),
    and the column hit instead is disturbed. n = 4096 has one global pass, n = 16384 six."""
    u = n - 6
    cases = prepared(oracle, n, u)
    names = ["all_equal", "limb_ladder[0]", "many_leftovers", "sign_bits[0]", "zero_one[%d]" % (u // 2)][:L]
    orders = ["descending", "shuffle", "organ_pipe", "bit_reversed", "ascending"]
    cols = [(in_order(cases[nm][0], u, orders[i]),) + cases[nm][1:] for i, nm in enumerate(names)]
    with Buffers(ctx, L, n) as bufs:
        run_columns(ctx, bufs, cols, n, u, (n, L, names))


# ------------------------------------------------------------------------------ failures
FAIL_N, FAIL_U = 256, 250
FAIL_TABLE = [10 + 2 * i for i in range(FAIL_U)]  # even values: 11 lies between two of them, 3 below and r - 1 above all
FAILURES = {
    # kind: (the value that is not in the table's usable rows, the input row it is put in)
    "below_every_table_value": (3, 5),
    "above_every_table_value": (R - 1, 5),  # the binary search ends at lo == usable
    "between_at_the_first_row": (11, 0),
    "between_at_the_last_usable_row": (11, FAIL_U - 1),
    "only_in_the_table_beyond_usable": (LC.TABLE_PAD, 7),
}


def fail_columns(oracle, seed, bad=None, input_pad=LC.INPUT_PAD):
    """(input, table, A', S') of a lookup into FAIL_TABLE; with `bad` = (value, row) the input is not in the table."""
    rnd = np.random.RandomState(seed)
    inp = [FAIL_TABLE[int(i)] for i in rnd.randint(0, 40, FAIL_U)]
    tab = [FAIL_TABLE[int(i)] for i in rnd.permutation(FAIL_U)]
    want = (None, None)
    if bad is None:
        a_want, s_want = LC.reference(inp, tab, FAIL_U)
        want = (column(oracle, a_want, FAIL_N, 0), column(oracle, s_want, FAIL_N, 0))
    else:
        inp[bad[1]] = bad[0]
        with pytest.raises(AssertionError):
            LC.reference(inp + [input_pad] * 6, tab + [LC.TABLE_PAD] * 6, FAIL_U)
    return (column(oracle, inp, FAIL_N, input_pad), column(oracle, tab, FAIL_N, LC.TABLE_PAD)) + want


def refused_lookup(ctx, pkg, bufs, cols):
    """The call over `cols` is refused with "not in table"; returns the lookup index the message names."""
    with pytest.raises(pkg.AmdzkError) as e:
        call(ctx, bufs, np.stack([c[0] for c in cols]), np.stack([c[1] for c in cols]), FAIL_U)
    assert e.value.code == E_INVALID and "not in table" in str(e.value), str(e.value)
    same(bufs.tab.download((len(cols), FAIL_N, 4)), np.stack([c[1] for c in cols]), "the table buffer after a refusal")
    return int(re.search(r"lookup (\d+) input not in table", str(e.value)).group(1))


@pytest.mark.parametrize("kind", sorted(FAILURES))
def test_not_in_table(ctx, pkg, oracle, kind):
    """One input value that the table's usable rows do not hold: alone, then as lookup 0 and as lookup 2 of a batch of
    three whose other lookups are fine (the message names it), then in lookups 0 and 2 at once (either is named). After
    every refusal the same ctx permutes a good pair correctly. A binary search that stops one short, reads table[usable]
    when it ends at lo == usable, or a table sorted together with its rows beyond `usable` accepts one of these."""
    bad = FAILURES[kind]
    good = [fail_columns(oracle, seed) for seed in (1, 2, 3)]
    with Buffers(ctx, 3, FAIL_N) as bufs:
        assert refused_lookup(ctx, pkg, bufs, [fail_columns(oracle, 4, bad)]) == 0
        run_columns(ctx, bufs, good[:1], FAIL_N, FAIL_U, (kind, "after a refusal"))
        for at in (0, 2):
            cols = list(good)
            cols[at] = fail_columns(oracle, 5 + at, bad)
            assert refused_lookup(ctx, pkg, bufs, cols) == at
            run_columns(ctx, bufs, good, FAIL_N, FAIL_U, (kind, at, "after a refusal"))
        cols = [fail_columns(oracle, 8, bad), good[1], fail_columns(oracle, 9, bad)]
        assert refused_lookup(ctx, pkg, bufs, cols) in (0, 2)
        run_columns(ctx, bufs, good, FAIL_N, FAIL_U, (kind, "after two failing lookups"))


def test_a_missing_value_beyond_usable_is_not_a_failure(ctx, oracle):
    """The input's rows at or beyond `usable` are not looked up: 12345 there is in no table row."""
    assert 12345 not in FAIL_TABLE
    with Buffers(ctx, 1, FAIL_N) as bufs:
        run_columns(ctx, bufs, [fail_columns(oracle, 11, input_pad=12345)], FAIL_N, FAIL_U, "12345 beyond usable")


# ------------------------------------------------------------------------------ refusals
def test_refused_arguments_and_no_lookups(ctx, pkg, oracle):
    n, u = 64, 58
    cols = prepared(oracle, n, u)["many_leftovers"]
    inputs, tables = in_order(cols[0], u, "shuffle")[None], cols[1][None]
    with Buffers(ctx, 1, n) as bufs:
        def untouched(what):
            same(bufs.inp.download((1, n, 4)), inputs, "%s: the input buffer" % what)
            same(bufs.tab.download((1, n, 4)), tables, "%s: the table buffer" % what)
            same(bufs.out.download((n, 4)), np.tile(POISON, (n, 1)), "%s: the output buffer" % what)

        for bad_n, bad_u in ((0, 0), (1, 1), (3, 2), (n, n + 1)):
            with pytest.raises(pkg.AmdzkError) as e:
                call(ctx, bufs, inputs, tables, bad_u, n=bad_n)
            assert e.value.code == E_INVALID and "n must be a power of two >= usable" in str(e.value), (bad_n, bad_u, str(e.value))
            untouched("n = %d, usable = %d" % (bad_n, bad_u))
        ptrs = [bufs.inp.ptr, bufs.tab.ptr, bufs.out.ptr]
        for i in range(3):
            args = list(ptrs)
            args[i] = None
            with pytest.raises(pkg.AmdzkError) as e:
                ctx._chk(ctx.L.amdzk_permute_expression_pair_dev(ctx.h, args[0], args[1], args[2], 1, n, u))
            assert e.value.code == E_INVALID and "null argument" in str(e.value), (i, str(e.value))
            untouched("null pointer %d" % i)
        assert ctx.L.amdzk_permute_expression_pair_dev(None, ptrs[0], ptrs[1], ptrs[2], 1, n, u) == E_INVALID
        with launches(ctx) as got:
            call(ctx, bufs, inputs, tables, u, nlookups=0)
        assert got == {}
        untouched("nlookups = 0")
        run_columns(ctx, bufs, [(inputs[0], tables[0], cols[2], cols[3])], n, u, "after the refusals")


# ------------------------------------------------------------------------------ the prover's route, tables sorted at keygen
@pytest.mark.parametrize("tables", ["range_first", "pair_first"])
def test_prover_permutes_across_a_tile_with_presorted_tables(ctx, pkg, oracle, tables, monkeypatch):
    """create_proof's own permutation at k = 12 (usable = 4090: two sort tiles, one global pass, the scans' tile edge at row
    4096 beyond the usable rows), looked at column by column. `range_first` puts the one-column fixed table in front: its
    sorted form is made at keygen (lk_const = 1) and the prover sorts the two input columns and the one remaining table
    as two batches of unequal size; `pair_first` puts it behind the theta-compressed table, so nothing is cached. Each
    runs with the cache and with AMDZK_NO_TABLE_CACHE=1 (read at keygen). Theta comes from the prover (pk.inspect(1)),
    inputs and tables are compressed here with Python integers, and A' and S' on the usable rows must equal the
    reference's; the cached and the uncached run must give the same columns and the same proof."""
    import circuits
    import plonk_ref as PR
    from test_gpu_plonk_ops import prove_and_inspect

    c = circuits.lookup_circuit(pkg.plonk, 12, seed=41, tables=tables)
    desc, n, u = c.desc, c.n, c.usable
    A, I, L = desc["num_advice"], desc["num_instance"], len(desc["lookups"])
    assert n == 4096 and u > LC.SORT_TILE and L == 2
    inst_vals = [list(v) + [0] * (n - len(v)) for v in c.instances]
    od = zu.OracleDomain(oracle, desc["cs_degree"], c.k)
    runs = []
    for cache in (True, False):
        if not cache:
            monkeypatch.setenv("AMDZK_NO_TABLE_CACHE", "1")
        res, params = prove_and_inspect(ctx, pkg, oracle, c, seed=17)
        theta = res["chal"][0]
        rows = lambda p: zu.fr_array_to_ints(od.coeff_to_lagrange(res["polys_raw"][p]))[:u]
        got = [(rows(A + I + l), rows(A + I + L + l)) for l in range(L)]
        res["pk"].free()
        params.free()

        def compressed(exprs, row):
            acc = 0
            for e in exprs:
                v = PR.evaluate_expr(e, lambda cc, r: c.fixed[cc][(row + r) % n], lambda cc, r: c.advice[cc][(row + r) % n],
                                     lambda cc, r: inst_vals[cc][(row + r) % n])
                acc = (acc * theta + v) % R
            return acc

        for l, lk in enumerate(desc["lookups"]):
            inp, tab = [compressed(lk["inputs"], r) for r in range(u)], [compressed(lk["tables"], r) for r in range(u)]
            a_want, s_want = LC.reference(inp, tab, u)
            assert LC.check_definition(inp, tab, u, a_want, s_want) is None
            for what, g, w in (("A'", got[l][0], a_want), ("S'", got[l][1], s_want)):
                bad = [r for r in range(u) if g[r] != w[r]]
                assert not bad, "%s, cache %s, lookup %d: %s differs first at row %d: got %#x, want %#x" % (tables, cache, l, what, bad[0],
                                                                                                        g[bad[0]], w[bad[0]])
        runs.append((got, res["proof"]))
    assert runs[0][0] == runs[1][0], "the cached and the uncached run permute differently"
    assert runs[0][1] == runs[1][1], "the cached and the uncached run give different proofs"
