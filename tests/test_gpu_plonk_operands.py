"""GPU: the PLONK-layer kernels (csrc/plonk_kernels.hip: lincomb, poly_eval, kate_div, batch_invert, the scan kernels) at
extreme operands and on the launch paths tests/test_gpu_plonk_ops.py does not reach.

Operands are Montgomery words written directly (the word is the operand, as in test_gpu_ntt.py), all below r: a word w
stands for the value w * 2^-256 mod r. Every expected output is computed with Python integers on the words themselves
— a Montgomery product of the words a and b is the word a * b * 2^-256 mod r — never by the oracle library and never by
the device, and compared exactly. tests/test_fp29_wide_256.py shows that the reference model of the wide accumulator
stays inside its own bounds on these operands, so a mismatch here is the kernel's.

lincomb_kernel and poly_eval_kernel sum up to 256 unreduced products in 17 un-carried 64-bit columns; with uniform
random data a bound that is one bit too tight is hit with negligible probability. The data patterns are test_gpu_ntt.py's
(zkutil.PATTERNS); coefficients, points and roots enter the kernels as 32 w mod r (fr29_const_to_r261), so the scalar
list has words chosen by their image as well.

Which launch a case takes is decided by zk_lincomb / zk_poly_eval (plonk_kernels.hip). The cases state the path they
are meant to take, a Python copy of zk_lincomb's rule is asserted against that statement, and the library's own launch
counters (Context.prof_dump) are asserted against both: when the rule changes, the case fails instead of quietly
testing something else."""
import contextlib
import ctypes as C
import random

import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu
R = zu.R
MINV = pow(1 << 256, -1, R)
ONE = (1 << 256) % R  # the word of 1
T = R >> 232
INV32 = pow(32, -1, R)
DATA_PATTERNS = ["const_rm1", "const_t232m1", "alt_rm1_0", "alt_0_rm1", "half_rm1_0", "random_8th_rm1", "zero"]
# scalar words; the last two are chosen by what fr29_const_to_r261 makes of them: limbs all ones, and r - 1
SCALARS = {"zero": 0, "one": ONE, "rm1": R - 1, "t232m1": (T << 232) - 1, "image_all_ones": ((T << 232) - 1) * INV32 % R,
           "image_rm1": (R - 1) * INV32 % R}
POISON = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # not below r: a value no kernel writes


def _order_512():
    """A value x with x^256 = -1: poly_eval's power table (x^256)^j then alternates between 1 and r - 1."""
    g = 2
    while pow(pow(g, (R - 1) // 512, R), 256, R) != R - 1:
        g += 1
    return pow(g, (R - 1) // 512, R)


POINTS = dict(SCALARS, order_512=_order_512() * ONE % R)


def test_the_scalars_are_what_their_names_say():
    w = SCALARS["image_all_ones"]
    assert w < R and 32 * w % R == (T << 232) - 1 and 32 * SCALARS["image_rm1"] % R == R - 1
    assert all(((T << 232) - 1) >> (29 * i) & 0x1FFFFFFF == 0x1FFFFFFF for i in range(8))
    x = POINTS["order_512"] * MINV % R
    assert pow(x, 512, R) == 1 and pow(x, 256, R) == R - 1
    assert all(0 <= s < R for s in POINTS.values())


# ------------------------------------------------------------------------------ words <-> arrays, device plumbing
def to_words(a):
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def from_words(ws):
    return np.frombuffer(b"".join(w.to_bytes(32, "little") for w in ws), dtype=np.uint64).reshape(-1, 4).copy()


def upload(ctx, arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint64)
    return ctx.alloc(max(32, arr.nbytes)).upload(arr)


def ptr_array(addrs):
    return (C.c_void_p * max(1, len(addrs)))(*addrs)


@contextlib.contextmanager
def launches(ctx):
    """{kernel name: (launches, milliseconds)} of the calls made inside the block."""
    got = {}
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        yield got
        got.update(ctx.prof_dump())
    finally:
        ctx.prof_enable(False)


def count(got, name):
    return got.get(name, (0, 0.0))[0]


def first_mismatch(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return "first mismatch at index %d: got %#x, want %#x" % (i, g, w)
    return "lengths %d / %d" % (len(got), len(want))


# ------------------------------------------------------------------------------ lincomb
def lincomb_plan(m, n):
    """zk_lincomb's launch rule: (gx, nparts, per_part)."""
    gx = min((n + 255) // 256, 2048)
    nparts = 1
    while nparts < 16 and gx * nparts * 2 <= 2048 and m // (nparts * 2) >= 32:
        nparts *= 2
    return gx, nparts, (m if nparts == 1 else (m + nparts - 1) // nparts)


def axpy(ctx, addrs, coef_words, d_out, n, accumulate):
    m = len(addrs)
    coefs = from_words(coef_words) if m else None
    ctx._chk(ctx.L.amdzk_poly_axpy_dev(ctx.h, ptr_array(addrs) if m else None, coefs.ctypes.data_as(C.c_void_p) if m else None, m, d_out.ptr, n,
                                       accumulate))


def lincomb_want(cols, col_of, coefs, rows, before=None):
    """Words of (before +) sum_j coefs[j] * cols[col_of[j]] on `rows`; terms on the same column are gathered first."""
    gathered = [0] * len(cols)
    for j, c in enumerate(coefs):
        gathered[col_of[j]] += c
    used = [(g % R, col) for g, col in zip(gathered, cols) if g % R]
    return [(sum(g * col[i] for g, col in used) * MINV + (before[i] if before else 0)) % R for i in rows]


def run_lincomb(ctx, d_cols, n, col_of, coefs, path, accumulate=0, prefill=None):
    """One amdzk_poly_axpy_dev call over the columns d_cols (a device buffer of [ncols][n]) into an output pre-filled
    with `prefill` (default: poison); asserts the launch path (nparts, per_part) and returns the output's words."""
    m = len(coefs)
    gx, nparts, per_part = lincomb_plan(m, n)
    assert (nparts, per_part) == path, "zk_lincomb's rule gives another path for m = %d, n = %d" % (m, n)
    d_out = upload(ctx, np.tile(POISON, (n, 1)) if prefill is None else prefill)
    with launches(ctx) as got:
        axpy(ctx, [d_cols.ptr.value + c * n * 32 for c in col_of], coefs, d_out, n, accumulate)
    assert count(got, "lincomb") == (1 if m else 0) and count(got, "lincomb_sum_parts") == (1 if nparts > 1 else 0), got
    out = d_out.download((n, 4))
    d_out.free()
    return to_words(out)


@pytest.mark.parametrize("m,path", [(64, (2, 32)), (65, (2, 33)), (127, (2, 64)), (128, (4, 32)), (513, (16, 33))])
def test_lincomb_part_splits(ctx, m, path):
    """gridDim.y = nparts > 1, every term on a column of its own: an even split, a last part one term short (65: 33 + 32;
    127: 64 + 63), four parts, and sixteen with a last part of 18 (513 = 15 * 33 + 18) — at one row, just below and just
    above one workgroup of rows, and 300."""
    rnd = random.Random(1000 + m)
    for n in (1, 255, 257, 300):
        cols = zu.random_fr(m * n, seed=17 * m + n).reshape(m, n, 4)
        cols[m // 2] = zu.PATTERNS["random_8th_rm1"](n)
        coefs = [rnd.randrange(R) for _ in range(m)]
        coefs[m - 1] = SCALARS["image_all_ones"]  # the last part's last term must not be lost
        d_cols = upload(ctx, cols)
        got = run_lincomb(ctx, d_cols, n, list(range(m)), coefs, path)
        d_cols.free()
        want = lincomb_want([to_words(c) for c in cols], list(range(m)), coefs, range(n))
        assert got == want, "m = %d, n = %d: %s" % (m, n, first_mismatch(got, want))


def _mixed_columns(n, extra, seed):
    """The seven data patterns and `extra` random columns of n rows."""
    cols = [zu.PATTERNS[p](n) for p in DATA_PATTERNS] + [zu.random_fr(n, seed=seed + i) for i in range(extra)]
    return np.stack(cols)


@pytest.mark.parametrize("m,path", [(4176, (16, 261)), (8192, (16, 512))])
def test_lincomb_chunk_crossing_inside_a_part(ctx, m, path):
    """per_part > LC_CHUNK = 256: every part walks the chunk loop a second time (j0 = 256, the add(ld_fr(out + i), part)
    branch on the part's own slice of the workspace) — with 5 terms in the second chunk (261), and with a chunk boundary
    exactly at the part's end (512). 17 distinct columns, term j on column j mod 17 (256 mod 17 != 0: a chunk that read
    another chunk's coefficients would pair them with other columns)."""
    n, ncols = 300, 17
    rnd = random.Random(m)
    cols = _mixed_columns(n, ncols - len(DATA_PATTERNS), seed=m)
    scal = list(SCALARS.values())
    coefs = [scal[j % len(scal)] if j % 5 == 0 else rnd.randrange(R) for j in range(m)]
    col_of = [j % ncols for j in range(m)]
    d_cols = upload(ctx, cols)
    got = run_lincomb(ctx, d_cols, n, col_of, coefs, path)
    d_cols.free()
    want = lincomb_want([to_words(c) for c in cols], col_of, coefs, range(n))
    assert got == want, first_mismatch(got, want)


BIG_N = (1 << 18) + 1  # 1025 workgroups of rows: zk_lincomb no longer splits the terms, one launch walks all of them


@pytest.fixture(scope="module")
def big_columns(ctx):
    cols = [zu.PATTERNS["random_8th_rm1"](BIG_N), zu.PATTERNS["const_rm1"](BIG_N), zu.random_fr(BIG_N, seed=4242)]
    rnd = random.Random(99)
    rows = {0, BIG_N - 1} | {k * 65536 + d for k in range(1, 5) for d in (-1, 0, 1)} | {rnd.randrange(BIG_N) for _ in range(64)}
    rows = sorted(r for r in rows if r < BIG_N)
    sample = [dict(zip(rows, to_words(c[rows]))) for c in cols]
    d_cols = upload(ctx, np.stack(cols))
    yield d_cols, rows, sample
    d_cols.free()


@pytest.mark.parametrize("m", [256, 257, 300, 513])
def test_lincomb_one_part_with_several_chunks(ctx, big_columns, m):
    """gridDim.y = 1 and m > 256: the kernel's chunk loop writes its second and third partial sums onto the caller's
    output (m = 256: exactly one chunk, the control). Python checks a sample of rows — first, last, around every multiple
    of 65536, 64 random ones; every row is compared with the same sum made by hand of calls of at most 256 terms, each
    after the first with accumulate = 1 (one chunk each, the in-kernel accumulate branch)."""
    d_cols, rows, sample = big_columns
    rnd = random.Random(m)
    scal = list(SCALARS.values())
    coefs = [scal[j % len(scal)] if j % 7 == 0 else rnd.randrange(R) for j in range(m)]
    col_of = [(j * j + j // 3) % 3 for j in range(m)]
    assert lincomb_plan(m, BIG_N) == (1025, 1, m)
    addrs = [d_cols.ptr.value + c * BIG_N * 32 for c in col_of]
    d_out = upload(ctx, np.tile(POISON, (BIG_N, 1)))
    with launches(ctx) as got:
        axpy(ctx, addrs, coefs, d_out, BIG_N, 0)
    assert count(got, "lincomb") == 1 and count(got, "lincomb_sum_parts") == 0, got
    whole = d_out.download((BIG_N, 4))
    want = lincomb_want(sample, col_of, coefs, rows)
    have = to_words(whole[rows])
    assert have == want, "row %d" % rows[[h == w for h, w in zip(have, want)].index(False)]
    d_out.upload(np.tile(POISON, (BIG_N, 1)))
    for lo in range(0, m, 256):
        axpy(ctx, addrs[lo:lo + 256], coefs[lo:lo + 256], d_out, BIG_N, 1 if lo else 0)
    by_hand = d_out.download((BIG_N, 4))
    d_out.free()
    assert np.array_equal(whole, by_hand)


@pytest.mark.parametrize("m,path", [(3, (1, 3)), (513, (16, 33))])
def test_lincomb_accumulate(ctx, m, path):
    """accumulate = 1 adds to what the output holds — in lincomb_kernel itself (one part) and in lincomb_sum_parts_kernel
    (sixteen); accumulate = 0 overwrites a poisoned output on both routes."""
    n = 300
    rnd = random.Random(7 * m)
    cols = _mixed_columns(n, 2, seed=m)
    coefs = [rnd.randrange(R) for _ in range(m)]
    col_of = [j % len(cols) for j in range(m)]
    before = zu.PATTERNS["random_8th_rm1"](n)
    words = [to_words(c) for c in cols]
    d_cols = upload(ctx, cols)
    got = run_lincomb(ctx, d_cols, n, col_of, coefs, path, accumulate=1, prefill=before)
    want = lincomb_want(words, col_of, coefs, range(n), before=to_words(before))
    assert got == want, "accumulate = 1: " + first_mismatch(got, want)
    got = run_lincomb(ctx, d_cols, n, col_of, coefs, path, accumulate=0)
    want = lincomb_want(words, col_of, coefs, range(n))
    assert got == want, "accumulate = 0: " + first_mismatch(got, want)
    d_cols.free()


def test_lincomb_of_no_terms(ctx):
    """m = 0: zeros with accumulate = 0, the output untouched with accumulate = 1."""
    n = 300
    d_cols = upload(ctx, np.zeros((1, 4), np.uint64))
    assert run_lincomb(ctx, d_cols, n, [], [], (1, 0), accumulate=0) == [0] * n
    before = zu.PATTERNS["random_8th_rm1"](n)
    assert run_lincomb(ctx, d_cols, n, [], [], (1, 0), accumulate=1, prefill=before) == to_words(before)
    d_cols.free()


# m = 255, 256, 257 at n = 300 are cut into parts of at most 64 terms; sixteen times as many terms give sixteen parts of
# 255, 256 (one full chunk: the case the bound T < 256 p^2 is about) and 257 (a chunk and one term) each.
EXTREME_M = [(255, (4, 64)), (256, (8, 32)), (257, (8, 33)), (4080, (16, 255)), (4096, (16, 256)), (4112, (16, 257))]


@pytest.mark.parametrize("pattern", DATA_PATTERNS + ["mixed"])
@pytest.mark.parametrize("m,path", EXTREME_M)
def test_lincomb_extreme_operands(ctx, m, path, pattern):
    """Every term of the sum the same extreme product: all m terms read one column of the pattern and carry the same
    coefficient, for every coefficient of the scalar list ("mixed": term j on pattern j mod 7 with coefficient j mod 6)."""
    n = 300
    if pattern == "mixed":
        cols = _mixed_columns(n, 0, seed=0)
        runs = [("mixed", [j % len(cols) for j in range(m)], [list(SCALARS.values())[j % len(SCALARS)] for j in range(m)])]
    else:
        cols = zu.PATTERNS[pattern](n)[None]
        runs = [(name, [0] * m, [s] * m) for name, s in SCALARS.items()]
    words = [to_words(c) for c in cols]
    d_cols = upload(ctx, cols)
    for name, col_of, coefs in runs:
        got = run_lincomb(ctx, d_cols, n, col_of, coefs, path)
        want = lincomb_want(words, col_of, coefs, range(n))
        assert got == want, "lincomb: pattern %s, scalar %s, m = %d, n = %d: %s" % (pattern, name, m, n, first_mismatch(got, want))
    d_cols.free()


# ------------------------------------------------------------------------------ poly_eval
def horner(coef_words, x_word):
    """The word of p(x) for coefficient words and the word of x."""
    x = x_word * MINV % R
    if x == 0 or not any(coef_words):
        return coef_words[0] if coef_words else 0
    acc = 0
    for c in reversed(coef_words):
        acc = (acc * x + c) % R
    return acc


def eval_polys(ctx, addrs, point_words, n):
    nq = len(addrs)
    pts = from_words(point_words)
    out = np.zeros((nq, 4), np.uint64)
    ctx._chk(ctx.L.amdzk_eval_poly_dev(ctx.h, ptr_array(addrs), pts.ctypes.data_as(C.c_void_p), nq, n, out.ctypes.data_as(C.c_void_p)))
    return to_words(out)


@pytest.mark.parametrize("n", [255, 256, 257, 65536, 65537, (1 << 17) + 77])
def test_eval_extreme_operands(ctx, n):
    """Every data pattern at every point of the list, one query each in one call. Up to 65536 coefficients a workgroup
    takes the whole polynomial (n = 65536: 256 terms per lane against the full power table, the bound's own case; 255 ...
    257: the first lane gets a second term); above, zk_poly_eval cuts a query into segments of 65536 on gridDim.y = 2 and
    3 and poly_eval_combine_kernel folds them. (The second operand of every term is an entry of the power table, a
    product's result: no point sets its limbs one by one, so unlike lincomb's coefficients these inputs cannot bring a
    column to the edge of its 64 bits. The model's margin for that case is pinned in test_fp29_wide_256.py.)"""
    cols = np.stack([zu.PATTERNS[p](n) for p in DATA_PATTERNS])
    words = [to_words(c) for c in cols]
    queries = [(p, s) for p in range(len(DATA_PATTERNS)) for s in POINTS]
    d_cols = upload(ctx, cols)
    with launches(ctx) as got:
        have = eval_polys(ctx, [d_cols.ptr.value + p * n * 32 for p, _ in queries], [POINTS[s] for _, s in queries], n)
    d_cols.free()
    assert count(got, "poly_eval") == 1 and count(got, "poly_eval_combine") == (1 if n > 65536 else 0), got
    for (p, s), h in zip(queries, have):
        want = horner(words[p], POINTS[s])
        assert h == want, "poly_eval: pattern %s, point %s, n = %d: got %#x, want %#x" % (DATA_PATTERNS[p], s, n, h, want)


@pytest.mark.parametrize("pattern", ["random_8th_rm1", "const_rm1"])
def test_eval_more_queries_than_grid_rows(ctx, pattern):
    """nq = 65536 > 65535 queries of n = 65537 > 2^16 coefficients: gridDim.y cannot hold the segments next to that many
    queries, so every workgroup walks both segments itself and folds them with (x^256)^256 (nseg = 2, gridDim.y = 1: the
    f29_add(f29_mul(acc, xbig), part) line). All queries read one polynomial; eight points dealt round-robin."""
    n, nq = 65537, 65536
    col = zu.PATTERNS[pattern](n)
    words = to_words(col)
    pts = list(POINTS.values()) + [random.Random(5).randrange(R)]
    assert len(pts) == 8
    d_col = upload(ctx, col)
    with launches(ctx) as got:
        have = eval_polys(ctx, [d_col.ptr.value] * nq, [pts[q % 8] for q in range(nq)], n)
    d_col.free()
    assert count(got, "poly_eval") == 1 and count(got, "poly_eval_combine") == 0, got
    print("poly_eval, 65536 queries x 65537 coefficients in one launch: %.1f ms" % got["poly_eval"][1])
    want = [horner(words, x) for x in pts]
    bad = [q for q in range(nq) if have[q] != want[q % 8]]
    assert not bad, "poly_eval: pattern %s, n = %d, %d of %d queries wrong, the first is query %d (point %d)" % (pattern, n, len(bad), nq, bad[0], bad[0] % 8)


def test_eval_a_thousand_queries(ctx):
    n, nq = 300, 1000
    cols = _mixed_columns(n, 1, seed=300)
    words = [to_words(c) for c in cols]
    rnd = random.Random(1000)
    pts = list(POINTS.values()) + [rnd.randrange(R) for _ in range(6)]
    qs = [(q % len(cols), (q // 3) % len(pts)) for q in range(nq)]
    d_cols = upload(ctx, cols)
    have = eval_polys(ctx, [d_cols.ptr.value + c * n * 32 for c, _ in qs], [pts[p] for _, p in qs], n)
    d_cols.free()
    memo = {}
    for q, (c, p) in enumerate(qs):
        if (c, p) not in memo:
            memo[c, p] = horner(words[c], pts[p])
        assert have[q] == memo[c, p], "query %d (column %d, point %d)" % (q, c, p)


# ------------------------------------------------------------------------------ kate_div
@pytest.mark.parametrize("n", [2048, 2049, 6000])
def test_kate_division_extreme_operands(ctx, n):
    """Every data pattern divided by X - b for every root of the scalar list, one polynomial each in one call: one block
    of KD_BLOCK = 2048 coefficients exactly, one more (the carry pass), and three blocks with a ragged tail. Expected:
    synthetic division, and q(X) (X - b) + a(b) = a(X) coefficient by coefficient."""
    pairs = [(p, s) for p in DATA_PATTERNS for s in SCALARS]
    src = {p: zu.PATTERNS[p](n) for p in DATA_PATTERNS}
    buf = upload(ctx, np.stack([src[p] for p, _ in pairs]))
    roots = from_words([SCALARS[s] for _, s in pairs])
    with launches(ctx) as got:
        ctx._chk(ctx.L.amdzk_kate_div_dev(ctx.h, ptr_array([buf.ptr.value + i * n * 32 for i in range(len(pairs))]),
                                          roots.ctypes.data_as(C.c_void_p), len(pairs), n))
    assert count(got, "kate_div") == 1 and count(got, "kate_div_carry") == (1 if n > 2048 else 0), got
    out = buf.download((len(pairs), n, 4))
    buf.free()
    for i, (p, s) in enumerate(pairs):
        a = to_words(src[p])
        b = SCALARS[s] * MINV % R
        q, acc = [0] * n, 0
        for j in range(n - 1, 0, -1):
            acc = (acc * b + a[j]) % R
            q[j - 1] = acc
        rem = (acc * b + a[0]) % R  # the word of a(b)
        have = to_words(out[i])
        assert have == q, "kate_div: pattern %s, root %s, n = %d: %s" % (p, s, n, first_mismatch(have, q))
        back = [((have[j - 1] if j else 0) - b * have[j] + (0 if j else rem)) % R for j in range(n)]
        assert back == a and rem == horner(a, SCALARS[s])


# ------------------------------------------------------------------------------ batch_invert
BI_WG = 2048  # elements per workgroup = per inversion: thread t of workgroup w owns w * 2048 + j * 256 + t, j < 8
# What inv_gcd is handed is the Montgomery WORD of the workgroup's product: small, huge, even, odd, a power of two. Each
# name once as the word itself and once as the word of that value.
_TARGET_VALUES = {"1": 1, "2": 2, "r-1": R - 1, "(r+1)/2": (R + 1) // 2, "2^253": 1 << 253, "t232m1": (T << 232) - 1}
INV_TARGETS = sorted({w for v in _TARGET_VALUES.values() for w in (v, v * ONE % R)} | {MINV * ONE % R, MINV})


_inverse_of = {0: 0}


def invert_words(ws):
    """Words of the inverses: (w 2^-256)^-1 2^256 = w^-1 2^512; zero stays zero."""
    k = ONE * ONE % R
    for w in ws:
        if w not in _inverse_of:
            _inverse_of[w] = pow(w, -1, R) * k % R
    return [_inverse_of[w] for w in ws]


def batch_invert(ctx, ws):
    buf = upload(ctx, from_words(ws))
    with launches(ctx) as got:
        ctx._chk(ctx.L.amdzk_batch_invert_dev(ctx.h, buf.ptr, len(ws)))
    assert count(got, "batch_invert") == 1
    out = to_words(buf.download((len(ws), 4)))
    buf.free()
    return out


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4096, 4097, 6145])
def test_batch_invert_at_workgroup_boundaries(ctx, n):
    """One inversion per 2048 elements: sizes around one, two and three workgroups (6145: a fourth with one element).
    (a) A workgroup of ones with one chosen word: that word is the product inv_gcd gets; every target, the slot moving
    through the threads and the eight elements of a thread, in the last workgroup (the ragged one) and the first.
    (b) A workgroup whose only non-zero element is its last. (c) the word r - 1 throughout (const_rm1), and the word of the value r - 1, which is its own inverse.
    (d) random data with zeros, every workgroup different."""
    assert 1 in INV_TARGETS and 2 in INV_TARGETS and R - 1 in INV_TARGETS and ONE in INV_TARGETS and len(INV_TARGETS) >= 12
    nwg = (n + BI_WG - 1) // BI_WG
    rnd = random.Random(n)
    base = [rnd.randrange(1, R) for _ in range(n)]
    for k, target in enumerate(INV_TARGETS):
        wg = nwg - 1 if k % 2 == 0 else 0
        lo, hi = wg * BI_WG, min(n, (wg + 1) * BI_WG)
        ws = list(base)
        ws[lo:hi] = [ONE] * (hi - lo)
        ws[lo + (k * 331 + 255 * (k % 3)) % (hi - lo)] = target
        got, want = batch_invert(ctx, ws), invert_words(ws)
        assert got == want, "batch_invert: n = %d, workgroup %d of ones with the word %#x: %s" % (n, wg, target, first_mismatch(got, want))
    for wg in range(nwg):
        lo, hi = wg * BI_WG, min(n, (wg + 1) * BI_WG)
        ws = list(base)
        ws[lo:hi] = [0] * (hi - lo - 1) + [SCALARS["t232m1"]]
        got, want = batch_invert(ctx, ws), invert_words(ws)
        assert got == want, "batch_invert: n = %d, workgroup %d zero but for its last element: %s" % (n, wg, first_mismatch(got, want))
    minus_one = R - ONE  # the word of the value r - 1, its own inverse; the word r - 1 (const_rm1) is the value -2^-256
    assert invert_words([minus_one]) == [minus_one] and invert_words([R - 1]) == [R - ONE * ONE % R]
    for name, w in (("the word r - 1", R - 1), ("the word of r - 1", minus_one)):
        got, want = batch_invert(ctx, [w] * n), invert_words([w] * n)
        assert got == want, "batch_invert: n = %d, %s throughout: %s" % (n, name, first_mismatch(got, want))
    ws = [0 if i % 7 == 3 else w for i, w in enumerate(base)]
    got, want = batch_invert(ctx, ws), invert_words(ws)
    assert got == want, "batch_invert: n = %d, random with zeros: %s" % (n, first_mismatch(got, want))


# ------------------------------------------------------------------------------ grand_product
SENTINEL = 0x5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A5A  # fills the gap between columns


def grand_product(ctx, cols, stride, chain, chain_row=0):
    """amdzk_grand_product_dev on columns of words laid out `stride` apart, the gaps filled with SENTINEL, which must
    survive; returns the columns' words."""
    ncols, n = len(cols), len(cols[0])
    host = np.tile(from_words([SENTINEL]), (ncols * stride, 1)).reshape(ncols, stride, 4)
    for c, col in enumerate(cols):
        host[c, :n] = from_words(col)
    buf = upload(ctx, host)
    with launches(ctx) as got:
        ctx._chk(ctx.L.amdzk_grand_product_dev(ctx.h, buf.ptr, ncols, n, stride, 1 if chain else 0, chain_row))
    assert count(got, "scan_local") == 1 and count(got, "scan_blocks") == 1 and count(got, "scan_chain") == (1 if chain else 0), got
    out = buf.download(host.shape)
    buf.free()
    assert stride == n or to_words(out[:, n:].reshape(-1, 4)) == [SENTINEL] * (ncols * (stride - n)), "the gap between columns was written"
    return [to_words(out[c, :n]) for c in range(ncols)]


def running_products(cols, chain, chain_row):
    """z[0] = start, z[i] = z[i-1] * f[i-1] on words; start = the word of 1, or with `chain` the previous column's
    z[chain_row]."""
    out, start = [], ONE
    for col in cols:
        z, acc = [], start
        for w in col:
            z.append(acc)
            acc = acc * w * MINV % R
        out.append(z)
        if chain:
            start = z[chain_row]
    return out


def check_grand_product(ctx, cols, what):
    n = len(cols[0])
    u = n - 1 if n < 10 else n - 6
    for stride in (n, n + 5):
        for chain in (False, True):
            got, want = grand_product(ctx, cols, stride, chain, u), running_products(cols, chain, u)
            for c in range(len(cols)):
                assert got[c] == want[c], "grand_product: %s, n = %d, stride %d, chain %d, column %d: %s" % (
                    what, n, stride, chain, c, first_mismatch(got[c], want[c]))


@pytest.mark.parametrize("n", [7, 2049])
@pytest.mark.parametrize("ncols", [64, 65, 130])
def test_grand_product_many_columns(ctx, ncols, n):
    """scan_blocks_kernel gives every column a lane in workgroups of 64: one workgroup exactly, a second with one lane, a
    third with two — in one block of rows and in two (SCAN_BLOCK = 2048), plain and chained through z[u], packed and with
    col_stride = n + 5 (a sentinel in the gap)."""
    rnd = random.Random(ncols * 10000 + n)
    cols = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(ncols)]
    cols[ncols - 1][n // 2] = R - 1
    check_grand_product(ctx, cols, "%d random columns" % ncols)


def test_grand_product_with_a_zero_factor(ctx):
    """A zero in a column: every later row of it is zero, and chained, every later column is zero from its first row."""
    n, ncols = 2049, 66
    rnd = random.Random(66)
    cols = [[rnd.randrange(1, R) for _ in range(n)] for _ in range(ncols)]
    cols[3][700] = 0      # before the chain row, in the first block of rows
    cols[64][2046] = 0    # behind the chain row n - 6, in a column of the second workgroup of scan_blocks_kernel
    want = running_products(cols, True, n - 6)
    assert want[3][701:] == [0] * (n - 701) and want[3][700] != 0 and all(w == [0] * n for w in want[4:])
    plain = running_products(cols, False, 0)[64]
    assert plain[2046] != 0 and plain[2047:] == [0, 0]
    check_grand_product(ctx, cols, "zero factors")


@pytest.mark.parametrize("n", [2048, 2049, 4097])
def test_grand_product_extreme_columns(ctx, n):
    """The word r - 1 throughout (the running product is the powers of the value -2^-256), the all-ones word throughout,
    and r - 1 alternating with zero, beside random columns: one block of rows, one more row, and two blocks and one row."""
    rnd = random.Random(n)
    cols = [to_words(zu.PATTERNS["const_rm1"](n)), to_words(zu.PATTERNS["alt_rm1_0"](n)), [rnd.randrange(1, R) for _ in range(n)],
            to_words(zu.PATTERNS["const_t232m1"](n)), to_words(zu.PATTERNS["random_8th_rm1"](n))]
    check_grand_product(ctx, cols[:1] + cols[2:], "const_rm1, random, const_t232m1, random_8th_rm1")
    check_grand_product(ctx, [cols[0], cols[2], cols[1], cols[4]], "const_rm1, random, alt_rm1_0, random_8th_rm1")
