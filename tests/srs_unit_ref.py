"""References for the SRS unit (csrc/srs.hip), in Python integers: the G1 point codec of ParamsKZG::{write, read}, and two
scalar-domain simulators that restate the INDEX ARITHMETIC of the device's group FFT (ecfft_round_kernel) and of its prefix
scan (ec_prefix_sums) and classify every point addition the device performs.

The simulators work on scalars because every test point is a_i * G with a known a_i and G has prime order r: two points are
equal, opposite or the identity exactly when their scalars are equal, opposite or zero mod r. So a test can CHOOSE its input
such that the device meets a doubling, a cancellation or an identity at a chosen thread of a chosen round, and assert on the
CPU that it does (tests/test_srs_unit_ref.py), before the device is asked for the points (tests/test_gpu_srs_unit.py)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyref as P  # noqa: E402

Q, R = P.Q, P.R


# ------------------------------------------------------------------------------------------------ the G1 codec
def g1_y_from_x(x, sign):
    """The y with y^2 = x^3 + 3 whose parity is `sign`, or None when x^3 + 3 is a non-residue (q = 3 mod 4)."""
    rhs = (x * x * x + P.CURVE_B) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    if y * y % Q != rhs:
        return None
    return y if (y & 1) == sign else (Q - y) % Q


def g1_decompress(b):
    """halo2curves' G1Affine::from_bytes on 32 bytes: ("point", (x, y)), ("identity", None) or ("refused", reason).
    x little-endian in bits 0..254, bit 255 = parity of y; x must be canonical; 32 zero bytes are the identity."""
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    sign, x = v >> 255, v & ((1 << 255) - 1)
    if x >= Q:
        return "refused", "x >= q"
    if x == 0 and sign == 0:
        return "identity", None
    y = g1_y_from_x(x, sign)
    if y is None:
        return "refused", "no point of the curve has this x"
    return "point", (x, y)


def g1_encode(x, sign):
    """The 32 bytes that claim (x, parity sign) — x any integer below 2^255, on the curve or not."""
    assert 0 <= x < 1 << 255 and sign in (0, 1)
    return (x | sign << 255).to_bytes(32, "little")


# Encodings ParamsKZG::read must refuse, by name. x = 0 has no point because 3 is a non-residue; 4 and 10 are the two
# smallest x above 1 that no point has.
REFUSED_ENCODINGS = [
    ("x_eq_q", g1_encode(Q, 0)),
    ("x_eq_q_plus_1", g1_encode(Q + 1, 0)),  # = 1 mod q: the generator's x, not canonical
    ("x_1_bit_254", g1_encode(1 | 1 << 254, 0)),
    ("all_ff", b"\xff" * 32),
    ("x_0_sign_set", g1_encode(0, 1)),
    ("x_4_sign_0", g1_encode(4, 0)),
    ("x_4_sign_1", g1_encode(4, 1)),
    ("x_10_sign_0", g1_encode(10, 0)),
    ("x_10_sign_1", g1_encode(10, 1)),
]
# Encodings it must accept (besides random points): (name, bytes)
ACCEPTED_ENCODINGS = [
    ("identity", bytes(32)),
    ("x_1_sign_0", g1_encode(1, 0)),
    ("x_1_sign_1", g1_encode(1, 1)),
    ("x_qm1_sign_0", g1_encode(Q - 1, 0)),
    ("x_qm1_sign_1", g1_encode(Q - 1, 1)),
]


def edge_points():
    """Named points for the compressor: (1, 2) and (1, q - 2); both points with x = q - 1; the first multiple of G whose
    canonical x has bit 253 set; the point with the smallest x above 1 (far below 2^32), both parities."""
    out = [("gen", (1, 2)), ("neg_gen", (1, Q - 2))]
    y = g1_y_from_x(Q - 1, 0)
    out += [("x_qm1_even", (Q - 1, y)), ("x_qm1_odd", (Q - 1, Q - y))]
    p, i = P.G1_GEN, 1
    while not p[0] >> 253:
        p, i = P.g1_add(p, P.G1_GEN), i + 1
    out.append(("x_bit_253", p))
    x = 2
    while g1_y_from_x(x, 0) is None:
        x += 1
    out += [("x_small_even", (x, g1_y_from_x(x, 0))), ("x_small_odd", (x, g1_y_from_x(x, 1)))]
    return out


# ------------------------------------------------------------------------------------------------ the group FFT
def brev(i, k):
    return int(format(i, "0%db" % k)[::-1], 2) if k else 0


def classify_butterfly(u, v):
    if u == 0 and v == 0:
        return "u0v0"
    if u == 0:
        return "u0"
    if v == 0:
        return "v0"
    if u == v:
        return "eq"  # u + v doubles, u - v is the identity
    if (u + v) % R == 0:
        return "neg"  # u + v is the identity, u - v doubles
    return "gen"


BUTTERFLY_KINDS = ("gen", "eq", "neg", "u0", "v0", "u0v0")


def ecfft_sim(a, k):
    """ecfft_to_lagrange on scalars: k DIF rounds with ecfft_round_kernel's indices (thread j of round s: half = 2^(k-1-s),
    pos = j & (half - 1), i0 = (j >> half_log << half_log + 1) + pos, i1 = i0 + half, twiddle omega^-(pos << s), none at
    pos = 0), then ecfft_finish_kernel (times 1/n, to the bit-reversed index).
    Returns (state after the rounds, output, kinds) with kinds[s][j] the class of thread j's butterfly in round s."""
    n = 1 << k
    a = [x % R for x in a]
    assert len(a) == n
    w = pow(P.omega(k), -1, R) if k else 1
    tw = [pow(w, i, R) for i in range(max(n // 2, 1))]
    kinds = []
    for s in range(k):
        half_log = k - 1 - s
        half = 1 << half_log
        row = []
        for j in range(n // 2):
            pos = j & (half - 1)
            i0 = ((j >> half_log) << (half_log + 1)) + pos
            i1 = i0 + half
            u, v = a[i0], a[i1]
            row.append(classify_butterfly(u, v))
            a[i0] = (u + v) % R
            d = (u - v) % R
            if pos:
                d = d * tw[pos << s] % R
            a[i1] = d
        kinds.append(row)
    ninv = pow(n, -1, R)
    out = [0] * n
    for i in range(n):
        out[brev(i, k)] = a[i] * ninv % R
    return a, out, kinds


def ecfft_invert_round0(t, k):
    """The input whose state after round 0 is t: round 0 pairs (j, j + n/2) as (u + v, (u - v) omega^-j), invertible over Fr."""
    n = 1 << k
    half = n // 2
    w = P.omega(k)  # the inverse of the round's twiddle base
    inv2 = pow(2, -1, R)
    a = [0] * n
    for j in range(half):
        s, d = t[j], t[j + half] * pow(w, j, R) % R
        a[j], a[j + half] = (s + d) * inv2 % R, (s - d) * inv2 % R
    return a


def _rand_fr(rnd):
    while True:
        v = int.from_bytes(rnd.bytes(32), "little") % R
        if v:
            return v


_CLASS_SHIFT = (0, 5, 3, 4, 0, 1, 3, 5)


def ecfft_degenerate_input(k, seed=2024):
    """Scalars a (n = 2^k, k >= 2) whose round 1 is degenerate everywhere: round 1 pairs state[i0] with state[i0 + n/4], and
    the pair at position pos of its quarter is given a class that cycles through the six with pos, restarted with a shift of
    its own (_CLASS_SHIFT) in each eighth of the quarter and one further in the first half of the threads. The state at the
    start of round 1 is chosen, round 0 is inverted. The identities made in round 1 (eq: u - v, neg: u + v, u0v0: both) then
    meet each other (u0v0) and finite points (u0, v0) in rounds 2 and 3, which pair positions n/8 and n/16 apart: the shifts
    were searched for so that both rounds see all three in blocks 1 and up; test_srs_unit_ref.py asserts that they do."""
    import numpy as np
    rnd = np.random.RandomState(seed)
    n = 1 << k
    quarter = n // 4
    eighth = quarter // 8
    assert eighth >= 6
    t = [0] * n
    for j in range(n // 2):
        i0 = ((j >> (k - 2)) << (k - 1)) + (j & (quarter - 1))
        i1 = i0 + quarter
        pos = j & (quarter - 1)
        kind = BUTTERFLY_KINDS[(pos % eighth + _CLASS_SHIFT[pos // eighth] + (j < quarter)) % 6]
        x, y = _rand_fr(rnd), _rand_fr(rnd)
        t[i0], t[i1] = {"gen": (x, y), "eq": (x, x), "neg": (x, R - x), "u0": (0, y), "v0": (x, 0), "u0v0": (0, 0)}[kind]
    return ecfft_invert_round0(t, k)


def butterfly_counts(kinds_row, first_thread=0):
    c = dict.fromkeys(BUTTERFLY_KINDS, 0)
    for kind in kinds_row[first_thread:]:
        c[kind] += 1
    return c


# ------------------------------------------------------------------------------------------------ the prefix scan
CHUNK = 16  # PREFIX_CHUNK
STEP_KINDS = ("general", "into_identity", "adding_identity", "doubling", "cancelling")


def classify_step(acc, nxt):
    if nxt == 0:
        return "adding_identity"
    if acc == 0:
        return "into_identity"
    if acc == nxt:
        return "doubling"
    if (acc + nxt) % R == 0:
        return "cancelling"
    return "general"


def prefix_level_sizes(n):
    """[n, chunks of n, chunks of those, ...] down to the one chunk at the top (ec_prefix_sums' `sizes`, with n in front)."""
    sizes = [n]
    while sizes[-1] > CHUNK:
        sizes.append((sizes[-1] + CHUNK - 1) // CHUNK)
    return sizes


def prefix_sim(a):
    """ec_prefix_sums on scalars. Returns (prefix, steps, info):
    prefix[i] = a[0] + ... + a[i];
    steps = [(level, pass, chunk, index in the level, first step of its chunk?, kind)] for every addition of every kernel —
    pass "total" is prefix_chunk_total_kernel (level 0: <G1Affine>, above: <G1X>), pass "apply" is prefix_apply_x_kernel
    (levels above 0) or prefix_apply_affine_kernel (level 0);
    info = {"sizes", "totals": the chunk totals per level, "carries": the carries each apply pass started from (chunk > 0),
    "ragged": [(level, chunk, lo, hi)] where hi = m < lo + 16 bound}."""
    a = [x % R for x in a]
    sizes = prefix_level_sizes(len(a))
    levels = [a]
    steps, ragged = [], []
    for l in range(len(sizes) - 1):  # up
        src, m = levels[l], sizes[l]
        tot = []
        for t in range((m + CHUNK - 1) // CHUNK):
            lo, hi = t * CHUNK, min(t * CHUNK + CHUNK, m)
            if hi < lo + CHUNK:
                ragged.append((l, t, lo, hi))
            acc = 0
            for i in range(lo, hi):
                steps.append((l, "total", t, i, i == lo, classify_step(acc, src[i])))
                acc = (acc + src[i]) % R
            tot.append(acc)
        assert len(tot) == sizes[l + 1]
        levels.append(tot)
    totals = [list(lv) for lv in levels[1:]]
    carries = {}
    scanned = [None] * len(sizes)
    for l in range(len(sizes) - 1, -1, -1):  # down
        src, m = levels[l], sizes[l]
        carry = scanned[l + 1] if l + 1 < len(sizes) else None
        out = [0] * m
        carries[l] = []
        for t in range((m + CHUNK - 1) // CHUNK):
            lo, hi = t * CHUNK, min(t * CHUNK + CHUNK, m)
            if hi < lo + CHUNK and (l, t, lo, hi) not in ragged:
                ragged.append((l, t, lo, hi))
            acc = carry[t - 1] if (carry is not None and t) else 0
            if t:
                carries[l].append(acc)
            for i in range(lo, hi):
                steps.append((l, "apply", t, i, i == lo, classify_step(acc, src[i])))
                acc = (acc + src[i]) % R
                out[i] = acc
        scanned[l] = out
    return scanned[0], steps, {"sizes": sizes, "totals": totals, "carries": carries, "ragged": ragged, "scanned": scanned}


# What the one chunk at the top holds when it has 2 entries: too few steps for every kind, so the three k with a top of 2 take
# one each. [0, t]: adding the identity, then into the identity behind a chunk's first step. [t, t]: doubling. [t, -t]: cancelling.
TOP_OF_2 = {5: "zero_first", 9: "double", 13: "cancel"}


def _top_values(k, size, rnd):
    t = _rand_fr(rnd)
    if size == 4:  # adding the identity; into the identity at step 1; doubling; cancelling: the total is the identity
        return [0, t, t, (-2 * t) % R]
    assert size == 2
    return {"zero_first": [0, t], "double": [t, t], "cancel": [t, R - t]}[TOP_OF_2[k]]


def _chunk_summing_to(total, carry, t, rnd):
    """16 scalars with this sum. An odd chunk behind a carry c != 0: degenerate from acc = c (what the apply pass sees): c
    (doubling), -2c (cancelling), y (into the identity), 0 (adding the identity). Chunks 2, 6, 10, ...: random. Every other
    chunk, chunk 0 among them: degenerate from acc = 0 (what the total pass sees, and the apply pass where the carry is the
    identity): x, x, -2x, y, 0. The last entry makes the sum."""
    x, y = _rand_fr(rnd), _rand_fr(rnd)
    if t % 2 == 1 and carry:
        head = [carry, (-2 * carry) % R, y, 0]
    elif t % 4 == 2:
        head = []
    else:
        head = [x, x, (-2 * x) % R, y, 0]
    body = head + [_rand_fr(rnd) for _ in range(CHUNK - 1 - len(head))]
    return body + [(total - sum(body)) % R]


def prefix_degenerate_scalars(k, seed=77):
    """a_i (n = 2^k, k in 5, 9, 10, 13) built from the top: the top chunk's values are chosen (_top_values), and every level
    below is filled chunk by chunk so that chunk t sums to the value above it (_chunk_summing_to)."""
    import numpy as np
    rnd = np.random.RandomState(seed + k)
    sizes = prefix_level_sizes(1 << k)
    assert sizes[-1] in (2, 4), "this construction is for sizes whose top chunk is ragged"
    level = _top_values(k, sizes[-1], rnd)
    for size in reversed(sizes[:-1]):
        assert size == CHUNK * len(level)
        lower, carry = [], 0
        for t, total in enumerate(level):
            lower += _chunk_summing_to(total, carry, t, rnd)
            carry = (carry + total) % R
        level = lower
    return level


def prefix_coverage(steps, info):
    """{(level, pass): {kind: count}}. A chunk's first step from acc = 0 is into_identity whatever the data are, so an
    into_identity counts only behind a chunk's first step."""
    cov = {}
    for level, pas, t, i, first, kind in steps:
        if first and kind == "into_identity":
            continue
        cov.setdefault((level, pas), dict.fromkeys(STEP_KINDS, 0))[kind] += 1
    return cov


def prefix_rows_to_read(steps, info, cap=64):
    """Rows i of level 0 whose S_i a test reads one by one: the scanned value at every level's chunk edges (first, last of the
    first chunk, first of the second, last of the last-but-one, last) and at the degenerate steps of each (level, pass), the
    first of each kind. A scanned value at index j of level l is S at row (j + 1) * 16^l - 1."""
    sizes = info["sizes"]
    n = sizes[0]
    rows = []

    def add(level, j):
        r = (j + 1) * CHUNK ** level - 1
        if 0 <= r < n and r not in rows:
            rows.append(r)

    for l, m in enumerate(sizes):
        for j in (0, CHUNK - 1, CHUNK, CHUNK + 1, m - CHUNK - 1, m - CHUNK, m - 2, m - 1):
            if 0 <= j < m:
                add(l, j)
    seen = set()
    for level, pas, t, i, first, kind in steps:
        if kind != "general" and (level, pas, kind) not in seen and not (first and kind == "into_identity"):
            seen.add((level, pas, kind))
            add(level, i)
    assert len(rows) <= cap, len(rows)
    return sorted(rows)
