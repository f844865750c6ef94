"""Shared model of the 9 x 29-bit field arithmetic (csrc/fp29.cuh) for tests/test_fp29_asm_text.py (CPU: the text of
the asm products under an instruction emulator) and tests/test_gpu_field_ops.py (GPU: the compiled functions).
Plain Python integers only.

Reference A — integers mod p: what every function means (`val`, `mont_mul`, `affine_add`, ...).
Reference B — the column algorithms of fp29.cuh restated statement for statement on limb lists, every documented
precondition an assertion (ContractError) and every machine accumulator checked against its width (OverflowError_):
what the device has to return limb for limb ("same values", fp29.cuh).
Operand classes — deterministic limb vectors at the places where a lazily reduced Montgomery product goes wrong."""
import random

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MASK = (1 << 29) - 1
M32 = (1 << 32) - 1
RADIX = 1 << 261


class ContractError(AssertionError):
    """An operand outside the documented precondition of the function it was given to."""


class OverflowError_(AssertionError):
    """A machine accumulator of the restated algorithm left its width."""


def require(cond, what):
    if not cond:
        raise ContractError(what)


def digits(v):
    d = [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]
    assert val(d) == v
    return d


def val(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def words(v):  # packed 8 x u32, little endian
    assert 0 <= v < 1 << 256
    return [(v >> (32 * i)) & M32 for i in range(8)]


def from_words(w):
    return sum(x << (32 * i) for i, x in enumerate(w))


class Field:
    def __init__(self, tag, struct, packed_struct, p):
        self.tag, self.struct, self.packed_struct, self.p = tag, struct, packed_struct, p
        self.P = digits(p)
        self.pinv = (-pow(p, -1, 1 << 29)) % (1 << 29)
        self.recip42 = (1 << 42) // ((p >> 232) + 1)
        self.one = digits(RADIX % p)
        self.k_in = digits((1 << 266) % p)
        self.k_out = digits((1 << 256) % p)
        self.rinv = pow(RADIX, -1, p)
        self.max_acc = 0  # largest accumulator value reference B has seen since the last reset

    def c(self, k):  # k*p, every digit but the top raised by 2^30, compensated by -2 in the next
        d = digits(k * self.p)
        return [d[0] + (1 << 30)] + [d[i] + (1 << 30) - 2 for i in range(1, 8)] + [d[8] - 2]

    def __repr__(self):
        return self.tag


FQ = Field("FQ", "Fq29P", "FqP", Q)
FR = Field("FR", "Fr29P", "FrP", R)
FIELDS = {"FQ": FQ, "FR": FR}


# ------------------------------------------------------------------------------------------ reference A
def mont_mul(F, a, b):
    return a * b * F.rinv % F.p


def mont_mul2(F, a, b, c, d):
    return (a * b + c * d) * F.rinv % F.p


def mont_redc(F, t):
    return t * F.rinv % F.p


def affine_add(P1, P2):
    """y^2 = x^3 + 3 over Fq, None = the identity."""
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return x3, (lam * (x1 - x3) - y1) % Q


def affine_neg(P1):
    return None if P1 is None else (P1[0], (-P1[1]) % Q)


def affine_mul(k, P1):
    acc = None
    while k:
        if k & 1:
            acc = affine_add(acc, P1)
        P1 = affine_add(P1, P1)
        k >>= 1
    return acc


G1 = (1, 2)


def on_curve(P1):
    return P1 is None or (P1[1] * P1[1] - P1[0] ** 3 - 3) % Q == 0


# ------------------------------------------------------------------------------------------ reference B
def _acc(F, acc):
    if acc >> 64:
        raise OverflowError_("64-bit accumulator overflow: 2^%.3f" % _log2(acc))
    if acc > F.max_acc:
        F.max_acc = acc
    return acc


def _log2(v):
    import math
    return math.log2(v) if v else 0.0


def _u32(v, what):
    if not 0 <= v <= M32:
        raise OverflowError_("32-bit limb wraps in " + what)
    return v


def mul_admits(F, a, b):
    """The documented contract of f29_mul: both operands with limbs below 2^30, or one below 2.5 * 2^30 (f29_sub10_lazy,
    f29_sub10_lazy2) and the other normalised; a*b < 169 p^2."""
    ma, mb = max(a), max(b)
    require((ma < 1 << 30 and mb < 1 << 30) or (ma < 0xA0000000 and mb < 1 << 29) or (mb < 0xA0000000 and ma < 1 << 29), "mul: limbs out of range")
    require(val(a) * val(b) < 169 * F.p * F.p, "mul: a*b >= 169 p^2")


def sqr_admits(F, a):
    require(all(x < 1 << 29 for x in a[:8]), "sqr: operand not normalised")
    require(a[8] <= M32 and val(a) ** 2 < 169 * F.p * F.p, "sqr: a*a >= 169 p^2")


def mul2_admits(F, a, b, c, d):
    require(all(x < 1 << 29 for x in a[:8] + c[:8] + d[:8]) and all(x < 1 << 31 for x in b[:8]), "mul2: operand not normalised")
    require(max(a[8], b[8], c[8], d[8]) <= M32, "mul2: top limb")
    require(val(a) * val(b) + val(c) * val(d) < 169 * F.p * F.p, "mul2: a*b + c*d >= 169 p^2")


def _montgomery_columns(F, column):
    """The shared skeleton of f29_mul / f29_sqr / f29_mul2 / f29_wide_redc: `column(k)` is the sum of the partial products
    (or the carried column) that enters column k; returns (limbs, Montgomery factors)."""
    m, r, acc = [0] * 9, [0] * 9, 0
    for k in range(9):
        for t in column(k):
            acc = _acc(F, acc + t)
        for i in range(k):
            acc = _acc(F, acc + m[i] * F.P[k - i])
        m[k] = ((acc & M32) * F.pinv) & MASK  # f29_mulq: 32-bit product, masked
        acc = _acc(F, acc + m[k] * F.P[0])
        acc >>= 29
    for k in range(9, 17):
        for t in column(k):
            acc = _acc(F, acc + t)
        for i in range(k - 8, 9):
            acc = _acc(F, acc + m[i] * F.P[k - i])
        r[k - 9] = acc & MASK
        acc >>= 29
    r[8] = acc & M32  # (uint32_t)acc
    if acc >> 32:
        raise OverflowError_("top limb of a product does not fit 32 bits")
    return r, m


def _idx(k):
    return range(max(0, k - 8), min(k, 8) + 1)


def f29_mul(F, a, b, with_m=False):
    mul_admits(F, a, b)
    r, m = _montgomery_columns(F, lambda k: [a[i] * b[k - i] for i in _idx(k)])
    return (r, m) if with_m else r


def f29_sqr(F, a, with_m=False):
    sqr_admits(F, a)
    d = [(x << 1) & M32 for x in a]

    def column(k):
        t = [a[i] * d[k - i] for i in _idx(k) if 2 * i < k]
        if k % 2 == 0:
            t.append(a[k // 2] * a[k // 2])
        return t
    r, m = _montgomery_columns(F, column)
    return (r, m) if with_m else r


def f29_mul2(F, a, b, c, d):
    mul2_admits(F, a, b, c, d)
    return _montgomery_columns(F, lambda k: [a[i] * b[k - i] for i in _idx(k)] + [c[i] * d[k - i] for i in _idx(k)])[0]


def f29_wide_zero():
    return [0] * 17


def f29_wide_madd(F, w, a, b):
    require(all(x < 1 << 29 for x in a) and all(x < 1 << 29 for x in b), "wide_madd: operand not normalised")
    for k in range(17):
        for i in _idx(k):
            w[k] = _acc(F, w[k] + a[i] * b[k - i])


def f29_wide_carry(F, w):
    for k in range(16):
        w[k + 1] = _acc(F, w[k + 1] + (w[k] >> 29))
        w[k] &= MASK


def f29_wide_redc(F, w):
    require(all(x < 1 << 29 for x in w[:16]), "wide_redc: columns not carried")
    return _montgomery_columns(F, lambda k: [w[k]])[0]


def f29_norm(v):
    v = list(v)
    for i in range(8):
        v[i + 1] = _u32(v[i + 1] + (v[i] >> 29), "norm")
        v[i] &= MASK
    return v


def f29_add_lazy(a, b):
    return [_u32(x + y, "add_lazy") for x, y in zip(a, b)]


def f29_add(a, b):
    return f29_norm(f29_add_lazy(a, b))


def _diff(F, K, a, b, what):
    c = F.c(K)
    require(b[8] <= c[8], what + ": subtrahend too large for this constant")
    return [_u32(x + ck - y, what) for x, ck, y in zip(a, c, b)]


def f29_sub(F, K, a, b):
    """a - b + K p, normalised (K in 3, 5, 6, 7, 8, 10)."""
    require(all(x < 1 << 29 for x in a[:8] + b[:8]), "sub: operand not normalised")
    return f29_norm(_diff(F, K, a, b, "sub"))


def f29_neg(F, K, b):
    """K p - b, normalised (K in 3, 6, 10)."""
    require(all(x < 1 << 29 for x in b[:8]), "neg: operand not normalised")
    return f29_norm(_diff(F, K, [0] * 9, b, "neg"))


def f29_sub10_lazy(F, a, b):
    require(all(x < 1 << 29 for x in a[:8] + b[:8]), "sub_lazy: operand not normalised")
    return _diff(F, 10, a, b, "sub_lazy")


def f29_sub10_lazy2(F, a, b):
    require(all(x < 1 << 30 for x in a[:8] + b[:8]), "sub_lazy2: operand limbs above 2^30")
    return _diff(F, 10, a, b, "sub_lazy2")


def f29_reduce_weak(F, v):
    require(v[8] < 1 << 29, "reduce_weak: value >= 2^261")
    require(all(x < 1 << 31 for x in v[:8]), "reduce_weak: limb above 2^31")
    q = (v[8] * F.recip42) >> 42
    r, acc = [0] * 9, 0
    for i in range(9):
        acc += v[i] - q * F.P[i]
        if not -(1 << 63) <= acc < 1 << 63:
            raise OverflowError_("reduce_weak: signed accumulator")
        r[i] = (acc & MASK) if i < 8 else (acc & M32)
        if i == 8 and not 0 <= acc <= M32:
            raise OverflowError_("reduce_weak: top limb negative or too wide")
        acc >>= 29  # Python's >> on a negative int is arithmetic, as in the C code
    return r


def f29_is_zero_mod_p(F, v):
    return not any(v) or v == F.P


def f29_unpack(w):
    r = []
    for i in range(9):
        bit = 29 * i
        lo, sh = bit >> 5, bit & 31
        v = w[lo] | ((w[lo + 1] << 32) if lo + 1 < 8 else 0)
        r.append((v >> sh) & MASK)
    return r


def f29_pack_canonical(F, v):
    require(all(x < 1 << 29 for x in v[:8]) and val(v) < 2 * F.p, "pack_canonical: not normalised or not below 2p")
    t, borrow = [0] * 9, 0
    for i in range(9):
        d = (v[i] - F.P[i] - borrow) & M32
        borrow = d >> 31
        t[i] = (d & MASK) if i < 8 else d
    c = v if borrow else t
    out = []
    for j in range(8):
        bit = 32 * j
        i0 = bit // 29
        sh = bit - 29 * i0
        w = (c[i0] >> sh) | (c[i0 + 1] << (29 - sh))
        if i0 + 2 < 9:
            w |= c[i0 + 2] << (58 - sh)
        out.append(w & M32)
    return out


def f29_shl5(v):
    r = [(v[0] << 5) & MASK]
    for i in range(1, 8):
        r.append(((v[i] << 5) | (v[i - 1] >> 24)) & MASK)
    r.append(_u32((v[8] << 5) | (v[7] >> 24), "shl5"))
    return r


def fq29_from_r256(x):
    return f29_mul(FQ, f29_unpack(x), FQ.k_in)


def fq29_to_r256(v):
    return f29_pack_canonical(FQ, f29_mul(FQ, v, FQ.k_out))


def fr29_mul_const(x, c261):
    return f29_pack_canonical(FR, f29_mul(FR, f29_unpack(x), f29_unpack(c261)))


fr29_mul_rr = fr29_mul_const  # the same statements; the radices of the operands differ, not the code


def fr29_mul_std(a, b):
    return f29_pack_canonical(FR, f29_mul(FR, f29_unpack(a), f29_shl5(f29_unpack(b))))


def fr29_from_mont(x):
    return f29_pack_canonical(FR, f29_mul(FR, f29_unpack(x), [32] + [0] * 8))


def fr29_inv(x):
    a = f29_mul(FR, f29_unpack(x), FR.k_in)
    r, started = list(FR.one), False
    pw = words(R)
    for limb in range(7, -1, -1):
        w = pw[limb] - 2 if limb == 0 else pw[limb]
        for b in range(31, -1, -1):
            if started:
                r = f29_sqr(FR, r)
            if (w >> b) & 1:
                r = f29_mul(FR, r, a)
                started = True
    return f29_pack_canonical(FR, f29_mul(FR, r, FR.k_out))


# ---- XYZZ on Fq29, statement for statement; a point is (x, y, zz, zzz) of limb lists, the identity has zz all zero
def x29_inf():
    return ([0] * 9, [0] * 9, [0] * 9, [0] * 9)


def x29_dbl_affine(qx, qy):
    F = FQ
    u = f29_add(qy, qy)
    v = f29_sqr(F, u)
    w = f29_mul(F, u, v)
    s = f29_mul(F, qx, v)
    xx = f29_sqr(F, qx)
    m = f29_add(f29_add_lazy(xx, xx), xx)
    rx = f29_sub(F, 5, f29_sqr(F, m), f29_add(s, s))
    d = f29_sub(F, 8, s, rx)
    ry = f29_mul2(F, m, d, f29_neg(F, 3, w), qy)
    return (rx, ry, v, w)


def x29_add_affine(a, qx, qy, q_inf):
    F = FQ
    if q_inf:
        return a
    if not any(a[2]):
        return (list(qx), list(qy), list(F.one), list(F.one))
    ax, ay, azz, azzz = a
    u2 = f29_mul(F, qx, azz)
    s2 = f29_mul(F, qy, azzz)
    p = f29_sub(F, 10, u2, ax)
    r = f29_sub(F, 6, s2, ay)
    pp = f29_sqr(F, p)
    rr = f29_sqr(F, r)
    if f29_is_zero_mod_p(F, pp):
        if f29_is_zero_mod_p(F, rr):
            return x29_dbl_affine(qx, qy)
        return x29_inf()
    ppp = f29_mul(F, p, pp)
    q = f29_mul(F, ax, pp)
    s = f29_add(ppp, f29_add_lazy(q, q))
    ox = f29_sub(F, 7, rr, s)
    t = f29_sub10_lazy(F, q, ox)
    oy = f29_mul2(F, r, t, f29_neg(F, 6, ay), ppp)
    return (ox, oy, f29_mul(F, azz, pp), f29_mul(F, azzz, ppp))


def x29_dbl(pt):
    F = FQ
    if not any(pt[2]):
        return pt
    px, py, pzz, pzzz = pt
    u = f29_add(py, py)
    v = f29_sqr(F, u)
    w = f29_mul(F, u, v)
    s = f29_mul(F, px, v)
    xx = f29_sqr(F, px)
    m = f29_add(f29_add_lazy(xx, xx), xx)
    rx = f29_sub(F, 5, f29_sqr(F, m), f29_add(s, s))
    d = f29_sub(F, 8, s, rx)
    ry = f29_mul2(F, m, d, f29_neg(F, 3, w), py)
    return (rx, ry, f29_mul(F, v, pzz), f29_mul(F, w, pzzz))


def x29_add(a, b):
    F = FQ
    if not any(b[2]):
        return a
    if not any(a[2]):
        return b
    u1 = f29_mul(F, a[0], b[2])
    u2 = f29_mul(F, b[0], a[2])
    s1 = f29_mul(F, a[1], b[3])
    s2 = f29_mul(F, b[1], a[3])
    p = f29_sub(F, 3, u2, u1)
    r = f29_sub(F, 3, s2, s1)
    pp = f29_sqr(F, p)
    rr = f29_sqr(F, r)
    if f29_is_zero_mod_p(F, pp):
        if f29_is_zero_mod_p(F, rr):
            return x29_dbl(a)
        return x29_inf()
    ppp = f29_mul(F, p, pp)
    q = f29_mul(F, u1, pp)
    s = f29_add(ppp, f29_add_lazy(q, q))
    ox = f29_sub(F, 7, rr, s)
    t = f29_sub10_lazy(F, q, ox)
    oy = f29_mul2(F, r, t, f29_neg(F, 3, s1), ppp)
    return (ox, oy, f29_mul(F, f29_mul(F, a[2], b[2]), pp), f29_mul(F, f29_mul(F, a[3], b[3]), ppp))


# ---- the same formulas spread over the four lanes of a quad (csrc/fp29_quad.cuh). Lane `role` multiplies the role-th pair of
# every round (quad_sel) and a broadcast (quad_bcast<J>) is lane J's product, so reference B evaluates all four products of
# a round — the duplicates that fill idle lanes too: every f29_mul precondition of every lane is enforced — and the four
# lanes end with the same point.
def _quad_round(F, a4, b4):
    return [f29_mul(F, a, b) for a, b in zip(a4, b4)]


def x29_dbl_quad(pt):
    F = FQ
    if not any(pt[2]):
        return pt
    px, py, pzz, pzzz = pt
    u = f29_add(py, py)
    res = _quad_round(F, (u, px, u, px), (u, px, u, px))
    v, xx = res[0], res[1]
    m = f29_add(f29_add_lazy(xx, xx), xx)
    res = _quad_round(F, (u, px, m, m), (v, v, m, m))
    w, sv, mm = res[0], res[1], res[2]
    rx = f29_sub(F, 5, mm, f29_add(sv, sv))
    d = f29_sub(F, 8, sv, rx)
    res = _quad_round(F, (m, f29_neg(F, 3, w), v, w), (d, py, pzz, pzzz))
    return (rx, f29_add(res[0], res[1]), res[2], res[3])


def x29_add_quad(a, b):
    F = FQ
    if not any(b[2]):
        return a
    if not any(a[2]):
        return b
    res = _quad_round(F, (a[0], b[0], a[1], b[1]), (b[2], a[2], b[3], a[3]))
    u1, s1 = res[0], res[2]
    p = f29_sub(F, 3, res[1], u1)
    r = f29_sub(F, 3, res[3], s1)
    res = _quad_round(F, (p, r, a[2], a[3]), (p, r, b[2], b[3]))
    pp, rr, zz12, zzz12 = res
    if f29_is_zero_mod_p(F, pp):
        if f29_is_zero_mod_p(F, rr):
            return x29_dbl_quad(a)
        return x29_inf()
    res = _quad_round(F, (p, u1, zz12, zz12), (pp, pp, pp, pp))
    ppp, q, ozz = res[0], res[1], res[2]
    sq = f29_add(ppp, f29_add_lazy(q, q))
    ox = f29_sub(F, 7, rr, sq)
    t = f29_sub(F, 10, q, ox)
    res = _quad_round(F, (r, f29_neg(F, 3, s1), zzz12, zzz12), (t, ppp, ppp, ppp))
    return (ox, f29_add(res[0], res[1]), ozz, res[2])


def x29_to_r256(a):
    if not any(a[2]):
        return [0] * 32
    return sum((fq29_to_r256(c) for c in a), [])


def x29_affine(a):
    """Reference A's view of an XYZZ point in radix 2^261: (x, y) as plain integers, None for the identity."""
    if not any(a[2]):
        return None
    x, y, zz, zzz = (val(c) * FQ.rinv % Q for c in a)
    return x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q


def xyzz_words_affine(w):
    """The same for a packed radix-2^256 G1X (32 words)."""
    x, y, zz, zzz = (from_words(w[8 * i:8 * i + 8]) for i in range(4))
    if zz == 0:
        return None
    return x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q  # the radix cancels in both quotients


def affine_to_r261(P1):
    return digits(P1[0] * RADIX % Q), digits(P1[1] * RADIX % Q)


# ------------------------------------------------------------------------------------------ operand classes
def _top_for(low, v):
    """Limbs `low` (eight) plus the largest top limb that keeps the value <= v."""
    t = (v - val(low)) >> 232
    assert t >= 0
    return list(low) + [t]


def _fill_b(F, a, low_b):
    """b with limbs 0..7 = low_b and the largest top limb with a*b < 169 p^2; also the same one step outside."""
    b = _top_for(low_b, (169 * F.p * F.p - 1) // val(a))
    out = b[:8] + [b[8] + 1]
    assert val(a) * val(b) < 169 * F.p * F.p <= val(a) * val(out)
    return b, out


def canonical(F, rnd):
    return digits(rnd.randrange(F.p))


def class_small(F):
    """Class 1: named values (products return values in [p, 2p), consumers must take them) and Montgomery forms."""
    p = F.p
    vs = [0, 1, 2, p - 1, p, p + 1, 2 * p - 1, 0, RADIX % p, (-RADIX) % p]
    return [digits(v) for v in vs]


def class_random(F, n, seed):
    rnd = random.Random(seed)
    return [(canonical(F, rnd), canonical(F, rnd)) for _ in range(n)]


def class_one_hot(F):
    """Class 2: limb i = 2^29 - 1 and the rest 0 on one side, limb j on the other: every a_i * b_j alone in its column."""
    hot = [[MASK if j == i else 0 for j in range(9)] for i in range(9)]
    out = []
    for a in hot:
        for b in hot:
            if val(a) * val(b) < 169 * F.p * F.p:  # limb 8 = 2^29 - 1 on both sides is 169 p * 169 p: outside the contract
                out.append((a, b))
    return out


def class_bound_pairs(F, limb):
    """Classes 3 (limb = 2^29 - 1) and 4 (limb = 2^30 - 1): limbs 0..7 all `limb`, values near 13p x 13p and 16p x 10.5p,
    just inside a*b < 169 p^2; returns (inside pairs, outside pairs)."""
    low = [limb] * 8
    inside, outside = [], []
    for va in (13 * F.p, 16 * F.p - 1):
        a = _top_for(low, va)
        assert val(a) < 16 * F.p and a[8] < 1 << 26
        b, bo = _fill_b(F, a, low)
        assert val(b) < 16 * F.p and b[8] < 1 << 26
        inside += [(a, b), (b, a)]
        outside += [(a, bo), (bo, a)]
    return inside, outside


def class_sqr_bound(F):
    """The largest normalised operand of the square (a*a < 169 p^2, limbs 0..7 = 2^29 - 1) and one step outside."""
    low = [MASK] * 8
    import math
    a = _top_for(low, math.isqrt(169 * F.p * F.p - 1))
    out = a[:8] + [a[8] + 1]
    assert val(a) ** 2 < 169 * F.p * F.p <= val(out) ** 2
    return a, out


def class_lazy_mul(F):
    """Class 5 for f29_mul: one operand with limbs 0..7 at the top of the f29_sub10_lazy2 range (0x9FFFFFFF, which also
    covers f29_sub10_lazy's), the other normalised, a*b just under 169 p^2. [(a, b), (b, a)] and the outside pairs."""
    inside, outside = [], []
    for lim, va in ((0x9FFFFFFF, 12 * F.p), (0x7FFFFFFF, 12 * F.p), (0x9FFFFFFF, 16 * F.p - 1)):
        a = _top_for([lim] * 8, va)
        b, bo = _fill_b(F, a, [MASK] * 8)
        inside += [(a, b), (b, a)]
        outside += [(a, bo)]
    return inside, outside


def class_lazy_mul2(F):
    """Class 5 for f29_mul2: b from the f29_sub10_lazy range (limbs below 2^31), a, c, d normalised at 2^29 - 1,
    a*b + c*d just under 169 p^2."""
    low = [MASK] * 8
    a = _top_for(low, 8 * F.p)
    b = _top_for([(1 << 31) - 1] * 8, 12 * F.p)
    c = _top_for(low, 6 * F.p)
    room = 169 * F.p * F.p - 1 - val(a) * val(b)
    d = _top_for(low, room // val(c))
    do = d[:8] + [d[8] + 1]
    assert val(a) * val(b) + val(c) * val(d) < 169 * F.p * F.p <= val(a) * val(b) + val(c) * val(do)
    return (a, b, c, d), (a, b, c, do)


def class_m_factor(F, seed=29):
    """Class 6: for every k and for t in (0, 2^29 - 1) a pair whose Montgomery factor m_k is t. m_k is linear in a_k modulo
    2^29 (a_k enters column k for the first time, times b_0, b_0 odd): solve, do not search. For k = 8 bases are drawn
    until the solution keeps the value below 16p (limb 8 below 2^26)."""
    rnd = random.Random(seed)
    out = []
    for k in range(9):
        for t in (0, MASK):
            while True:
                a, b = canonical(F, rnd), canonical(F, rnd)
                b[0] |= 1
                a[k] = 0
                m0 = f29_mul(F, a, b, with_m=True)[1][k]
                a[k] = (t - m0) * pow(b[0] * F.pinv, -1, 1 << 29) % (1 << 29)
                if k < 8 or a[8] < 1 << 26:
                    break
            assert f29_mul(F, a, b, with_m=True)[1][k] == t
            out.append((k, t, a, b))
    return out


def class_m_factor_sqr(F, seed=31):
    """Class 6 for the square: a_k enters column k as 2 a_0 a_k, so with a_0 odd every m_k of the right parity can be
    reached; bases are drawn until it fits (k = 0: a_0 = 0 gives m_0 = 0; m_0 = 2^29 - 1 needs a_0^2 = p_0 mod 2^29,
    which exists only for p_0 = 1 mod 8: the scalar field, not the base field)."""
    rnd = random.Random(seed)
    out = [(0, 0, [0] + canonical(F, rnd)[1:])]
    if F.P[0] % 8 == 1:  # lift the square root of p_0 from modulo 8 to modulo 2^29, one bit at a time
        a0 = 1
        for bits in range(4, 30):
            if (a0 * a0 - F.P[0]) % (1 << bits):
                a0 += 1 << (bits - 2)
        a = [a0] + canonical(F, rnd)[1:]
        assert f29_sqr(F, a, with_m=True)[1][0] == MASK
        out.append((0, MASK, a))
    lim8 = class_sqr_bound(F)[0][8]
    for k in range(1, 9):
        for t in (0, MASK):
            for _ in range(4000):
                a = canonical(F, rnd)
                a[0] |= 1
                a[k] = 0
                m0 = f29_sqr(F, a, with_m=True)[1][k]
                if (t - m0) % 2:
                    continue
                half = pow(a[0] * F.pinv, -1, 1 << 28)
                a[k] = ((t - m0) // 2 % (1 << 28)) * half % (1 << 28)
                if k == 8 and a[8] >= lim8:
                    continue
                if f29_sqr(F, a, with_m=True)[1][k] == t:
                    out.append((k, t, a))
                    break
            else:
                raise AssertionError("no square operand with m_%d = %#x" % (k, t))
    return out


WIDE_GROUP = 6  # terms between two f29_wide_carry calls: the documented limit and what the interpreter uses


def wide_sum(F, pairs, nterms):
    """Reference B for the wide accumulator as the h(X) interpreter drives it: term j is pairs[j % len(pairs)], a carry
    pass after every sixth term and before the reduction. Returns (result limbs, integer T)."""
    w, T = f29_wide_zero(), 0
    for j in range(nterms):
        a, b = pairs[j % len(pairs)]
        f29_wide_madd(F, w, a, b)
        T += val(a) * val(b)
        if j % WIDE_GROUP == WIDE_GROUP - 1:
            f29_wide_carry(F, w)
    f29_wide_carry(F, w)
    assert sum(c << (29 * k) for k, c in enumerate(w)) == T
    return f29_wide_redc(F, w), T


def class_wide(F, seed=37):
    """Class 7: (pairs, nterms). Six terms of all-limbs-2^29-1 operands between carries (the documented limit), and
    canonical operands in the group sizes the interpreter uses (a carry every sixth term; 1, 5, 6, 7, 12, 18 terms)."""
    rnd = random.Random(seed)
    top = [MASK] * 9
    out = [([(top, top)] * 6, 6), ([(top, top)] * 6, 5)]
    for n in (1, 5, 6, 7, 12, 18):
        out.append(([(canonical(F, rnd), canonical(F, rnd)) for _ in range(6)], n))
    hot = [MASK] * 8 + [F.P[8]]
    out.append(([(hot, hot)] * 6, 18))
    return out


def class_reduce_weak(F, seed=41):
    """Class 8: top limbs where the quotient estimate is exact and where it is one short (every boundary k (p8 + 1) + d
    that tools/gen_fp29_consts.py reasons about, thinned to a few dozen k), lower limbs 0, random normalised, 2^29 - 1 and
    lazy up to 2^31 - 1."""
    rnd = random.Random(seed)
    p8 = F.p >> 232
    tops = [0, 1, p8 - 1, p8, p8 + 1, MASK]
    for k in [1, 2, 3, 12, 13, 16, 17, 84, 85, 167, 168, 169] + [rnd.randrange(1, 170) for _ in range(12)]:
        tops += [k * (p8 + 1) + d for d in (-2, -1, 0, 1, 2, p8)]
    tops = sorted({t for t in tops if 0 <= t < 1 << 29})
    exact = [t for t in tops if (t * F.recip42) >> 42 == t // (p8 + 1)]
    short = [t for t in tops if (t * F.recip42) >> 42 == t // (p8 + 1) - 1]
    assert exact and short and len(exact) + len(short) == len(tops)
    out = []
    for t in tops:
        for low in ([0] * 8, [MASK] * 8, [(1 << 31) - 1] * 8, [rnd.randrange(1 << 29) for _ in range(8)], [rnd.randrange(1 << 31) for _ in range(8)]):
            out.append(low + [t])
    return out


def class_points(seed=43, n=6):
    """Class 9 raw material: n random affine points (multiples of the generator)."""
    rnd = random.Random(seed)
    pts = [affine_mul(rnd.randrange(1, R), G1) for _ in range(n)]
    assert all(on_curve(P1) for P1 in pts) and affine_mul(R, G1) is None
    return pts


# ------------------------------------------------------------------------------------------ cases
# One case = one call of one harness function (tests/native/fp29_device_check.hip): the words that go in, what reference
# B says comes out, and reference A's judgement of any output (`check`). The CPU suite runs `check` on B's output; the GPU
# suite compares the device's words with B's, then runs `check` on them.
IN_WORDS, OUT_WORDS = 112, 320  # data words of one record (the largest: six operand pairs in; eight XYZZ points out)
(F_MUL, F_SQR, F_MUL2, F_MUL_CHAIN, F_SQR_CHAIN, F_MUL2_CHAIN, F_WIDE, F_REDUCE_WEAK, F_SUB_MUL, F_NEG_MUL2, F_LAZY_MUL,
 F_LAZY2_MUL, F_LAZY_MUL2, F_UNPACK_PACK, F_FROM_TO_R256, F_TO_R256, F_MUL_CONST, F_MUL_RR, F_MUL_STD, F_FROM_MONT, F_INV29,
 F_BN_MUL, F_BN_INV, F_DBL_AFFINE, F_ADD_AFFINE, F_DBL, F_ADD, F_ADD_CHAIN, F_DBL_QUAD, F_ADD_QUAD, F_QUAD_CHAIN) = range(1, 32)
FUNC_NAMES = {v: k[2:].lower() for k, v in list(globals().items()) if k.startswith("F_") and isinstance(v, int)}
CHAIN_STEPS, CHAIN_EVERY = 64, 8
QUAD_FUNCS = (F_DBL_QUAD, F_ADD_QUAD, F_QUAD_CHAIN)  # one record per QUAD of lanes (the others: one record per lane)
AUX_SIT_OUT = 1  # quad functions: this record's quad does not call the formula and writes nothing
QUAD_CHAIN_STEPS, QUAD_CHAIN_EVERY = 16, 4


class Case:
    def __init__(self, func, F, what, data, expect, check, aux=0):
        assert len(data) <= IN_WORDS and len(expect) <= OUT_WORDS and all(0 <= x <= M32 for x in data + expect)
        self.func, self.F, self.what, self.data, self.expect, self.check, self.aux = func, F, what, list(data), list(expect), check, aux

    def describe(self):
        return "%s %s [%s] aux=%d in=%s" % (FUNC_NAMES[self.func], self.F.tag, self.what, self.aux, " ".join("%08x" % x for x in self.data))


def _vecs(out, n=9):
    return [out[i:i + n] for i in range(0, len(out), n)]


def _is_product(F, r, want, bound=2):
    assert all(x < 1 << 29 for x in r[:8]), "result not normalised"
    assert val(r) < bound * F.p, "result not below %sp" % bound
    assert val(r) % F.p == want % F.p, "wrong residue"


def _chain(F, step, first, check_residue):
    """64 dependent applications of `step`, a checkpoint at every eighth."""
    r, a, outs, wants = first, val(first), [], []
    for n in range(1, CHAIN_STEPS + 1):
        r, a = step(r), check_residue(a)
        if n % CHAIN_EVERY == 0:
            outs += r
            wants.append(a)

    def check(out):
        for r_, w in zip(_vecs(out), wants):
            _is_product(F, r_, w)
    return outs, check


def case_mul(F, what, a, b):
    return Case(F_MUL, F, what, a + b, f29_mul(F, a, b), lambda o: _is_product(F, o, mont_mul(F, val(a), val(b))))


def case_sqr(F, what, a):
    return Case(F_SQR, F, what, a, f29_sqr(F, a), lambda o: _is_product(F, o, mont_mul(F, val(a), val(a))))


def case_mul2(F, what, a, b, c, d):
    return Case(F_MUL2, F, what, a + b + c + d, f29_mul2(F, a, b, c, d), lambda o: _is_product(F, o, mont_mul2(F, val(a), val(b), val(c), val(d))))


def case_mul_chain(F, what, a, b):
    outs, check = _chain(F, lambda r: f29_mul(F, r, b), a, lambda x: mont_mul(F, x, val(b)))
    return Case(F_MUL_CHAIN, F, what, a + b, outs, check)


def case_sqr_chain(F, what, a):
    outs, check = _chain(F, lambda r: f29_sqr(F, r), a, lambda x: mont_mul(F, x, x))
    return Case(F_SQR_CHAIN, F, what, a, outs, check)


def case_mul2_chain(F, what, a, b, c, d):
    outs, check = _chain(F, lambda r: f29_mul2(F, r, b, c, d), a, lambda x: mont_mul2(F, x, val(b), val(c), val(d)))
    return Case(F_MUL2_CHAIN, F, what, a + b + c + d, outs, check)


def case_wide(F, what, pairs, nterms):
    assert len(pairs) == 6
    r, T = wide_sum(F, pairs, nterms)

    def check(o):
        assert all(x < 1 << 29 for x in o[:8]) and val(o) < T // RADIX + F.p + 1 and val(o) % F.p == mont_redc(F, T)
    return Case(F_WIDE, F, what, sum((a + b for a, b in pairs), []), r, check, aux=nterms)


def case_reduce_weak(F, what, v):
    def check(o):
        assert all(x < 1 << 29 for x in o[:8]) and val(o) % F.p == val(v) % F.p
        assert val(o) * 10000 < 10003 * F.p, "reduce_weak: result not below 1.0003 p"
        if all(x < 1 << 29 for x in v):
            assert val(o) * 10000 < 10002 * F.p, "reduce_weak: normalised operand, result not below 1.0002 p"
    return Case(F_REDUCE_WEAK, F, what, v, f29_reduce_weak(F, v), check)


def case_sub_mul(F, what, K, a, b, c):
    d = f29_sub(F, K, a, b)

    def check(o):
        d_, r_ = _vecs(o)
        assert all(x < 1 << 29 for x in d_[:8]) and val(d_) == val(a) - val(b) + K * F.p
        _is_product(F, r_, mont_mul(F, val(a) - val(b), val(c)))
    return Case(F_SUB_MUL, F, what, a + b + c, d + f29_mul(F, d, c), check, aux=K)


def case_neg_mul2(F, what, K, a, b, c, d):
    n = f29_neg(F, K, c)

    def check(o):
        n_, r_ = _vecs(o)
        assert all(x < 1 << 29 for x in n_[:8]) and val(n_) == K * F.p - val(c)
        _is_product(F, r_, mont_mul2(F, val(a), val(b), -val(c), val(d)))
    return Case(F_NEG_MUL2, F, what, a + b + c + d, n + f29_mul2(F, a, b, n, d), check, aux=K)


def case_lazy_mul(F, what, a, b, c):
    d = f29_sub10_lazy(F, a, b)

    def check(o):
        d_, r_ = _vecs(o)
        assert max(d_[:8]) < 1 << 31 and val(d_) == val(a) - val(b) + 10 * F.p
        _is_product(F, r_, mont_mul(F, val(a) - val(b), val(c)))
    return Case(F_LAZY_MUL, F, what, a + b + c, d + f29_mul(F, d, c), check)


def case_lazy2_mul(F, what, a, b, c, d, e):
    s0, s1 = f29_add_lazy(a, b), f29_add_lazy(c, d)
    t = f29_sub10_lazy2(F, s0, s1)

    def check(o):
        t_, r_ = _vecs(o)
        assert max(t_[:8]) < 0xA0000000 and val(t_) == val(a) + val(b) - val(c) - val(d) + 10 * F.p
        _is_product(F, r_, mont_mul(F, val(a) + val(b) - val(c) - val(d), val(e)))
    return Case(F_LAZY2_MUL, F, what, a + b + c + d + e, t + f29_mul(F, t, e), check)


def case_lazy_mul2(F, what, a, b, c, d, e):
    t = f29_sub10_lazy(F, b, c)
    return Case(F_LAZY_MUL2, F, what, a + b + c + d + e, f29_mul2(F, a, t, d, e),
                lambda o: _is_product(F, o, mont_mul2(F, val(a), val(b) - val(c), val(d), val(e))))


def case_unpack_pack(F, what, x):
    u = f29_unpack(words(x))

    def check(o):
        assert val(o[:9]) == x and all(v < 1 << 29 for v in o[:9]) and from_words(o[9:17]) == x % F.p
    return Case(F_UNPACK_PACK, F, what, words(x), u + f29_pack_canonical(F, u), check)


def case_from_to_r256(what, x):
    v = fq29_from_r256(words(x))

    def check(o):
        _is_product(FQ, o[:9], x * 32)
        assert from_words(o[9:17]) == x
    return Case(F_FROM_TO_R256, FQ, what, words(x), v + fq29_to_r256(v), check)


def case_to_r256(what, v):
    return Case(F_TO_R256, FQ, what, v, fq29_to_r256(v), lambda o: _eq(from_words(o), val(v) * pow(32, -1, Q) % Q))


def _eq(got, want):
    assert got == want, "got %x want %x" % (got, want)


R256 = 1 << 256


def case_fr_packed(func, what, x, y=None):
    """The packed scalar-field entry points; x, y canonical integers (the stored 32 bytes)."""
    if func in (F_MUL_CONST, F_MUL_RR):
        B_, want = fr29_mul_const(words(x), words(y)), x * y * FR.rinv % R
    elif func == F_MUL_STD:
        B_, want = fr29_mul_std(words(x), words(y)), x * y * pow(R256, -1, R) % R
    elif func == F_FROM_MONT:
        B_, want = fr29_from_mont(words(x)), x * pow(R256, -1, R) % R
    else:
        B_, want = fr29_inv(words(x)), pow(x, -1, R) * R256 * R256 % R
    return Case(func, FR, what, words(x) + (words(y) if y is not None else []), B_, lambda o: _eq(from_words(o), want))


def case_bn_mul(F, what, a, b):
    """bn254.cuh mul, device branch: the first operand below p, the second any 256-bit value. No limb-exact reference is
    needed: the result is canonical, so reference A alone fixes every bit."""
    want = a * b * pow(R256, -1, F.p) % F.p
    return Case(F_BN_MUL, F, what, words(a) + words(b), words(want), lambda o: _eq(from_words(o), want))


def case_bn_inv(F, what, a):
    want = pow(a, -1, F.p) * R256 * R256 % F.p if a % F.p else 0
    return Case(F_BN_INV, F, what, words(a), words(want), lambda o: _eq(from_words(o), want))


def _pt_words(pt):
    return pt[0] + pt[1] + pt[2] + pt[3]


def _pt_check(want, y_bound=2):
    """y_bound: 2 where y leaves a formula as one reduced product, 4 for the quad formulas (the sum of two), 5 where the
    formula hands a (lifted) operand back unchanged: the documented bound of an accumulator that comes IN."""
    def check(o):
        pt = tuple(_vecs(o[:36]))
        assert x29_affine(pt) == want, "raw XYZZ: wrong point"
        if want is not None:
            assert all(x < 1 << 29 for c in pt for x in c[:8])
            assert val(pt[0]) < 9 * Q and val(pt[1]) < y_bound * Q and max(val(pt[2]), val(pt[3])) < 2 * Q, "outside the accumulator bounds"
        assert xyzz_words_affine(o[36:68]) == want, "packed XYZZ: wrong point"
        assert all(from_words(o[36 + 8 * i:44 + 8 * i]) < Q for i in range(4))
    return check


def x29_from_affine(P1):
    if P1 is None:
        return x29_inf()
    x, y = affine_to_r261(P1)
    return (x, y, list(FQ.one), list(FQ.one))


ACC_BOUNDS = (9, 5, 2, 2)  # fp29.cuh "XYZZ on Fq29": what the formulas accept of an accumulator, in units of p


def x29_lift(pt):
    """The same point with every coordinate at the top of the documented accumulator bounds: the largest v + k p below
    9p / 5p / 2p / 2p, limbs 0..7 normalised. The identity (zz all zero) has one representation and stays."""
    if not any(pt[2]):
        return pt
    out = tuple(digits(val(c) % Q + (b * Q - 1 - val(c) % Q) // Q * Q) for c, b in zip(pt, ACC_BOUNDS))
    assert all((b - 1) * Q <= val(c) < b * Q and max(c[:8]) <= MASK for c, b in zip(out, ACC_BOUNDS))
    return out


def _passes_through(r, operands):
    """The formula returned one of its operands as it came (identity on the other side): the bounds of what came in hold."""
    return any(r == o for o in operands)


def case_dbl_affine(what, P1):
    qx, qy = affine_to_r261(P1)
    r = x29_dbl_affine(qx, qy)
    return Case(F_DBL_AFFINE, FQ, what, qx + qy, _pt_words(r) + x29_to_r256(r), _pt_check(affine_add(P1, P1)))


def case_add_affine(what, acc, acc_affine, P2):
    qx, qy = affine_to_r261(P2) if P2 is not None else ([0] * 9, [0] * 9)
    r = x29_add_affine(acc, qx, qy, P2 is None)
    return Case(F_ADD_AFFINE, FQ, what, _pt_words(acc) + qx + qy, _pt_words(r) + x29_to_r256(r),
                _pt_check(affine_add(acc_affine, P2), 5 if _passes_through(r, [acc]) else 2), aux=int(P2 is None))


def case_dbl(what, pt, pt_affine):
    r = x29_dbl(pt)
    return Case(F_DBL, FQ, what, _pt_words(pt), _pt_words(r) + x29_to_r256(r), _pt_check(affine_add(pt_affine, pt_affine)))


def case_add(what, a, a_affine, b, b_affine):
    r = x29_add(a, b)
    return Case(F_ADD, FQ, what, _pt_words(a) + _pt_words(b), _pt_words(r) + x29_to_r256(r),
                _pt_check(affine_add(a_affine, b_affine), 5 if _passes_through(r, [a, b]) else 2))


# ---- the quad formulas: one record per quad; every lane returns its 36 words, lane 0 the packed form as well
def _quad_check(want, y_bound):
    one = _pt_check(want, y_bound)

    def check(o):
        copies = _vecs(o[:144], 36)
        assert all(c == copies[0] for c in copies[1:]), "the four lanes of the quad hold different points"
        one(copies[0] + o[144:176])
    return check


def _quad_expect(r):
    return _pt_words(r) * 4 + x29_to_r256(r)


def case_dbl_quad(what, pt, pt_affine, kind):
    r = x29_dbl_quad(pt)
    c = Case(F_DBL_QUAD, FQ, what, _pt_words(pt), _quad_expect(r), _quad_check(affine_add(pt_affine, pt_affine), 4))
    c.kind = kind
    return c


def case_add_quad(what, a, a_affine, b, b_affine, kind):
    r = x29_add_quad(a, b)
    c = Case(F_ADD_QUAD, FQ, what, _pt_words(a) + _pt_words(b), _quad_expect(r),
             _quad_check(affine_add(a_affine, b_affine), 5 if _passes_through(r, [a, b]) else 4))
    c.kind = kind
    return c


def case_quad_sits_out(func, data):
    """A quad that does not call the formula (the quads at and above `s` in a round of msm_rowcol_quad_kernel) beside quads
    that do: nothing may come back from it, and its neighbours' DPP moves must not notice."""
    c = Case(func, FQ, "sits out", data, [], lambda o: None, aux=AUX_SIT_OUT)
    c.kind = "sits out"
    return c


def case_quad_chain(what, pts):
    """msm_window_combine_kernel's shape: 16 steps of three doublings and one addition of pts[j % 4] (affine, zz = zzz = 1),
    from the identity, outputs (y below 4p) fed back in. The running point after steps 4, 8 and 12 from lane 0, after step 16
    from all four lanes, then its packed form."""
    assert len(pts) == 4
    acc, acc_a, cps, wants, kinds = x29_inf(), None, [], [], set()
    for j in range(QUAD_CHAIN_STEPS):
        for _ in range(3):
            acc, acc_a = x29_dbl_quad(acc), affine_add(acc_a, acc_a)
        P2 = pts[j % 4]
        kinds.add("restart" if acc_a is None else "doubling" if acc_a == P2 else "cancellation" if acc_a == affine_neg(P2) else "generic")
        acc, acc_a = x29_add_quad(acc, x29_from_affine(P2)), affine_add(acc_a, P2)
        if j % QUAD_CHAIN_EVERY == QUAD_CHAIN_EVERY - 1:
            cps.append(acc)
            wants.append(acc_a)
    last = _quad_check(wants[3], 4)

    def check(o):
        for i in range(3):
            pt = tuple(_vecs(o[36 * i:36 * i + 36]))
            assert x29_affine(pt) == wants[i], "checkpoint %d: wrong point" % i
            assert wants[i] is None or (val(pt[0]) < 9 * Q and val(pt[1]) < 4 * Q and max(val(pt[2]), val(pt[3])) < 2 * Q
                                        and all(x < 1 << 29 for c in pt for x in c[:8])), "checkpoint %d: outside the bounds" % i
        last(o[108:])
    c = Case(F_QUAD_CHAIN, FQ, what, sum((sum(affine_to_r261(P2), []) for P2 in pts), []),
             sum((_pt_words(cp) for cp in cps[:3]), []) + _quad_expect(cps[3]), check)
    c.kind, c.kinds = "chain", kinds
    return c


def quad_order(by_kind, filler, every=5):
    """Round-robin over the kinds, so that neighbouring quads of a wavefront take different branches; every `every`-th
    record gets a quad that sits out on both sides."""
    lists = [list(v) for v in by_kind.values()]
    out = []
    while any(lists):
        for l in lists:
            if l:
                out.append(l.pop(0))
    fenced = []
    for i, c in enumerate(out):
        fenced += [filler, c, filler] if i % every == every - 1 else [c]
    return fenced


def case_add_chain(what, pts):
    """64 mixed additions, step j adds pts[j % 4]; the running sum at every eighth step comes back."""
    assert len(pts) == 4
    acc, acc_a, outs, wants, seen_inf = x29_inf(), None, [], [], False
    for j in range(CHAIN_STEPS):
        P2 = pts[j % 4]
        qx, qy = affine_to_r261(P2)
        acc, acc_a = x29_add_affine(acc, qx, qy, False), affine_add(acc_a, P2)
        seen_inf |= acc_a is None
        if j % CHAIN_EVERY == CHAIN_EVERY - 1:
            outs += _pt_words(acc)
            wants.append(acc_a)

    def check(o):
        for i, w in enumerate(wants):
            assert x29_affine(tuple(_vecs(o[36 * i:36 * i + 36]))) == w, "checkpoint %d: wrong point" % i
    c = Case(F_ADD_CHAIN, FQ, what, sum((sum(affine_to_r261(P2), []) for P2 in pts), []), outs, check)
    c.seen_inf = seen_inf
    return c


def build_cases(n_random=64):
    """Every operand class for every function whose contract admits it, plus `n_random` random cases per function."""
    cs = []
    for F in (FQ, FR):
        rnd = random.Random(1000 + F.p % 997)
        small = class_small(F)
        names = ["0", "1", "2", "p-1", "p", "p+1", "2p-1", "M(0)", "M(1)", "M(-1)"]
        rand = class_random(F, n_random, 7)
        c3, c3_out = class_bound_pairs(F, MASK)
        c4, _ = class_bound_pairs(F, (1 << 30) - 1)
        c5, _ = class_lazy_mul(F)
        # f29_mul, context (i)
        for i, a in enumerate(small):
            for j, b in enumerate(small):
                cs.append(case_mul(F, "small %s x %s" % (names[i], names[j]), a, b))
        cs += [case_mul(F, "random", a, b) for a, b in rand]
        cs += [case_mul(F, "one hot", a, b) for a, b in class_one_hot(F)]
        cs += [case_mul(F, "limbs 2^29-1 at the 169 p^2 bound", a, b) for a, b in c3]
        cs += [case_mul(F, "limbs 2^30-1 at the 169 p^2 bound", a, b) for a, b in c4]
        cs += [case_mul(F, "lazy x normalised at the 169 p^2 bound", a, b) for a, b in c5]
        cs += [case_mul(F, "m_%d = %#x" % (k, t), a, b) for k, t, a, b in class_m_factor(F)]
        # f29_sqr
        sq_max, _ = class_sqr_bound(F)
        cs += [case_sqr(F, "small " + names[i], a) for i, a in enumerate(small)]
        cs += [case_sqr(F, "random", a) for a, _ in rand]
        cs += [case_sqr(F, "one hot", [MASK if j == i else 0 for j in range(9)]) for i in range(8)]
        cs += [case_sqr(F, "largest normalised operand", sq_max), case_sqr(F, "limbs 2^29-1, 13p", c3[0][0])]
        cs += [case_sqr(F, "m_%d = %#x" % (k, t), a) for k, t, a in class_m_factor_sqr(F)]
        # f29_mul2
        l2, _ = class_lazy_mul2(F)
        cs.append(case_mul2(F, "b lazy below 2^31, at the 169 p^2 bound", *l2))
        cs.append(case_mul2(F, "normalised 13p x 6.5p twice", c3[0][0], _top_for([MASK] * 8, 13 * F.p // 2), c3[0][0], _top_for([MASK] * 8, 13 * F.p // 2 - (1 << 233))))
        for i in range(0, 10, 3):
            cs.append(case_mul2(F, "small", small[i], small[(i + 3) % 10], small[(i + 5) % 10], small[(i + 6) % 10]))
        for i in range(n_random):
            cs.append(case_mul2(F, "random", rand[i][0], rand[i][1], rand[-1 - i][1], rand[-1 - i][0]))
        # context (ii): dependent chains
        for i in range(8):
            cs.append(case_mul_chain(F, "random", *rand[i]))
            cs.append(case_sqr_chain(F, "random", rand[i][0]))
            cs.append(case_mul2_chain(F, "random", rand[i][0], rand[i][1], rand[-1 - i][1], rand[-1 - i][0]))
        for a, b in c3 + c4 + c5[:2]:
            cs.append(case_mul_chain(F, "first step at the 169 p^2 bound", a, b))
        cs.append(case_sqr_chain(F, "largest normalised operand first", sq_max))
        cs.append(case_mul2_chain(F, "first step at the 169 p^2 bound", *l2))
        for i in (1, 3, 6, 9):
            cs.append(case_mul_chain(F, "small", small[i], small[(i + 5) % 10]))
            cs.append(case_sqr_chain(F, "small", small[i]))
        # wide accumulator
        for pairs, n in class_wide(F):
            cs.append(case_wide(F, "%d terms%s" % (n, ", all limbs 2^29-1" if pairs[0][0][8] == MASK else ""), pairs, n))
        cs += [case_reduce_weak(F, "top limb class", v) for v in class_reduce_weak(F)]
        # differences feeding a product
        hi = lambda k: _top_for([MASK] * 8, k * F.p - 1)  # the largest normalised-looking value below k p
        for K in (3, 5, 6, 7, 8, 10):
            cs.append(case_sub_mul(F, "largest subtrahend", K, hi(2), hi(K - 1), small[6]))
            cs.append(case_sub_mul(F, "zero minus largest", K, small[0], hi(K - 1), hi(2)))
            for i in range(4):
                cs.append(case_sub_mul(F, "random", K, rand[i][0], rand[i][1], rand[i + 4][0]))
        for K in (3, 6, 10):
            cs.append(case_neg_mul2(F, "largest", K, hi(2), hi(2), hi(K - 1), hi(2)))
            for i in range(4):
                cs.append(case_neg_mul2(F, "random", K, rand[i][0], rand[i][1], rand[i + 4][0], rand[i + 4][1]))
        cs.append(case_lazy_mul(F, "largest limbs: 2^29-1 minus 0", hi(2), small[0], hi(2)))
        cs.append(case_lazy_mul(F, "0 minus largest", small[0], hi(9), hi(2)))
        cs.append(case_lazy2_mul(F, "largest limbs", hi(4), hi(4), small[0], small[0], hi(2)))
        cs.append(case_lazy2_mul(F, "0 minus largest", small[0], small[0], hi(4), hi(4), hi(2)))
        cs.append(case_lazy_mul2(F, "largest limbs", hi(2), hi(2), small[0], hi(2), hi(2)))
        for i in range(8):
            (a, b), (c, d) = rand[i], rand[i + 8]
            cs.append(case_lazy_mul(F, "random", a, b, c))
            cs.append(case_lazy2_mul(F, "random", a, b, c, d, rand[i + 16 if i + 16 < len(rand) else 0][0]))
            cs.append(case_lazy_mul2(F, "random", a, b, c, d, rand[-1 - i][0]))
        # packing
        for x in [0, 1, F.p - 1, F.p, F.p + 1, 2 * F.p - 1, (1 << 232) - 1, 1 << 232] + [rnd.randrange(2 * F.p) for _ in range(n_random)]:
            cs.append(case_unpack_pack(F, "below 2p", x))
        # bn254.cuh device branches
        edge = [0, 1, 2, F.p - 1, R256 % F.p, (-R256) % F.p]
        for a in edge:
            for b in edge + [F.p, 2 * F.p, R256 - 1]:
                cs.append(case_bn_mul(F, "edge", a, b))
        cs += [case_bn_mul(F, "random", val(a), val(b)) for a, b in rand]
        cs += [case_bn_mul(F, "second operand any 256-bit value", val(a), rnd.randrange(R256)) for a, _ in rand[:8]]
        cs += [case_bn_inv(F, "edge", a) for a in edge] + [case_bn_inv(F, "random", val(a)) for a, _ in rand[:6]]
    # the packed entry points of the scalar and the base field
    F = FR
    rnd = random.Random(77)
    edge = [0, 1, 2, R - 1, R256 % R, RADIX % R, (-RADIX) % R]
    xs = edge + [rnd.randrange(R) for _ in range(n_random)]
    for i, x in enumerate(xs):
        y = xs[(3 * i + 1) % len(xs)]
        for f in (F_MUL_CONST, F_MUL_RR, F_MUL_STD):
            cs.append(case_fr_packed(f, "canonical", x, y))
        cs.append(case_fr_packed(F_FROM_MONT, "canonical", x))
    cs += [case_fr_packed(F_INV29, "canonical", x) for x in edge[1:] + xs[len(edge):len(edge) + 6]]
    for x in [0, 1, Q - 1, R256 % Q] + [rnd.randrange(Q) for _ in range(n_random)]:
        cs.append(case_from_to_r256("canonical", x))
    for v in [digits(0), digits(Q), digits(2 * Q - 1), _top_for([MASK] * 8, 16 * Q - 1)] + [digits(rnd.randrange(16 * Q)) for _ in range(n_random)]:
        cs.append(case_to_r256("below 16p", v))
    # context (iii): the point formulas
    pts = class_points()
    A, B_, C, D = pts[:4]
    for i, P1 in enumerate(pts):
        P2 = pts[(i + 1) % len(pts)]
        X1, X2 = x29_from_affine(P1), x29_from_affine(P2)
        S = x29_add_affine(X1, *affine_to_r261(P2), False)  # a genuine XYZZ point with zz != 1: P1 + P2
        Sa = affine_add(P1, P2)
        cs.append(case_dbl_affine("random", P1))
        cs.append(case_add_affine("random, zz = 1", X1, P1, P2))
        cs.append(case_add_affine("random", S, Sa, pts[(i + 2) % len(pts)]))
        cs.append(case_add_affine("P + P", S, Sa, Sa))
        cs.append(case_add_affine("P + (-P)", S, Sa, affine_neg(Sa)))
        cs.append(case_add_affine("identity + Q", x29_inf(), None, P2))
        cs.append(case_add_affine("P + identity", S, Sa, None))
        cs.append(case_dbl("random", S, Sa))
        cs.append(case_dbl("identity", x29_inf(), None))
        T = x29_dbl(S)  # 2 (P1 + P2), another representation class
        Ta = affine_add(Sa, Sa)
        cs.append(case_add("random", S, Sa, x29_add_affine(X2, *affine_to_r261(pts[(i + 3) % len(pts)]), False), affine_add(P2, pts[(i + 3) % len(pts)])))
        cs.append(case_add("P + P, two representations", T, Ta, x29_add(S, S), Ta))
        cs.append(case_add("P + P, same representation", S, Sa, S, Sa))
        cs.append(case_add("P + (-P)", T, Ta, x29_from_affine(affine_neg(Ta)), affine_neg(Ta)))
        cs.append(case_add("identity + P", x29_inf(), None, S, Sa))
        cs.append(case_add("P + identity", S, Sa, x29_inf(), None))
    # the same formulas with the accumulator at the top of its documented bounds (x29_lift), and the quad formulas on all of it
    dq = {"generic": [], "identity": []}
    aq = {}  # round-robin lists (the two doublings apart, so that every list is equally long) -> cases
    for i, P1 in enumerate(pts):
        P2, P3, P4 = pts[(i + 1) % len(pts)], pts[(i + 2) % len(pts)], pts[(i + 3) % len(pts)]
        S = x29_add_affine(x29_from_affine(P1), *affine_to_r261(P2), False)
        Sa = affine_add(P1, P2)
        T, Ta = x29_dbl(S), affine_add(Sa, Sa)
        U, Ua = x29_add_affine(x29_from_affine(P2), *affine_to_r261(P4), False), affine_add(P2, P4)
        SS = x29_add(S, S)  # 2 (P1 + P2) again, another representation than T
        negT = x29_from_affine(affine_neg(Ta))
        LS, LT, LU, LSS, LnegT = (x29_lift(X) for X in (S, T, U, SS, negT))
        top = "operands at the top of 9p / 5p / 2p / 2p: "
        cs.append(case_add_affine(top + "random", LS, Sa, P3))
        cs.append(case_add_affine(top + "P + P", LS, Sa, Sa))
        cs.append(case_add_affine(top + "P + (-P)", LS, Sa, affine_neg(Sa)))
        cs.append(case_add_affine(top + "P + identity", LS, Sa, None))
        cs.append(case_dbl(top + "random", LS, Sa))
        pairs = [("generic", "random", S, Sa, U, Ua, LS, LU),
                 ("doubling", "P + P, two representations", T, Ta, SS, Ta, LT, LSS),
                 ("doubling", "P + P, same representation", S, Sa, S, Sa, LS, LS),
                 ("cancellation", "P + (-P)", T, Ta, negT, affine_neg(Ta), LT, LnegT),
                 ("identity", "identity + P", x29_inf(), None, S, Sa, x29_inf(), LS),
                 ("identity", "P + identity", S, Sa, x29_inf(), None, LS, x29_inf())]
        for kind, what, a, aa, b, ba, la, lb in pairs:
            cs.append(case_add(top + what, la, aa, lb, ba))
            mine = aq.setdefault(kind + what[:12], [])
            mine.append(case_add_quad(what, a, aa, b, ba, kind))
            mine.append(case_add_quad(top + what, la, aa, lb, ba, kind))
            if kind != "identity":
                cs.append(case_add("top of the bounds + canonical: " + what, la, aa, b, ba))
                mine.append(case_add_quad("top of the bounds + canonical: " + what, la, aa, b, ba, kind))
                mine.append(case_add_quad("canonical + top of the bounds: " + what, a, aa, lb, ba, kind))
        dq["generic"] += [case_dbl_quad("random", S, Sa, "generic"), case_dbl_quad(top + "random", LS, Sa, "generic"),
                          case_dbl_quad("random, zz = 1", x29_from_affine(P1), P1, "generic")]
        dq["identity"].append(case_dbl_quad("identity", x29_inf(), None, "identity"))
    S0 = x29_add_affine(x29_from_affine(A), *affine_to_r261(B_), False)
    dbl_q = quad_order(dq, case_quad_sits_out(F_DBL_QUAD, _pt_words(S0)), every=3)
    add_q = quad_order(aq, case_quad_sits_out(F_ADD_QUAD, _pt_words(S0) + _pt_words(x29_dbl(S0))))
    for w in range(0, len(add_q), 16):  # sixteen quads are one wavefront
        assert len({c.kind for c in add_q[w:w + 16]} - {"sits out"}) >= 3, "a wavefront of add_quad cases with fewer than three branch kinds"
    assert all(any(c.kind == "sits out" for c in q[w:w + 16]) for q in (dbl_q, add_q) for w in range(0, len(q) - 15, 16))
    cs += dbl_q + add_q
    # A, -8A, D, 8D: A; 8A - 8A = identity (cancellation); 8 * identity + D (restart); 8D + 8D (the addition doubles); generic after
    qchain = case_quad_chain("A, -8A, D, 8D repeated: cancellation, identity, restart and doubling", [A, affine_neg(affine_mul(8, A)), D, affine_mul(8, D)])
    assert qchain.kinds == {"restart", "cancellation", "doubling", "generic"}
    cs += [qchain, case_quad_sits_out(F_QUAD_CHAIN, qchain.data), case_quad_chain("four random points", [A, B_, C, D]),
           case_quad_chain("three random points and one of them again", [B_, C, D, C]),
           # the point set of the lane-serial chain below; with three doublings a step it meets no special case here
           case_quad_chain("A, B, -(A+B), D repeated", [A, B_, affine_neg(affine_add(A, B_)), D])]
    chain = case_add_chain("A, B, -(A+B), D repeated: identity, restart and doubling", [A, B_, affine_neg(affine_add(A, B_)), D])
    assert chain.seen_inf
    cs.append(chain)
    cs.append(case_add_chain("four random points", [A, B_, C, D]))
    return cs
