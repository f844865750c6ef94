"""Reference for the BN254 optimal ate pairing in Python integers, written independently of the device algorithm
(csrc/fq12.cuh, csrc/pairing.hpp): textbook affine chord-and-tangent lines on the twist, untwisted into Fq12 kept as ONE
polynomial ring Fq[w]/(w^12 - 18 w^6 + 82) (no tower, no sparse products, no Frobenius tables, no cyclotomic squaring),
and a literal pow(f, (p^12 - 1) / r).

Conventions (the published BN254 / EIP-197 ones; the reference repository holds no G2 data, so parity is unpinned):
  Fq2 = Fq[u]/(u^2 + 1), xi = 9 + u;  Fq6 = Fq2[v]/(v^3 - xi);  Fq12 = Fq6[w]/(w^2 - v), so w^6 = xi and u = w^6 - 9.
  G2: the order-r subgroup of the D-type twist y^2 = x^3 + 3/xi over Fq2; untwist (x, y) -> (x w^2, y w^3).
  G2 generator: EIP-197's.  u = 4965661367192848881.  Miller loop over 6u + 2, then the lines of pi(Q) and -pi^2(Q).
  e(P, Q) = f^((p^12 - 1)/r): the exact exponent, so the GT value is canonical.
One pairing costs about a second; miller() and final_exp() cache per process."""
import functools

P = Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
U = 4965661367192848881
ATE = 6 * U + 2
assert P == 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1 and R == 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1

G1_GEN = (1, 2)
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


# ---------------------------------------------------------------- Fq2 as (c0, c1) = c0 + c1 u
def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, P)
    return (a[0] * d % P, -a[1] * d % P)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


def f2_conj(a):
    return (a[0], -a[1] % P)


XI = (9, 1)
B2 = f2_mul((3, 0), f2_inv(XI))  # the twist's constant 3 / xi


# ---------------------------------------------------------------- G2 on the twist, affine, None = identity
def g2_on_curve(q):
    if q is None:
        return True
    x, y = q
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B2)


def g2_neg(q):
    return None if q is None else (q[0], f2_sub((0, 0), q[1]))


def g2_slope(a, b):
    if a == b:
        x2 = f2_mul(a[0], a[0])
        return f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(a[1], a[1])))
    return f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0] and a[1] != b[1]:
        return None
    if a == b and a[1] == (0, 0):
        return None
    lam = g2_slope(a, b)
    x = f2_sub(f2_sub(f2_mul(lam, lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_mul(q, k):
    r = None
    while k:
        if k & 1:
            r = g2_add(r, q)
        q = g2_add(q, q)
        k >>= 1
    return r


# ---------------------------------------------------------------- G1, affine, None = identity
def g1_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % P == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, P) % P
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, P) % P
    x = (lam * lam - a[0] - b[0]) % P
    return (x, (lam * (a[0] - x) - a[1]) % P)


def g1_mul(p, k):
    r = None
    while k:
        if k & 1:
            r = g1_add(r, p)
        p = g1_add(p, p)
        k >>= 1
    return r


def g1_neg(p):
    return None if p is None else (p[0], -p[1] % P)


# ---------------------------------------------------------------- Fq12 = Fq[w]/(w^12 - 18 w^6 + 82), 12 coefficients
F12_ONE = (1,) + (0,) * 11


def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for k in range(22, 11, -1):  # w^k = 18 w^(k-6) - 82 w^(k-12)
        c = t[k]
        if c:
            t[k - 6] += 18 * c
            t[k - 12] -= 82 * c
    return tuple(v % P for v in t[:12])


def f12_pow(a, e):
    r = F12_ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def f12_inv(a):
    return f12_pow(a, P**12 - 2)


def f12_from_fq2(c, e):
    """c * w^e for c in Fq2, e < 6: u = w^6 - 9."""
    r = [0] * 12
    r[e] = (c[0] - 9 * c[1]) % P
    r[e + 6] = c[1] % P
    return tuple(r)


def f12_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def f12_to_tower(a):
    """The 12 Fq of halo2curves' Fq12 in declaration order: c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1, where
    c_i.c_j = the Fq2 coefficient of w^i v^j = w^(i + 2j)."""
    out = []
    for i in range(2):
        for j in range(3):
            e = i + 2 * j
            out += [(a[e] + 9 * a[e + 6]) % P, a[e + 6]]
    return out


def f12_from_tower(t):
    """The inverse of f12_to_tower: c_i.c_j = (x, y) contributes (x - 9 y) w^e + y w^(e + 6), e = i + 2j."""
    a = [0] * 12
    for i in range(2):
        for j in range(3):
            e, k = i + 2 * j, 2 * (3 * i + j)
            a[e], a[e + 6] = (t[k] - 9 * t[k + 1]) % P, t[k + 1] % P
    return tuple(a)


# ---------------------------------------------------------------- the pairing
def _line(t, q, p):
    """The line through t and q (the tangent when t == q) on the twist, untwisted and evaluated at the G1 point p:
    (y_P - y_T w^3) - lambda w (x_P - x_T w^2)."""
    lam = g2_slope(t, q)
    c = f2_sub(f2_mul(lam, t[0]), t[1])  # lambda x_T - y_T, the coefficient of w^3
    r = f12_add(f12_from_fq2((p[1], 0), 0), f12_from_fq2(f2_mul(lam, ((-p[0]) % P, 0)), 1))
    return f12_add(r, f12_from_fq2(c, 3))


def g2_frobenius(q):
    """pi(x, y) on the twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))."""
    return (f2_mul(f2_conj(q[0]), f2_pow(XI, (P - 1) // 3)), f2_mul(f2_conj(q[1]), f2_pow(XI, (P - 1) // 2)))


@functools.lru_cache(maxsize=None)
def miller(p, q):
    """f_{6u+2,Q}(P) l_{[6u+2]Q, pi Q}(P) l_{[6u+2]Q + pi Q, -pi^2 Q}(P); 1 when either point is the identity."""
    if p is None or q is None:
        return F12_ONE
    f, t = F12_ONE, q
    for bit in bin(ATE)[3:]:
        f = f12_mul(f12_mul(f, f), _line(t, t, p))
        t = g2_add(t, t)
        if bit == "1":
            f = f12_mul(f, _line(t, q, p))
            t = g2_add(t, q)
    q1 = g2_frobenius(q)
    q2 = g2_neg(g2_frobenius(q1))
    f = f12_mul(f, _line(t, q1, p))
    t = g2_add(t, q1)
    return f12_mul(f, _line(t, q2, p))


@functools.lru_cache(maxsize=None)
def final_exp(f):
    return f12_pow(f, (P**12 - 1) // R)


def pairing(p, q):
    return final_exp(miller(p, q))


def pairing_product(pairs):
    """prod e(P_j, Q_j): one final exponentiation over the product of the Miller values."""
    f = F12_ONE
    for p, q in pairs:
        f = f12_mul(f, miller(p, q))
    return final_exp(f)


# ---------------------------------------------------------------- halo2curves' in-memory words (Montgomery, R = 2^256)
def fq_words(v):
    m = v * (1 << 256) % P
    return [(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def g1_words(p):
    return [0] * 8 if p is None else fq_words(p[0]) + fq_words(p[1])


def g2_words(q):
    """G2Affine {x.c0, x.c1, y.c0, y.c1}: 16 words; all zero = the identity."""
    return [0] * 16 if q is None else fq_words(q[0][0]) + fq_words(q[0][1]) + fq_words(q[1][0]) + fq_words(q[1][1])


def g2_from_words(w):
    inv = pow(1 << 256, -1, P)
    v = [sum(int(w[4 * i + j]) << (64 * j) for j in range(4)) * inv % P for i in range(4)]
    return None if not any(v) else ((v[0], v[1]), (v[2], v[3]))


def gt_words(f):
    """Fq12 in declaration order: 48 words."""
    return [w for c in f12_to_tower(f) for w in fq_words(c)]
