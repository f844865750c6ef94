"""Reference for amdzk_srs_check in Python integers. It knows what the device must not need: the discrete logarithms. An SRS
is given as the logarithms of its points to the base G = (1, 2) — for an honest one g_logs[i] = s^i and gl_logs[i] = L_i(s) —
and s2 is the logarithm of s_g2 to the base g2. The four sums of include/amdzk.h follow in the exponent:
  A = sum_{i<=n-2} rho^i g[i],  B = sum_{i<=n-2} rho^i g[i+1],  C = sum_j c_j g[j],  E = sum_i rho^i g_lagrange[i]
with c the coefficients of the polynomial that is rho^i at omega^i, and with them the verdicts: POWERS holds iff n = 1, or A and
B are not the identity and B = s2 A; LAGRANGE holds iff C = E. Points by tests/pairing_ref.py's G1 arithmetic."""
import pairing_ref as X

R = X.R
G = X.G1_GEN
CHECK_G2, CHECK_CURVE, CHECK_POWERS, CHECK_LAGRANGE = 1, 2, 4, 8
ALL = 15


def omega(k):
    """halo2curves' Fr::ROOT_OF_UNITY = 7^((r-1)/2^28) squared down to order 2^k: EvaluationDomain's omega."""
    assert k <= 28
    return pow(pow(7, (R - 1) >> 28, R), 1 << (28 - k), R)


def honest_logs(s, k):
    """(g_logs, gl_logs) of ParamsKZG::setup(k) with the trapdoor s: s^i and L_i(s) = omega^i (s^n - 1) / (n (s - omega^i))."""
    n, w = 1 << k, omega(k)
    g = [pow(s, i, R) for i in range(n)]
    m = (pow(s, n, R) - 1) * pow(n, -1, R) % R
    gl = [pow(w, i, R) * m % R * pow(s - pow(w, i, R), -1, R) % R for i in range(n)]
    assert sum(gl) % R == 1  # the Lagrange basis sums to one
    return g, gl


def interpolate(values, k):
    """Coefficients of the polynomial with these values on 1, omega, omega^2, ...: c_j = (1/n) sum_i v_i omega^(-ij)."""
    n = 1 << k

    def fft(a, w):
        if len(a) == 1:
            return a
        even, odd = fft(a[0::2], w * w % R), fft(a[1::2], w * w % R)
        out, t, h = [0] * len(a), 1, len(a) // 2
        for i in range(h):
            out[i], out[i + h] = (even[i] + t * odd[i]) % R, (even[i] - t * odd[i]) % R
            t = t * w % R
        return out
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in fft(list(values), pow(omega(k), -1, R))]


def sums(g_logs, gl_logs, rho, k):
    """The logarithms of (A, B, C, E); a missing basis (None) gives None for the sums that read it."""
    n = 1 << k
    e = [pow(rho, i, R) for i in range(n)]
    a = b = c = ee = None
    if g_logs is not None:
        a = sum(e[i] * g_logs[i] for i in range(n - 1)) % R
        b = sum(e[i] * g_logs[i + 1] for i in range(n - 1)) % R
        coeff = interpolate(e, k)
        if n <= 64:  # the definition, where it is cheap: the polynomial takes rho^i at omega^i
            w = omega(k)
            for i in sorted({0, min(1, n - 1), n - 1}):
                assert sum(cj * pow(w, i * j, R) for j, cj in enumerate(coeff)) % R == e[i]
        c = sum(cj * gj for cj, gj in zip(coeff, g_logs)) % R
    if gl_logs is not None:
        ee = sum(e[i] * gl_logs[i] for i in range(n)) % R
    return a, b, c, ee


def point(log):
    """log * G as an affine point, None = the identity."""
    return X.g1_mul(G, log % R)


def expected(g_logs, gl_logs, s2, rho, k):
    """{"logs": the logarithms of (A, B, C, E), "powers": bool, "lagrange": bool or None (a basis is missing)}: what the checks
    must find for on-curve bases and G2 points in G2."""
    a, b, c, e = sums(g_logs, gl_logs, rho, k)
    n = 1 << k
    powers = n == 1 or (a != 0 and b != 0 and b == s2 * a % R)
    return {"logs": (a, b, c, e), "powers": powers, "lagrange": c == e if (c is not None and e is not None) else None}


def rho_of_seed(seed):
    """The first Fr::random of ChaCha20Rng::seed_from_u64(seed), by the protocol oracle's generator."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import plonk_ref as PR
    return PR.ChaCha20Rng(seed).fr()
