"""Poseidon over Fr on Python integers, written from the text of include/amdzk.h ("Poseidon over Fr") alone: the reference
of the host and GPU tests. tests/test_poseidon_ref.py holds it to closed forms."""
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


class Spec:
    """rc: (r_f + r_p) rows of t integers; mds: t rows of t integers; init: t integers, or None = (2^64, 0, ..., 0)."""

    def __init__(self, t, rate, r_f, r_p, rc, mds, init=None):
        assert len(rc) == r_f + r_p and all(len(row) == t for row in rc)
        assert len(mds) == t and all(len(row) == t for row in mds)
        self.t, self.rate, self.r_f, self.r_p, self.rc, self.mds, self.init = t, rate, r_f, r_p, rc, mds, init

    def initial_state(self):
        return list(self.init) if self.init is not None else [1 << 64] + [0] * (self.t - 1)


def permute(spec, state):
    s = list(state)
    t, half = spec.t, spec.r_f // 2
    for rho in range(spec.r_f + spec.r_p):
        s = [(s[i] + spec.rc[rho][i]) % R for i in range(t)]
        if rho < half or rho >= half + spec.r_p:
            s = [pow(x, 5, R) for x in s]
        else:
            s[0] = pow(s[0], 5, R)
        s = [sum(spec.mds[i][j] * s[j] for j in range(t)) % R for i in range(t)]
    return s


def chunks(inputs, rate):
    """What a sponge adds before each of its permutations: the full chunks, then the left-over followed by ONE."""
    inputs = list(inputs)
    full = len(inputs) // rate
    out = [inputs[c * rate:(c + 1) * rate] for c in range(full)]
    out.append(inputs[full * rate:] + [1])
    return out


def sponge(spec, inputs, permute_fn=permute):
    s = spec.initial_state()
    for chunk in chunks(inputs, spec.rate):
        for i, v in enumerate(chunk):
            s[1 + i] = (s[1 + i] + v) % R
        s = permute_fn(spec, s)
    return s[1]
