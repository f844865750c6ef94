"""Specs and operands of the Poseidon tests. The constants are NOT those of any Poseidon instance: round constants from
hashlib.blake2b and an MDS that is random, Cauchy, all r - 1, all zero or the identity — the kernels' correctness does not
depend on which constants they are given, and the edge ones are what drives their sums of products to their bounds."""
import ctypes as C
import hashlib

import numpy as np

import poseidon_ref as PR

R = PR.R
KINDS = ("random", "cauchy", "max", "zero", "identity")


def stream(tag):
    """An endless deterministic stream of integers below r."""
    i = 0
    while True:
        h = hashlib.blake2b(b"%s/%d" % (tag.encode(), i), digest_size=40).digest()
        yield int.from_bytes(h, "little") % R
        i += 1


def take(gen, n):
    return [next(gen) for _ in range(n)]


def spec(t, rate, r_f, r_p, kind="random", init=False):
    g = stream("spec/%d/%d/%d/%d/%s" % (t, rate, r_f, r_p, kind))
    rounds = r_f + r_p
    if kind == "max":
        rc = [[R - 1] * t for _ in range(rounds)]
        mds = [[R - 1] * t for _ in range(t)]
    elif kind == "zero":
        rc = [[0] * t for _ in range(rounds)]
        mds = [[0] * t for _ in range(t)]
    else:
        rc = [take(g, t) for _ in range(rounds)]
        if kind == "identity":
            mds = [[int(i == j) for j in range(t)] for i in range(t)]
        elif kind == "cauchy":
            mds = [[pow(i + t + j, -1, R) for j in range(t)] for i in range(t)]  # 1 / (x_i + y_j), x_i = i, y_j = t + j
        else:
            mds = [take(g, t) for _ in range(t)]
    return PR.Spec(t, rate, r_f, r_p, rc, mds, take(g, t) if init else None)


def states(t, n, tag="states"):
    """n states, a prefix of one sequence whatever n: all 0, all 1, all r - 1, the three mixed, then random."""
    g = stream("%s/%d" % (tag, t))
    out = [[0] * t, [1] * t, [R - 1] * t, [(0, 1, R - 1)[i % 3] for i in range(t)]]
    while len(out) < n:
        out.append(take(g, t))
    return out[:n]


def inputs(length, tag, edge=False):
    g = stream("in/%s/%d" % (tag, length))
    v = take(g, length)
    if edge:
        for i, e in enumerate((R - 1, 0, 1)):
            if i < length:
                v[(i * 7) % length] = e
    return v


def to_words(values):
    """Integers -> (n, 4) uint64 Montgomery words."""
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (v % R) * (1 << 256) % R
        for k in range(4):
            out[i, k] = (m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return out


_RINV = pow(1 << 256, -1, R)


def from_words(words):
    """(n, 4) uint64 words -> the integers they hold as Montgomery values (a word pattern >= r is a failure)."""
    out = []
    for row in np.asarray(words, dtype=np.uint64).reshape(-1, 4):
        m = sum(int(w) << (64 * k) for k, w in enumerate(row))
        assert m < R, "not canonical: %x" % m
        out.append(m * _RINV % R)
    return out


def pkg_spec(pkg, s):
    """The package's Spec of a reference Spec."""
    return pkg.poseidon.Spec(s.t, s.rate, s.r_f, s.r_p, s.rc, s.mds, s.init)


# ---- descriptions the library refuses (amdzk_poseidon_check_desc without a device, amdzk_poseidon_compile with one)
def raw_desc(pkg, t=3, rate=2, r_f=2, r_p=1, size=None, rc=True, mds=True, init=False, poke=None):
    """(amdzk_poseidon_desc, keep-alive) over arrays of valid words; poke = (which array, element): that element becomes the
    modulus itself."""
    ffi = pkg.ffi
    tt = max(t, 1)
    arrays = {"rc": to_words(inputs(max(1, min(r_f + r_p, 4096)) * tt, "rc")), "mds": to_words(inputs(tt * tt, "mds")),
              "init": to_words(inputs(tt, "init"))}
    if poke:
        arrays[poke[0]][poke[1]] = [(R >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    d = ffi.PoseidonDesc(C.sizeof(ffi.PoseidonDesc) if size is None else size, t, rate, r_f, r_p, arrays["rc"].ctypes.data if rc else None,
                         arrays["mds"].ctypes.data if mds else None, arrays["init"].ctypes.data if init else None)
    return d, arrays


# (name, raw_desc arguments, status, what the message names)
DESC_REFUSALS = [
    ("size", dict(size=8), -2, "too small"),
    ("t=1", dict(t=1, rate=1), -2, "t = 1"),
    ("t=9", dict(t=9), -2, "t = 9"),
    ("rate=0", dict(rate=0), -2, "rate = 0"),
    ("rate=t", dict(rate=3), -2, "rate = 3"),
    ("r_f=0", dict(r_f=0), -2, "r_f = 0"),
    ("r_f odd", dict(r_f=3), -2, "r_f = 3"),
    ("null rc", dict(rc=False), -2, "null"),
    ("null mds", dict(mds=False), -2, "null"),
    ("rc >= r", dict(poke=("rc", 7)), -2, "round constant 1 of round 2"),
    ("mds >= r", dict(poke=("mds", 5)), -2, "mds[1][2]"),
    ("init >= r", dict(init=True, poke=("init", 2)), -2, "initial_state[2]"),
    ("too many rounds", dict(r_p=511), -5, "above 1536"),
    ("r_p wraps", dict(r_p=0xFFFFFFFF), -5, "above 1536"),
]
