#!/usr/bin/env python3
"""The dense case of committing a column through its row differences, on one GPU:

    python tools/bench_perm_diff_dense.py [--k 15] [--reps 30] [--out FILE]

One uniform random column Z of 2^k rows is committed (a) over g_lagrange and (b) as D[i] = Z[i] - Z[i+1], D[n-1] = Z[n-1],
over the prefix sums of g_lagrange (AMDZK_BASIS_G_LAGRANGE_PREFIX). A permutation product that changes on every row has
uniform differences, so (b) is what such a circuit pays: the same MSM on other scalars, plus the subtraction pass (one
elementwise kernel, `row_diff` in the per-kernel profile of a proof; not part of this script's timing — D is made on the
host). The two sides alternate inside one process; each figure is the median of --reps resident-column calls
(amdzk_msm_g1_dev, host wall clock around the blocking call) with its min .. max, and the points must agree."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def mont(xs):
    out = np.zeros((len(xs), 4), np.uint64)
    for i, x in enumerate(xs):
        v = (x << 256) % R
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & ((1 << 64) - 1)
    return out


def key_with_permutation(pkg, ctx, params, k):
    """the smallest circuit with permutation columns: making its key builds the prefix-sum basis on `params`"""
    plonk = pkg.plonk
    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    sel = cs.selector()
    cs.enable_equality(a)
    cs.enable_equality(b)
    cs.create_gate(lambda m: [m.query_selector(sel) * (m.query_advice(b, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))])
    c = pkg.workloads.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    fixed = np.zeros((len(c.fixed), c.n, 4), np.uint64)
    return plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, np.array([1, 0, 0, 0], np.uint64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    A, K = pkg.arithmetic, pkg.kzg
    n = 1 << args.k
    rnd = random.Random(15)
    z = [rnd.randrange(R) for _ in range(n)]
    d = [(z[i] - z[i + 1]) % R for i in range(n - 1)] + [z[n - 1]]
    lines = []
    with pkg.Context(0) as ctx:
        params = K.ParamsKZG.setup(ctx, args.k, np.array([0x1234567, 0, 0, 0], dtype=np.uint64))
        t0 = time.perf_counter()
        pk = key_with_permutation(pkg, ctx, params, args.k)
        t_key = time.perf_counter() - t0
        bz, bd = ctx.alloc(n * 32).upload(mont(z)), ctx.alloc(n * 32).upload(mont(d))
        sides = (("Z over g_lagrange", K.BASIS_G_LAGRANGE, bz), ("D over the prefix sums", K.BASIS_G_LAGRANGE_PREFIX, bd))
        pts, ts = {}, {name: [] for name, _, _ in sides}
        for rep in range(args.warmup + args.reps):
            for name, basis, buf in sides:
                t0 = time.perf_counter()
                pts[name] = A.best_multiexp_dev(ctx, params.h, basis, buf, 1, n)
                if rep >= args.warmup:
                    ts[name].append(time.perf_counter() - t0)
        assert np.array_equal(pts[sides[0][0]], pts[sides[1][0]]), "the two commitments differ"
        lines.append("dense case, one uniform random column of 2^%d rows, %d alternating calls each (median, min .. max, ms):" % (args.k, args.reps))
        for name, _, _ in sides:
            v = [x * 1e3 for x in ts[name]]
            lines.append("  %-24s %.3f   %.3f .. %.3f" % (name, statistics.median(v), min(v), max(v)))
        lines.append("  same point: yes; the key that built the basis (keygen of a two-column circuit, the build included) took %.1f ms" % (t_key * 1e3))
        bz.free(); bd.free(); pk.free(); params.free()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
