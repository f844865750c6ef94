#!/usr/bin/env python3
"""Time amdzk_verify_proofs_decide_mixed against the routes a caller had before it, on one GPU, and write
profiles/verify_mixed.txt.

    python tools/verify_mixed_bench.py [--k 15] [--reps 7] [--identities 1,16] [--out FILE]

An "identity" is four proofs of four DIFFERENT circuits, as the reference proves them: one of the full shape
(workloads.full_aadhaar_shape, k = 15) and one each of three small gate circuits (k = 4, 5, 6), every key a verifying key over
the same G. Three routes decide the same proofs, in one process, alternating rep by rep, median of --reps after a warm-up:

    mixed     ONE amdzk_verify_proofs_decide_mixed call, flags = 0: one decode launch, one pairing launch
    four      FOUR amdzk_verify_proofs_decide_vk calls, flags = 0, one per key: four decode launches, four pairing launches
    composed  FOUR amdzk_verify_proofs_vk calls and ONE amdzk_pairing_products over the four pairs (one check per KEY, weights
              from a seed: a verdict per key, not per proof)

Wall clock around the blocking calls, the Python binding's argument marshalling included on every route. Every verdict must be
1 and the routes must agree or the run stops."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
TAU = 0x1234567890ABCDEF1234567


def fr_from_int(x):
    v = x * (1 << 256) % R
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def neg_point(p):
    """-P of a G1Affine in Montgomery words ((0, 0) stays): the Montgomery form is linear, so -y is q - y on the words."""
    out = np.array(p, dtype=np.uint64).copy()
    y = sum(int(w) << (64 * i) for i, w in enumerate(out[4:]))
    if y:
        y = Q - y
        out[4:] = [(y >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]
    return out


def small_circuit(plonk, wl, k, extra_adv, extra_fix):
    """a * a = b in one row, plus extra queried advice and fixed columns (all zero): three small shapes that differ."""
    cs = plonk.ConstraintSystem()
    a, b = cs.advice_column(), cs.advice_column()
    xs = [cs.advice_column() for _ in range(extra_adv)]
    sel = cs.selector()
    fs = [cs.fixed_column() for _ in range(extra_fix)]
    cs.enable_equality(a)
    cs.create_gate(lambda m: [m.query_selector(sel) * (m.query_advice(b, 0) - m.query_advice(a, 0) * m.query_advice(a, 0))] +
                   [m.query_selector(sel) * m.query_advice(x, 0) for x in xs] + [m.query_selector(sel) * m.query_fixed(f, 0) for f in fs])
    c = wl.Circuit(cs, k)
    c.assembly = plonk.Assembly(c.n, len(cs.permutation_columns))
    c.fixed[sel.index][0] = 1
    c.advice[a.index][0], c.advice[b.index][0] = 11, 121
    c.instances = []
    wl.check_satisfied(c)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--identities", default="1,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_mixed.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge

    pkg = ge.load_package()
    plonk, wl, kzg = pkg.plonk, pkg.workloads, pkg.kzg
    shapes = [("full_aadhaar_shape k=%d" % args.k, wl.full_aadhaar_shape(k=args.k)), ("gate k=4", small_circuit(plonk, wl, 4, 0, 0)),
              ("gate k=5, 8 more advice", small_circuit(plonk, wl, 5, 8, 0)), ("gate k=6, 3 more advice, 2 fixed", small_circuit(plonk, wl, 6, 3, 2))]
    with pkg.Context(0) as ctx:
        def resident(cols):  # canonical limbs up, Fr::from_raw on the device
            host = np.ascontiguousarray(wl.canon_limbs(cols))
            d = ctx.alloc(host.nbytes).upload(host)
            ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, d.ptr, host.size // 4))
            return d

        vparams = kzg.ParamsVerifierKZG.setup(ctx, fr_from_int(TAU))
        keys = []  # (name, vk, instances, two proofs)
        for name, c in shapes:
            params = kzg.ParamsKZG.setup(ctx, c.k, fr_from_int(TAU))
            d_fixed = resident(c.fixed)
            fixed = d_fixed.download((len(c.fixed), c.n, 4))
            d_fixed.free()
            pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, fr_from_int(123456789))
            d_adv = resident(c.advice)
            inst = []
            for col in c.instances:
                d = resident([col]) if col else None
                inst.append(d.download((len(col), 4)) if col else np.zeros((0, 4), np.uint64))
                if d:
                    d.free()
            proofs = [plonk.create_proof(ctx, pk, inst, d_adv, seed=200 + s) for s in range(2)]
            keys.append((name, pk.get_vk(), inst, proofs))
            d_adv.free()
            pk.free()
            params.free()  # a verifier process is a ctx and key files: no SRS, no proving key
        ctx.sync()

        def timed(fn):
            t0 = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t0) * 1e3, out

        lines = ["amdzk_verify_proofs_decide_mixed, %s" % pkg.build_info()["text"],
                 "an identity = 4 proofs of 4 circuits under 4 verifying keys over one G: " + "; ".join("%s (%d bytes)" % (n, len(p[0])) for n, _, _, p in keys),
                 "Blake2b transcript, SHPLONK; proofs by the device prover in the same process; one process, one GPU",
                 "wall ms around the blocking calls (binding's marshalling included), the routes alternating rep by rep, median of %d after one warm-up" % args.reps,
                 "  mixed    = 1 amdzk_verify_proofs_decide_mixed call, flags = 0 (a verdict per proof)",
                 "  four     = 4 amdzk_verify_proofs_decide_vk calls, flags = 0 (a verdict per proof)",
                 "  composed = 4 amdzk_verify_proofs_vk calls + 1 amdzk_pairing_products with 4 checks (a verdict per key)",
                 "%10s %8s %12s %12s %14s %12s" % ("identities", "proofs", "mixed ms", "four ms", "composed ms", "four/mixed")]
        for ni in [int(v) for v in args.identities.split(",")]:
            # identity after identity, so that every run of 16 positions holds all four keys
            items = [plonk.VerifyItem(vk, inst, proofs[i % 2]) for i in range(ni) for _, vk, inst, proofs in keys]

            def mixed():
                return plonk.decide_proofs_mixed(ctx, vparams, items)[0]

            def four():
                return [plonk.decide_proofs(ctx, vk, vparams, [inst] * ni, [proofs[i % 2] for i in range(ni)])[0] for _, vk, inst, proofs in keys]

            def composed():
                g1 = []
                for _, vk, inst, proofs in keys:
                    g = plonk.verify_proofs(ctx, vk, [inst] * ni, [proofs[i % 2] for i in range(ni)], combine_seed=987654321)
                    if not g.well_formed:
                        raise SystemExit("a proof of the device prover is reported malformed")
                    g1 += [g.lhs, neg_point(g.rhs)]
                return list(kzg.pairing_products(ctx, [vparams.s_g2, vparams.g2], np.stack(g1), want_gt=False)[0])

            routes = {"mixed": mixed, "four": four, "composed": composed}
            a, b, c_ = mixed(), four(), composed()  # the warm-up, and the check
            by_key = [[a[i * len(keys) + j] for i in range(ni)] for j in range(len(keys))]
            if not (all(a) and by_key == b and all(bool(v) for v in c_) and len(c_) == len(keys)):
                raise SystemExit("the routes disagree or a valid proof is decided invalid: refusing to time a wrong verifier")
            wall = {r: [] for r in routes}
            for _ in range(args.reps):
                for r, fn in routes.items():
                    wall[r].append(timed(fn)[0])
            m = {r: statistics.median(v) for r, v in wall.items()}
            lines.append("%10d %8d %12.3f %12.3f %14.3f %12.2f" % (ni, ni * len(keys), m["mixed"], m["four"], m["composed"], m["four"] / m["mixed"]))
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        for _, vk, _, _ in keys:
            vk.free()
        vparams.free()


if __name__ == "__main__":
    main()
