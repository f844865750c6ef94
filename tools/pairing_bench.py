#!/usr/bin/env python3
"""Time the pairing unit on one GPU and write profiles/pairing.txt.

    python tools/pairing_bench.py [--k 15] [--reps 7] [--products 1,64,1024] [--batches 1,64 | ""] [--out FILE]

Part 1: amdzk_pairing_products with m = 2 at every --products size: the device time between amdzk_timer_start and
amdzk_timer_stop around the blocking call (upload, both kernels, download) and the host wall clock around it — medians of
--reps after one warm-up of that shape — and, from one more call with every kernel event-bracketed (amdzk_prof_*), the time
of each of the two kernels. The inputs are pairs that cancel, (aP, -P) over (Q, aQ), and every is_one must read 1 or the run
stops.
Part 2: amdzk_verify_proofs_decide per proof and combined at the metric shape (workloads.full_aadhaar_shape) for every
--batches size, beside amdzk_verify_proofs alone IN THE SAME RUN (the cost of everything but the verdict): wall clock,
medians as above. Proofs are made by the device prover in the same process; every verdict must be 1 or the run stops."""
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


def fq_words(x):
    v = x * (1 << 256) % Q
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def finish(lines, out):
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--products", default="1,64,1024")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairing.txt"))
    args = ap.parse_args()
    products = [int(v) for v in args.products.split(",")]
    batches = [int(v) for v in args.batches.split(",") if v]  # --batches "": part 1 alone
    import __graft_entry__ as ge

    pkg = ge.load_package()
    plonk, kzg, wl = pkg.plonk, pkg.kzg, pkg.workloads
    lines = ["pairing unit, %s" % pkg.build_info()["text"], "one process, one GPU; medians of %d after one warm-up per shape" % args.reps, ""]
    with pkg.Context(0) as ctx:
        # ---- part 1: (aP, -P) over (Q, aQ) with a = 2: 2P = (x2, y2) by the tangent at P = (1, 2)
        lam = 3 * pow(4, -1, Q) % Q
        x2 = (lam * lam - 2) % Q
        y2 = (lam * (1 - x2) - 2) % Q
        pair = np.array(fq_words(x2) + fq_words(y2) + fq_words(1) + fq_words(Q - 2), dtype=np.uint64).reshape(2, 8)
        g2, two_g2 = kzg.g2_setup(ctx, fr_from_int(2))
        qs = [kzg.G2Prepared(ctx, g2), kzg.G2Prepared(ctx, two_g2)]
        lines += ["amdzk_pairing_products, m = 2 (device ms: amdzk_timer_* around the call; kernels: one more call, event-bracketed)",
                  "%8s %12s %12s %16s %18s %18s" % ("n", "device ms", "wall ms", "wall us/product", "pairing_miller ms", "pairing_final ms")]
        for n in products:
            g1 = np.ascontiguousarray(np.tile(pair, (n, 1)))
            run = lambda: kzg.pairing_products(ctx, qs, g1, want_gt=False)[0]
            if not run().all():
                raise SystemExit("a pair that cancels does not read is_one: refusing to time a wrong pairing")
            dev, wall = [], []
            for _ in range(args.reps):
                ctx.timer_start()
                w, _ = timed(run)
                dev.append(ctx.timer_stop())
                wall.append(w)
            ctx.prof_enable(True)
            ctx.prof_reset()
            run()
            ctx.sync()
            prof = ctx.prof_dump()
            ctx.prof_enable(False)
            w = statistics.median(wall)
            lines.append("%8d %12.3f %12.3f %16.1f %18.3f %18.3f" % (n, statistics.median(dev), w, 1e3 * w / n, prof["pairing_miller"][1], prof["pairing_final"][1]))
        for q in qs:
            q.free()
        if not batches:
            return finish(lines, args.out)
        # ---- part 2: the metric shape
        c = wl.full_aadhaar_shape(k=args.k)
        nrows = c.n
        params = kzg.ParamsKZG.setup(ctx, c.k, fr_from_int(TAU))
        vparams = kzg.ParamsVerifierKZG.setup(ctx, fr_from_int(TAU))

        def resident(cols):  # canonical limbs up, Fr::from_raw on the device
            host = np.ascontiguousarray(wl.canon_limbs(cols))
            d = ctx.alloc(host.nbytes).upload(host)
            ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, d.ptr, host.size // 4))  # the buffer's own element count: an instance column is shorter than n
            return d

        d_fixed = resident(c.fixed)
        fixed = d_fixed.download((len(c.fixed), nrows, 4))
        d_fixed.free()
        pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, fr_from_int(123456789))
        d_adv = resident(c.advice)
        inst = []
        for col in c.instances:
            d = resident([col]) if col else None
            inst.append(d.download((len(col), 4)) if col else np.zeros((0, 4), np.uint64))
            if d:
                d.free()
        ctx.sync()
        distinct = min(max(batches), 8)  # the cost of a proof does not depend on its bytes: a large batch repeats these
        made = [plonk.create_proof(ctx, pk, inst, d_adv, seed=100 + s) for s in range(distinct)]
        lines += ["", "amdzk_verify_proofs_decide at full_aadhaar_shape k = %d (proof of %d bytes), Blake2b, SHPLONK; wall ms around the blocking call" % (c.k, len(made[0])),
                  "verify alone = amdzk_verify_proofs in the same run: everything but the verdict",
                  "%8s %14s %16s %16s %22s" % ("n_proofs", "verify alone", "decide per proof", "decide combined", "per proof ms/proof")]
        for nb in batches:
            proofs = [made[b % distinct] for b in range(nb)]
            runs = [lambda: plonk.verify_proofs(ctx, pk, [inst] * nb, proofs, combine_seed=12345),
                    lambda: plonk.decide_proofs(ctx, pk, vparams, [inst] * nb, proofs),
                    lambda: plonk.decide_proofs(ctx, pk, vparams, [inst] * nb, proofs, combined=True, combine_seed=12345)]
            if not runs[0]().well_formed or not all(runs[1]()[0]) or not all(runs[2]()[0]):
                raise SystemExit("a proof of the device prover is not decided valid: refusing to time a wrong verifier")
            med = []
            for run in runs:
                med.append(statistics.median([timed(run)[0] for _ in range(args.reps)]))
            lines.append("%8d %14.3f %16.3f %16.3f %22.3f" % (nb, med[0], med[1], med[2], med[1] / nb))
        finish(lines, args.out)
        d_adv.free()
        vparams.free()
        pk.free()
        params.free()


if __name__ == "__main__":
    main()
