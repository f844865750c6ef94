#!/usr/bin/env python3
"""Time amdzk_check_witness at the metric shape (workloads.full_aadhaar_shape, k = 15) on one GPU and write
profiles/check_witness.txt.

    python tools/bench_check_witness.py [--k 15] [--reps 5] [--out FILE]

Reported: the FIRST call on a fresh key, which includes decoding the sigma columns back to (column, row); the median
of --reps later calls; one proof (amdzk_create_proof, median of --reps after one warm-up) on the same key, the same box
and in the same process, for scale; and the check's per-kernel table (amdzk_prof_dump). Host wall clock around blocking
calls. The witness satisfies the circuit: the report must be empty, or the run stops."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def fr_from_int(x):
    v = x * (1 << 256) % R
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_witness.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge

    pkg = ge.load_package()
    plonk, wl = pkg.plonk, pkg.workloads
    c = wl.full_aadhaar_shape(k=args.k)
    n = c.n
    with pkg.Context(0) as ctx:
        params = pkg.kzg.ParamsKZG.setup(ctx, c.k, fr_from_int(0x1234567890ABCDEF1234567))

        def resident(cols):  # canonical limbs up, Fr::from_raw on the device
            host = np.ascontiguousarray(wl.canon_limbs(cols))
            d = ctx.alloc(host.nbytes).upload(host)
            ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, d.ptr, host.size // 4))  # the buffer's own element count: an instance column is shorter than n
            return d

        d_fixed = resident(c.fixed)
        fixed = d_fixed.download((len(c.fixed), n, 4))
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

        def timed(fn):
            t0 = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t0) * 1e3, out

        first_ms, rep = timed(lambda: plonk.check_witness(ctx, pk, inst, d_adv))
        if not rep.ok:
            raise SystemExit("the satisfying witness has %d failing constraints: refusing to time a wrong check" % len(rep.failures))
        later = []
        for _ in range(args.reps):
            ms, rep = timed(lambda: plonk.check_witness(ctx, pk, inst, d_adv))
            assert rep.ok
            later.append(ms)
        ctx.prof_enable(True)
        ctx.prof_reset()
        plonk.check_witness(ctx, pk, inst, d_adv)
        ctx.sync()
        prof = ctx.prof_dump()
        ctx.prof_enable(False)
        plonk.create_proof(ctx, pk, inst, d_adv, seed=1)
        proofs = [timed(lambda s=s: plonk.create_proof(ctx, pk, inst, d_adv, seed=2 + s))[0] for s in range(args.reps)]
        lines = ["amdzk_check_witness, %s" % pkg.build_info()["text"],
                 "shape: full_aadhaar_shape k = %d: %d advice, %d fixed, %d instance columns, %d gate polynomials, %d lookups, %d permutation columns"
                 % (c.k, len(c.advice), len(c.fixed), len(c.instances), len(c.desc["gates"]), len(c.desc["lookups"]), len(c.desc["permutation_columns"])),
                 "host wall clock around blocking calls, one process, one GPU; the witness satisfies the circuit (empty report)",
                 "first call (includes the sigma decode, %d MiB of (column, row) pairs): %.3f ms"
                 % (len(c.desc["permutation_columns"]) * n * 8 >> 20, first_ms),
                 "later calls: median of %d = %.3f ms (min %.3f, max %.3f)" % (args.reps, statistics.median(later), min(later), max(later)),
                 "one proof on the same key (amdzk_create_proof, lanes): median of %d = %.3f ms (min %.3f, max %.3f)"
                 % (args.reps, statistics.median(proofs), min(proofs), max(proofs)),
                 "per-kernel table of one later call (kernels event-bracketed, so they run one at a time):"]
        for name, (cnt, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
            lines.append("  %-28s %4d launches %9.3f ms" % (name, cnt, ms))
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        d_adv.free()
        pk.free()
        params.free()


if __name__ == "__main__":
    main()
