#!/usr/bin/env python3
"""Time amdzk_verify_proofs at the metric shape (workloads.full_aadhaar_shape, k = 15) on one GPU and write
profiles/verify_batch.txt.

    python tools/verify_bench.py [--shape full|gate] [--k 15] [--reps 5] [--batches 1,8,64] [--vk] [--out FILE] [--append]

The proofs are made by the device prover in the same process (distinct seeds). For every batch size: the host wall clock
around the blocking call (median of --reps after one warm-up), in total and per proof; and, from one more call with every
kernel event-bracketed (amdzk_prof_*), the device time of the decode kernel and of the MSM's kernels, and that call's host
time (its wall clock minus both; bracketed kernels run one at a time). No pairing is computed and no pair is checked: that
is the test suite's business. Every status must be "well formed" or the run stops.

--shape gate times the smallest proofs instead: the one-gate circuit of tools/verify_mixed_bench.py at k = 4 (480 bytes, 15
elements), where the call is launches and host work and the decode launch takes one block per proof (--k is not read).

--vk adds the same calls through a verifying key (amdzk_verify_proofs_vk with pk.get_vk()), alternating with the pk route
rep by rep, as a second table: wall clock of both routes side by side. The two pairs must be equal word for word or the
run stops. --append adds the report to --out behind a blank line instead of replacing the file (profiles/vk.txt:
tools/vk_bench.py, then this tool with --vk --batches 1,64 --out profiles/vk.txt --append)."""
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
    ap.add_argument("--shape", choices=["full", "gate"], default="full", help="full_aadhaar_shape at --k, or the k = 4 gate circuit")
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--vk", action="store_true", help="also time the verifying-key route beside the proving key's")
    ap.add_argument("--append", action="store_true", help="add the report to --out instead of replacing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.txt"))
    args = ap.parse_args()
    batches = [int(v) for v in args.batches.split(",")]
    import __graft_entry__ as ge

    pkg = ge.load_package()
    plonk, wl = pkg.plonk, pkg.workloads
    if args.shape == "gate":
        from verify_mixed_bench import small_circuit
        c = small_circuit(plonk, wl, 4, 0, 0)
    else:
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
        distinct = min(max(batches), 8)  # the cost of a proof does not depend on its bytes: a large batch repeats these
        made = [plonk.create_proof(ctx, pk, inst, d_adv, seed=100 + s) for s in range(distinct)]

        def timed(fn):
            t0 = time.perf_counter()
            out = fn()
            return (time.perf_counter() - t0) * 1e3, out

        lines = ["amdzk_verify_proofs, %s" % pkg.build_info()["text"],
                 "shape: %s k = %d: %d advice, %d fixed, %d instance columns, %d lookups, %d permutation columns; proof of %d bytes"
                 % ("gate" if args.shape == "gate" else "full_aadhaar_shape", c.k, len(c.advice), len(c.fixed), len(c.instances), len(c.desc["lookups"]), len(c.desc["permutation_columns"]), len(made[0])),
                 "Blake2b transcript, SHPLONK; proofs by the device prover in the same process; one process, one GPU",
                 "wall: host wall clock around the blocking call, median of %d after one warm-up" % args.reps,
                 "decode / msm / host: one more call with every kernel event-bracketed (kernels then run one at a time):",
                 "  decode = proof_decode, msm = every other kernel of the call, host = that call's wall clock minus both",
                 "%8s %12s %14s %12s %12s %12s" % ("n_proofs", "wall ms", "wall ms/proof", "decode ms", "msm ms", "host ms")]
        for nb in batches:
            proofs = [made[b % distinct] for b in range(nb)]
            run = lambda: plonk.verify_proofs(ctx, pk, [inst] * nb, proofs, combine_seed=12345)
            g = run()
            if not g.well_formed:
                raise SystemExit("a proof of the device prover is reported malformed: refusing to time a wrong verifier")
            wall = [timed(run)[0] for _ in range(args.reps)]
            ctx.prof_enable(True)
            ctx.prof_reset()
            prof_wall, _ = timed(run)
            ctx.sync()
            prof = ctx.prof_dump()
            ctx.prof_enable(False)
            decode = sum(ms for name, (_, ms) in prof.items() if name == "proof_decode")
            msm = sum(ms for name, (_, ms) in prof.items() if name != "proof_decode")
            w = statistics.median(wall)
            lines.append("%8d %12.3f %14.3f %12.3f %12.3f %12.3f" % (nb, w, w / nb, decode, msm, prof_wall - decode - msm))
        if args.vk:
            vk = pk.get_vk()
            lines += ["", "amdzk_verify_proofs_vk beside amdzk_verify_proofs: the same calls, the routes alternating rep by rep; wall ms, median of %d" % args.reps,
                      "%8s %12s %12s %16s %16s" % ("n_proofs", "pk wall ms", "vk wall ms", "pk ms/proof", "vk ms/proof")]
            for nb in batches:
                proofs = [made[b % distinct] for b in range(nb)]
                runs = {key: (lambda key=key: plonk.verify_proofs(ctx, key, [inst] * nb, proofs, combine_seed=12345)) for key in (pk, vk)}
                a, b = runs[pk](), runs[vk]()
                if not (np.array_equal(a.lhs, b.lhs) and np.array_equal(a.rhs, b.rhs) and a.statuses == b.statuses and b.well_formed):
                    raise SystemExit("the verifying key's route disagrees with the proving key's: refusing to time it")
                wall = {pk: [], vk: []}
                for _ in range(args.reps):
                    for key in (pk, vk):
                        wall[key].append(timed(runs[key])[0])
                wp, wv = statistics.median(wall[pk]), statistics.median(wall[vk])
                lines.append("%8d %12.3f %12.3f %16.3f %16.3f" % (nb, wp, wv, wp / nb, wv / nb))
            vk.free()
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(("\n" if args.append else "") + text)
        d_adv.free()
        pk.free()
        params.free()


if __name__ == "__main__":
    main()
