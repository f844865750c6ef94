#!/usr/bin/env python3
"""Time amdzk_create_proof_batch_opts on one GPU against the same proofs as consecutive amdzk_create_proof_opts calls and
write profiles/batch_opts.txt.

    python tools/bench_batch_opts.py [--k 15] [--proofs 10] [--reps 10] [--out FILE]

The circuit is tests/phased_circuits.rlc_circuit with three phases (two phase-0 columns, one column in each later phase,
two challenges, a gate per phase, a lookup and copies), one serial key and --proofs - 1 workspace clones, a seed per proof.
Both paths run the same callbacks, which return at once: the later phases' columns are resident before the call (the prover
does not look at their values), so the figures are the driver's — copy-in, blinding, transforms, commitments, transcript and
host waits — and not a synthesize's. HIP-event time of the whole call (amdzk_timer_*) or of the whole loop of single calls,
median of --reps after two warm-ups, one process."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--proofs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_opts.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge
    import phased_circuits as PC
    import zkutil as zu

    pkg = ge.load_package()
    plonk = pkg.plonk
    O = zu.Oracle()
    B = args.proofs
    c = PC.rlc_circuit(plonk, args.k, seed=1, three_phases=True)
    seeds = list(range(1, B + 1))
    lines = ["amdzk_create_proof_batch_opts, %s" % pkg.build_info()["text"],
             "%d proofs of the three-phase rlc_circuit at k = %d (4 advice columns in phases 0, 0, 1, 2; 2 challenges), one serial key and %d clones"
             % (B, args.k, B - 1),
             "HIP events around the whole call / the whole loop on one GPU, one process; median of %d after 2 warm-ups (min, max); callbacks return at once"
             % args.reps]
    with pkg.Context(0) as ctx:
        params = pkg.kzg.ParamsKZG.setup(ctx, c.k, zu.fr_from_int(0x1234567890ABCDEF1234567))
        fixed = np.stack([zu.ints_to_fr(O, col) for col in c.fixed])
        pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, zu.fr_from_int(77), flags=plonk.KEYGEN_SERIAL)
        pks = [pk] + [pk.clone_workspace() for _ in range(B - 1)]
        d_adv = []
        for b in range(B):
            adv, fill = (c.advice, c.fill) if b == 0 else c.witness_for(100 + b)
            adv = [list(col) for col in adv]
            fill(1, {0: 3, 1: 5}, adv)  # any values: resident before the call
            fill(2, {0: 3, 1: 5}, adv)
            arr = np.stack([zu.ints_to_fr(O, col) for col in adv])
            d_adv.append(ctx.alloc(arr.nbytes).upload(arr))
        inst = [[] for _ in range(B)]
        calls = []

        def batch():
            return plonk.create_proof_batch_opts(ctx, pks, inst, d_adv, seeds=seeds, synthesize=lambda p, w, ch, s: calls.append(p))

        def singles():
            return [plonk.create_proof_opts(ctx, [pks[b]], [inst[b]], [d_adv[b]], seed=seeds[b], synthesize=lambda p, ch, s: calls.append(p))
                    for b in range(B)]

        results = {}
        for name, fn in (("one amdzk_create_proof_batch_opts call", batch), ("%d consecutive amdzk_create_proof_opts calls" % B, singles)):
            times = []
            for rep in range(args.reps + 2):
                del calls[:]
                ctx.timer_start()
                results[name] = fn()
                ms = ctx.timer_stop()
                if rep >= 2:
                    times.append(ms)
            med = statistics.median(times)
            lines.append("%-48s %9.3f ms per %d proofs (%.3f .. %.3f), %8.3f ms per proof, %d callbacks"
                         % (name + ":", med, B, min(times), max(times), med / B, len(calls)))
        a, b = results.values()
        lines.append("the two paths' bytes are equal: %s" % (list(a) == list(b) and all(isinstance(p, bytes) for p in a)))
        for d in d_adv:
            d.free()
        for h in pks[1:]:
            h.free()
        pk.free()
        params.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
