#!/usr/bin/env python3
"""Time amdzk_srs_check on one GPU and write profiles/srs_check.txt.

    python tools/srs_check_bench.py [--ks 15,22] [--reps 5] [--out FILE]

Per k: ParamsKZG.setup and g2_setup with a fixed trapdoor, one warm-up call, then the device time between amdzk_timer_start and
amdzk_timer_stop around the blocking call (both host halves — the two membership tests and the two g2_prepare — are inside it)
and the host wall clock around it, medians of --reps; then one more call with every kernel event-bracketed (amdzk_prof_*) for
the per-kernel table. Every report must be clean or the run stops."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
TAU = 0x1234567890ABCDEF1234567


def fr_from_int(x):
    v = x * (1 << 256) % R
    return np.array([(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="15,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "srs_check.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge

    pkg = ge.load_package()
    kzg = pkg.kzg
    lines = ["amdzk_srs_check, %s" % pkg.build_info()["text"], "one process, one GPU; all four checks; medians of %d after one warm-up per k" % args.reps, ""]
    with pkg.Context(0) as ctx:
        g2, s_g2 = kzg.g2_setup(ctx, fr_from_int(TAU))
        t0 = time.perf_counter()
        assert kzg.g2_check(g2) == 0 and kzg.g2_check(s_g2) == 0
        lines.append("host: two amdzk_g2_check ([r]Q = O): %.2f ms" % ((time.perf_counter() - t0) * 1e3))
        for k in [int(v) for v in args.ks.split(",")]:
            params = kzg.ParamsKZG.setup(ctx, k, fr_from_int(TAU))

            def run(seed):
                rep = params.check(g2, s_g2, seed=seed)
                assert rep.ran == 15 and rep.failed == 0, (k, rep.ran, rep.failed)

            run(0)
            dev, wall = [], []
            for i in range(args.reps):
                ctx.timer_start()
                t0 = time.perf_counter()
                run(1 + i)
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(ctx.timer_stop())
            ctx.prof_reset()
            ctx.prof_enable(True)
            run(99)
            prof = ctx.prof_dump()
            ctx.prof_enable(False)
            ctx.prof_reset()
            lines.append("")
            lines.append("k = %d: %.2f ms between the timer events, %.2f ms wall clock (min %.2f, max %.2f)" %
                         (k, statistics.median(dev), statistics.median(wall), min(wall), max(wall)))
            lines.append("  %-28s %8s %12s" % ("kernel (profiled call)", "launches", "ms"))
            for name, (n, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
                lines.append("  %-28s %8d %12.3f" % (name, n, ms))
            lines.append("  %-28s %8s %12.3f" % ("sum of kernels", "", sum(ms for _, ms in prof.values())))
            params.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
