#!/usr/bin/env python3
"""Time amdzk_poseidon_hash_dev on one GPU and write profiles/poseidon.txt.

    python tools/bench_poseidon.py [--reps 7] [--sweep] [--out FILE]

Shapes: t = 5, rate = 4, (r_f, r_p) = (8, 57), 950 inputs — the reference's nullifier — at n = 1, 64, 4096 and 65536 sponges
(--sweep: every power of two up to 65536, to place the crossovers), and t = 3, rate = 2, 2 inputs — a tree level — at
n = 2^20. Per shape: HIP-event time of the whole call with the inputs resident (amdzk_timer_*), median of --reps after two
warm-up calls. Beside each figure the single-core time of pos::sponge for the same sponges — this library's own 32-bit host
field code built with g++ -O2 (tools/poseidon_host_time.cpp), NOT the Rust crate — and the same divided by sixteen, which is
arithmetic, not a measurement. The constants are arbitrary values below r: the times do not depend on them."""
import argparse
import ctypes as C
import os
import random
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def random_fr(rs, count):
    """count x 4 words below the modulus (top word < 2^60: any such value is a valid Montgomery form)."""
    a = rs.randint(0, 1 << 62, size=(count, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] >>= np.uint64(2)
    return a


def host_us(exe, t, rate, r_f, r_p, length, per):
    return float(subprocess.check_output([exe, str(t), str(rate), str(r_f), str(r_p), str(length), str(per)], text=True).split()[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge

    pkg = ge.load_package()
    pm = pkg.poseidon
    rs = np.random.RandomState(5)
    py = random.Random(5)
    tmp = tempfile.mkdtemp(prefix="poseidon_host_time")
    exe = os.path.join(tmp, "poseidon_host_time")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tools", "poseidon_host_time.cpp")])
    big = [1 << i for i in range(17)] if args.sweep else [1, 64, 4096, 65536]
    shapes = [(5, 4, 8, 57, 950, big, 20), (3, 2, 8, 57, 2, [1 << 20], 20000)]
    lines = ["amdzk_poseidon_hash_dev, %s" % pkg.build_info()["text"],
             "HIP events around the whole call (inputs resident) on one GPU, one process; median of %d calls after 2 warm-up calls (min .. max)" % args.reps,
             "host = pos::sponge of this library's 8 x 32-bit field code, g++ -O2, ONE core, median of 7 samples; host/16 is that figure divided by 16"]
    with pkg.Context(0) as ctx:
        for t, rate, r_f, r_p, length, ns, per in shapes:
            hus = host_us(exe, t, rate, r_f, r_p, length, per)
            lines.append("t = %d, rate = %d, (r_f, r_p) = (%d, %d), %d inputs = %d permutations per sponge; host: %.1f us per sponge"
                         % (t, rate, r_f, r_p, length, length // rate + 1, hus))
            spec = pm.Spec(t, rate, r_f, r_p, [[py.randrange(pm.R) for _ in range(t)] for _ in range(r_f + r_p)],
                           [[py.randrange(pm.R) for _ in range(t)] for _ in range(t)])
            P = pm.Poseidon(ctx, spec)
            nmax = max(ns)
            chunk_rows = min(nmax, 1024)
            chunk = random_fr(rs, chunk_rows * length).reshape(chunk_rows, length, 4)
            d_in = ctx.alloc(nmax * length * 32)
            for off in range(0, nmax, chunk_rows):  # the same rows over and over: the time does not depend on the values
                ctx._chk(ctx.L.amdzk_dev_upload(ctx.h, C.c_void_p(d_in.ptr.value + off * length * 32), chunk.ctypes.data, chunk.nbytes))
            d_out = ctx.alloc(nmax * 32)
            won1 = won16 = None
            for n in ns:
                times = []
                for rep in range(args.reps + 2):
                    ctx.timer_start()
                    P.hash_many_dev(d_in, length, n, d_out, length=length)
                    ms = ctx.timer_stop()
                    if rep >= 2:
                        times.append(ms)
                med = statistics.median(times)
                h1, h16 = n * hus / 1000.0, n * hus / 16000.0
                lines.append("  n = %7d: %10.3f ms (%.3f .. %.3f), %10.3f us per sponge | host %11.3f ms, host/16 %11.3f ms"
                             % (n, med, min(times), max(times), 1000.0 * med / n, h1, h16))
                if won1 is None and med < h1:
                    won1 = n
                if won16 is None and med < h16:
                    won16 = n
            lines.append("  the device call is faster than one core from n = %s on and than sixteen cores (host/16) from n = %s on, among the n measured"
                         % (won1, won16))
            P.free()
            d_in.free()
            d_out.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
