#!/usr/bin/env python3
"""Time amdzk_witness_run on one GPU at the scale of the benchmarked shape and write profiles/witness.txt.

    python tools/bench_witness.py [--k 15] [--columns 141] [--batches 1,10,64] [--reps 10] [--out FILE]

The program is synthetic: columns x 2^k nodes, EVERY node assigned to a cell — a few hundred inputs, one chain of 10^4
narrow levels (a hash or a modular exponentiation: one fused single-workgroup launch), and the rest in wide levels that mix
field products, sums, differences and BITS. Per batch: HIP-event time of the whole call (amdzk_timer_*: input staging,
every launch, the copy back of the publics, the host waits), median of --reps after two warm-up calls; the launches and
workspace bytes of amdzk_witness_plan; and, for the route this feature replaces, the time to upload the same cells from
host memory with amdzk_dev_upload."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

CHAIN = 10_000
N_INPUTS = 256
WIDE_LEVELS = 24


def synthetic(W, wm, k, columns, seed=1):
    """(program, number of cells): nodes built as arrays (the builder's methods one by one would take minutes in Python)."""
    n = 1 << k
    total = columns * n
    rs = np.random.RandomState(seed)
    p = W(k, columns)
    p.n_inputs = N_INPUTS
    p.constants = [1, 3, (1 << 64) - 1, 1 << 200]
    nodes = np.zeros((total, 4), dtype=np.uint32)
    nodes[:N_INPUTS, 0], nodes[:N_INPUTS, 1] = wm.INPUT, np.arange(N_INPUTS)
    c0 = N_INPUTS
    nodes[c0:c0 + 4, 0], nodes[c0:c0 + 4, 1] = wm.CONST, np.arange(4)
    at = c0 + 4
    # the narrow chain: x <- x * y, x <- x + c alternately
    idx = np.arange(at, at + CHAIN)
    nodes[idx, 0] = np.where((idx - at) % 2 == 0, wm.MUL, wm.ADD)
    nodes[idx, 1] = idx - 1
    nodes[at, 1] = 0
    nodes[idx, 2] = np.where((idx - at) % 2 == 0, 1, c0 + 1)
    at += CHAIN
    leaves = N_INPUTS + 4
    prev_lo, prev_hi = 0, leaves  # the level before: the leaves first
    rest = total - at
    for lv in range(WIDE_LEVELS):
        w = rest // WIDE_LEVELS + (1 if lv < rest % WIDE_LEVELS else 0)
        idx = np.arange(at, at + w)
        op = np.array([wm.MUL, wm.ADD, wm.BITS, wm.SUB, wm.MUL, wm.BITS], dtype=np.uint32)[(idx + lv) % 6]
        a = rs.randint(prev_lo, prev_hi, size=w)
        b = rs.randint(0, prev_hi, size=w)  # anywhere earlier among the leaves and the wide levels
        b = np.where((b >= leaves) & (b < leaves + CHAIN), b % leaves, b)  # not into the chain: the wide levels stay shallow
        lo = rs.randint(0, 200, size=w)
        ln = rs.randint(1, 57, size=w)
        nodes[idx, 0], nodes[idx, 1] = op, a
        nodes[idx, 2] = np.where(op == wm.BITS, lo, b)
        nodes[idx, 3] = np.where(op == wm.BITS, ln, 0)
        prev_lo, prev_hi = at, at + w
        at += w
    assert at == total
    p.nodes = nodes
    cells = np.zeros((total, 3), dtype=np.uint32)
    cells[:, 0] = np.arange(total)
    cells[:, 1] = np.arange(total) >> k
    cells[:, 2] = np.arange(total) & (n - 1)
    p.cells = cells
    p.publics = [total - 1, c0 + 4 + CHAIN - 1]
    return p, total


def random_fr(rs, count):
    """count x 4 words below the modulus (top word < 2^60: any such value is a valid Montgomery form)."""
    a = rs.randint(0, 1 << 62, size=(count, 4), dtype=np.int64).astype(np.uint64)
    a[:, 3] >>= np.uint64(2)
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--columns", type=int, default=141)
    ap.add_argument("--batches", default="1,10,64")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "witness.txt"))
    args = ap.parse_args()
    import __graft_entry__ as ge

    pkg = ge.load_package()
    wm = pkg.witness
    prog, total = synthetic(wm.WitnessProgram, wm, args.k, args.columns)
    batches = [int(b) for b in args.batches.split(",")]
    rs = np.random.RandomState(2)
    lines = ["amdzk_witness_run, %s" % pkg.build_info()["text"],
             "program: %d advice columns x 2^%d rows = %d nodes, every node a cell; %d inputs per proof; one chain of %d narrow levels, %d wide levels"
             % (args.columns, args.k, total, N_INPUTS, CHAIN, WIDE_LEVELS),
             "HIP events around the whole call on one GPU, one process; median of %d calls after 2 warm-up calls (min, max)" % args.reps]
    with pkg.Context(0) as ctx:
        cw = prog.compile(ctx)
        col_bytes = total * 32
        d_adv = []
        for B in batches:
            while len(d_adv) < B:
                d_adv.append(ctx.alloc(col_bytes))
            pl = prog.plan(B)
            inputs = [random_fr(rs, N_INPUTS) for _ in range(B)]
            times = []
            for rep in range(args.reps + 2):
                ctx.timer_start()
                cw.run(inputs, d_adv[:B])
                ms = ctx.timer_stop()
                if rep >= 2:
                    times.append(ms)
            med = statistics.median(times)
            lines.append("batch %3d: %9.3f ms per batch (%.3f .. %.3f), %8.3f ms per proof, %d levels, %d launches, workspace %d bytes (%.2f GiB)"
                         % (B, med, min(times), max(times), med / B, pl["levels"], pl["launches"], pl["scratch_bytes"], pl["scratch_bytes"] / 2**30))
            # the route this replaces: the same cells, synthesized by the host, uploaded from pageable host memory
            host = np.zeros(col_bytes // 8, dtype=np.uint64)
            host[:] = 0x0123456789ABCDEF
            ups = []
            for rep in range(args.reps + 2):
                ctx.timer_start()
                for b in range(B):
                    d_adv[b].upload(host)
                ms = ctx.timer_stop()
                if rep >= 2:
                    ups.append(ms)
            um = statistics.median(ups)
            lines.append("           amdzk_dev_upload of the same %d x %d bytes: %9.3f ms per batch (%.3f .. %.3f), %8.3f ms per proof"
                         % (B, col_bytes, um, min(ups), max(ups), um / B))
        ctx.prof_enable(True)
        ctx.prof_reset()
        cw.run([random_fr(rs, N_INPUTS)], d_adv[:1])
        prof = ctx.prof_dump()
        ctx.prof_enable(False)
        lines.append("per-kernel table of one call at batch 1 (kernels event-bracketed, so they run one at a time):")
        for name, (cnt, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1]):
            if name.startswith("wit_"):
                lines.append("  %-18s %4d launches %9.3f ms" % (name, cnt, ms))
        cw.free()
        for d in d_adv:
            d.free()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
