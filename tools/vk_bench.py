#!/usr/bin/env python3
"""Measure amdzk_keygen_vk beside amdzk_keygen_ex at the metric shape (workloads.full_aadhaar_shape, k = 15) on one GPU.

    python tools/vk_bench.py [--k 15] [--reps 5] [--out profiles/vk.txt]

profiles/vk.txt is this report followed by `python tools/verify_bench.py --vk --batches 1,64 --out profiles/vk.txt --append`.

One process, one SRS. Per rep, in this order: keygen_vk from the mapping (the verifying key alone), keygen_vk from the sigma
columns (the same key without the host loop that turns the mapping into sigma values), then keygen_ex (the proving key), each
from the same fixed columns, each freed before the next. For each: the host wall clock around the blocking C call and a
device sync, and the device memory the call holds when it returns — free memory (hipMemGetInfo, through
torch.cuda.mem_get_info) before the call minus after it — and, for keygen_vk, the most it held while it ran, which the
code states: (F + S) * 2^k * 32 bytes of Lagrange columns. Medians of --reps after one warm-up of each. The three keys'
files must be equal or the run stops."""
import argparse
import ctypes as C
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vk.txt"))
    args = ap.parse_args()
    import torch

    import __graft_entry__ as ge

    pkg = ge.load_package()
    plonk, wl = pkg.plonk, pkg.workloads
    c = wl.full_aadhaar_shape(k=args.k)
    n, F, S = c.n, len(c.fixed), len(c.desc["permutation_columns"])
    free = lambda: torch.cuda.mem_get_info(0)[0]
    with pkg.Context(0) as ctx:
        params = pkg.kzg.ParamsKZG.setup(ctx, c.k, fr_from_int(0x1234567890ABCDEF1234567))
        host = np.ascontiguousarray(wl.canon_limbs(c.fixed))
        d = ctx.alloc(host.nbytes).upload(host)
        ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, d.ptr, host.size // 4))
        fixed = d.download((F, n, 4))
        d.free()
        tr = fr_from_int(123456789)
        first = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, tr, flags=0)
        sigma = first.export(1)
        first.free()
        # the C calls themselves, on arrays made once: the Python mirror's own share (a nested list of 2 * S * 2^k integers
        # into an array, for one) is not what is measured
        cc, keep = plonk.flatten_circuit(c.desc)
        mp = np.ascontiguousarray(np.array(c.assembly.mapping, dtype=np.uint32).reshape(-1, n, 2))
        fixed, sigma = np.ascontiguousarray(fixed), np.ascontiguousarray(sigma)

        def call_vk(mapping, sig):
            h = C.c_void_p()
            ctx._chk(ctx.L.amdzk_keygen_vk(ctx.h, params.h, C.byref(cc), None, fixed.ctypes.data, mapping, sig, tr.ctypes.data, C.byref(h)))
            return plonk.VerifyingKey(ctx, h, c.desc)

        def call_ex():
            pk = object.__new__(plonk.ProvingKey)
            pk.ctx, pk.params, pk.desc, pk.h = ctx, params, c.desc, C.c_void_p()
            ctx._chk(ctx.L.amdzk_keygen_ex(ctx.h, params.h, C.byref(cc), fixed.ctypes.data, mp.ctypes.data, tr.ctypes.data, 0, C.byref(pk.h)))
            return pk

        makers = {"keygen_vk": lambda: call_vk(mp.ctypes.data, None), "keygen_vk_sigma": lambda: call_vk(None, sigma.ctypes.data), "keygen_ex": call_ex}
        wall, held, files = {m: [] for m in makers}, {m: [] for m in makers}, {}
        for rep in range(args.reps + 1):  # rep 0 warms up (the prefix basis of the SRS, the ctx's scratch)
            for name, make in makers.items():
                ctx.sync()
                before = free()
                t0 = time.perf_counter()
                key = make()
                ctx.sync()
                ms = (time.perf_counter() - t0) * 1e3
                after = free()
                if rep:
                    wall[name].append(ms)
                    held[name].append(before - after)
                else:
                    vk = key if name != "keygen_ex" else key.get_vk()
                    files[name] = vk.write()
                    if vk is not key:
                        vk.free()
                key.free()
        if not files["keygen_vk"] == files["keygen_vk_sigma"] == files["keygen_ex"]:
            raise SystemExit("keygen_vk's key is not the proving key's: refusing to report")
        mib = lambda b: b / (1 << 20)
        lines = ["amdzk_keygen_vk beside amdzk_keygen_ex, %s" % pkg.build_info()["text"],
                 "shape: full_aadhaar_shape k = %d: %d fixed, %d permutation columns, %d advice columns, %d lookups; cs_degree %d"
                 % (c.k, F, S, len(c.advice), len(c.desc["lookups"]), c.desc["cs_degree"]),
                 "one process, one GPU, one SRS; per rep keygen_vk (mapping), keygen_vk (sigma columns), keygen_ex(flags = 0), each freed before the next; medians of %d after a warm-up of each"
                 % args.reps,
                 "wall: host wall clock around the blocking call and a sync; held: hipMemGetInfo free before the call minus after it",
                 "%-16s %12s %14s" % ("call", "wall ms", "held MiB")] + [
                 "%-16s %12.1f %14.1f" % (name, statistics.median(wall[name]), mib(statistics.median(held[name]))) for name in makers] + [
                 "keygen_vk while it runs: (F + S) * 2^k * 32 B = %.1f MiB of Lagrange columns (from the code, not measured)" % mib((F + S) * n * 32),
                 "verifying-key file: %d bytes" % len(files["keygen_vk"])]
        text = "\n".join(lines) + "\n"
        sys.stdout.write(text)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        params.free()


if __name__ == "__main__":
    main()
