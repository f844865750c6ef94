#!/usr/bin/env python3
"""Measure the table-free MSM (amdzk_msm_g1_bases*) on one GPU and write profiles/msm_foreign_bases.txt.

    python tools/bench_msm_bases.py [--sizes 10,14,16,18,20,22] [--parent-lib ab/libamdzk_old.so] [--out FILE]

Per size one child process under its own time limit; the first child that fails ends the run (nothing more is started on
a device that has just misbehaved). Every figure is the median of --reps timed calls after --warmup untimed ones, host
wall clock around blocking calls, and the two sides of every comparison ALTERNATE inside one process on one device.

  1. one-shot route: amdzk_srs_upload + amdzk_msm_g1 + amdzk_srs_free (the only route before amdzk_msm_g1_bases; taken from
     --parent-lib, a libamdzk.so built from that commit: the run refuses to start without it) against
     amdzk_msm_g1_bases, host buffers on both sides; the break-even number of MSMs after which building a table wins.
  2. resident: amdzk_msm_g1_dev over a table already built against amdzk_msm_g1_bases_dev over resident bases, with the
     per-kernel tables of both (amdzk_prof_dump).
  3. window widths 8..16 (AMDZK_MSM_BASES_C) and the per-kernel table of the default width, msm_accum_final called out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def random_fr(n, seed):
    """n Montgomery-form scalars: 252 random bits as the limbs (always below r)."""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) << np.uint64(1)
    a[:, 3] &= np.uint64((1 << 60) - 1)
    return np.ascontiguousarray(a)


def bind_parent(path):
    """The handful of entry points of the one-shot window-table route, from a library that may predate the current header."""
    L = C.CDLL(path)
    vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    for name, res, args in (("amdzk_init", i32, [i32, C.POINTER(vp)]), ("amdzk_destroy", None, [vp]),
                            ("amdzk_srs_upload", i32, [vp, vp, vp, u32, C.POINTER(vp)]), ("amdzk_srs_free", None, [vp, vp]),
                            ("amdzk_msm_g1", i32, [vp, vp, i32, vp, sz, vp]), ("amdzk_version", i32, [])):
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


def median_ms(samples):
    return statistics.median(samples) * 1e3


def prof_of(ctx, fn):
    ctx.prof_reset()
    ctx.prof_enable(True)
    fn()
    table = ctx.prof_dump()
    ctx.prof_enable(False)
    return {k: round(v[1], 4) for k, v in sorted(table.items())}


def child(args):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    ar = pkg.arithmetic
    k = args.child
    n = 1 << k
    res = {"k": k}
    with pkg.Context(0) as ctx:
        # bases: tau powers built on the device (any points do: the work of an MSM does not depend on them)
        tau = np.array([0x1234567, 0, 0, 0], dtype=np.uint64)
        params = pkg.kzg.ParamsKZG.setup(ctx, k, tau)
        g = np.ascontiguousarray(params.get_g())
        s = random_fr(n, seed=1000 + k)
        plan = ar.multiexp_bases_plan(1, n)
        res["plan"] = plan

        # ---- 3. window widths (the variable is read at every call)
        sweep = {}
        for c in range(8, 17):
            os.environ["AMDZK_MSM_BASES_C"] = str(c)
            assert ar.multiexp_bases_plan(1, n)["window_bits"] == c
            d_s = ctx.alloc(s.nbytes).upload(s)
            d_b = ctx.alloc(g.nbytes).upload(g)
            ref = None
            t = []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                out = ar.best_multiexp_bases_dev(ctx, d_s, d_b, 1, n)
                if i >= args.warmup:
                    t.append(time.perf_counter() - t0)
                ref = out if ref is None else ref
                assert np.array_equal(out, ref)
            pk = prof_of(ctx, lambda: ar.best_multiexp_bases_dev(ctx, d_s, d_b, 1, n))
            sweep[c] = {"ms": round(median_ms(t), 4), "final_ms": pk.get("msm_accum_final", 0.0), "l1_ms": pk.get("msm_accum_l1", 0.0),
                        "combine_ms": pk.get("msm_window_combine", 0.0), "point": [int(x) for x in ref[0][:4]]}
            d_s.free(); d_b.free()
        del os.environ["AMDZK_MSM_BASES_C"]
        assert len({tuple(v["point"]) for v in sweep.values()}) == 1, "the widths disagree on the point"
        for v in sweep.values():
            del v["point"]
        res["sweep"] = sweep

        # ---- 2. resident table against resident bases, alternating
        d_s = ctx.alloc(s.nbytes).upload(s)
        d_b = ctx.alloc(g.nbytes).upload(g)
        t_tab, t_free = [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            a = ar.best_multiexp_dev(ctx, params.h, 0, d_s, 1, n)
            t1 = time.perf_counter()
            b = ar.best_multiexp_bases_dev(ctx, d_s, d_b, 1, n)
            t2 = time.perf_counter()
            assert np.array_equal(a, b), "table route and table-free route disagree"
            if i >= args.warmup:
                t_tab.append(t1 - t0)
                t_free.append(t2 - t1)
        res["resident"] = {"table_ms": round(median_ms(t_tab), 4), "bases_ms": round(median_ms(t_free), 4),
                           "table_kernels": prof_of(ctx, lambda: ar.best_multiexp_dev(ctx, params.h, 0, d_s, 1, n)),
                           "bases_kernels": prof_of(ctx, lambda: ar.best_multiexp_bases_dev(ctx, d_s, d_b, 1, n))}
        d_s.free(); d_b.free()
        params.free()

        # ---- 1. the one-shot route: table built, used once, freed — against the table-free call; host buffers
        if k in args.oneshot:
            P = bind_parent(os.path.abspath(args.parent_lib))
            ph = C.c_void_p()
            assert P.amdzk_init(0, C.byref(ph)) == 0
            res["oneshot_lib"] = "parent build, ABI %d" % P.amdzk_version()
            out_old = np.zeros(12, np.uint64)
            t_old, t_new = [], []
            for i in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                srs = C.c_void_p()
                assert P.amdzk_srs_upload(ph, ptr(g), None, k, C.byref(srs)) == 0
                assert P.amdzk_msm_g1(ph, srs, 0, ptr(s), n, ptr(out_old)) == 0
                P.amdzk_srs_free(ph, srs)
                t1 = time.perf_counter()
                out_new = ar.best_multiexp_bases(ctx, s, g)
                t2 = time.perf_counter()
                assert np.array_equal(out_old, out_new), "one-shot table route and table-free route disagree"
                if i >= args.warmup:
                    t_old.append(t1 - t0)
                    t_new.append(t2 - t1)
            P.amdzk_destroy(ph)
            res["oneshot"] = {"table_ms": round(median_ms(t_old), 4), "bases_ms": round(median_ms(t_new), 4)}
    print("RESULT " + json.dumps(res), flush=True)


def fmt_kernels(d):
    return "  ".join("%s %.3f" % (k, v) for k, v in d.items())


def report(results, args):
    L = ["python tools/bench_msm_bases.py --sizes %s --reps %d --warmup %d   (one MI355X, one process per size; median of %d timed calls after %d "
         "untimed, host wall clock around blocking calls, both sides of a comparison alternating in one process; uniform scalars, one column)"
         % (",".join(str(r["k"]) for r in results), args.reps, args.warmup, args.reps, args.warmup), ""]
    L.append("1. one-shot: amdzk_srs_upload + amdzk_msm_g1 + amdzk_srs_free against amdzk_msm_g1_bases, host buffers (ms per call)")
    for r in results:
        if "oneshot" in r:
            o, rs = r["oneshot"], r["resident"]
            # a table pays for itself after m MSMs:  build + m * table_msm  <  m * bases_msm. Both one-shot calls pay the same
            # transfers, so build = (one-shot table route - one-shot table-free call) + (resident table-free - resident table)
            gain = rs["bases_ms"] - rs["table_ms"]
            build = o["table_ms"] - o["bases_ms"] + gain
            even = "never (the table-free call is not slower per MSM)" if gain <= 0 else "%.1f MSMs" % (build / gain)
            L.append("2^%-2d table route %10.3f   table-free %9.3f   ratio %6.1f x   [%s]   table pays for itself after %s"
                     % (r["k"], o["table_ms"], o["bases_ms"], o["table_ms"] / o["bases_ms"], r["oneshot_lib"], even))
    L += ["", "2. resident: amdzk_msm_g1_dev over a table already built against amdzk_msm_g1_bases_dev over resident bases (ms per call)"]
    for r in results:
        rs = r["resident"]
        L.append("2^%-2d table %8.3f   table-free %8.3f   %.2f x" % (r["k"], rs["table_ms"], rs["bases_ms"], rs["bases_ms"] / rs["table_ms"]))
        L.append("     table      kernels (ms, event-bracketed, one call): " + fmt_kernels(rs["table_kernels"]))
        L.append("     table-free kernels (ms, event-bracketed, one call): " + fmt_kernels(rs["bases_kernels"]))
    L += ["", "3. window widths (AMDZK_MSM_BASES_C), resident call, ms; * = the width amdzk_msm_g1_bases_plan picks. Per width: whole call | "
          "msm_accum_l1 | msm_accum_final | msm_window_combine (the last three event-bracketed in a profiled call)"]
    for r in results:
        L.append("2^%-2d  default c = %d, %d windows, workspace %.1f MiB" % (r["k"], r["plan"]["window_bits"], r["plan"]["windows"], r["plan"]["scratch_bytes"] / 2 ** 20))
        for c, v in sorted(r["sweep"].items(), key=lambda kv: int(kv[0])):
            L.append("     c=%-2s%s %9.3f | l1 %8.3f | final %7.3f | combine %6.3f"
                     % (c, "*" if int(c) == r["plan"]["window_bits"] else " ", v["ms"], v["l1_ms"], v["final_ms"], v["combine_ms"]))
    return "\n".join(L) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,14,16,18,20,22")
    ap.add_argument("--oneshot-sizes", default="16,20,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "ab", "libamdzk_old.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_foreign_bases.txt"))
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per size")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.oneshot = [int(x) for x in args.oneshot_sizes.split(",") if x]
    if args.child is not None:
        return child(args)
    if args.oneshot and not os.path.exists(args.parent_lib):
        sys.exit("%s not found: comparison 1 is against the library of the commit before amdzk_msm_g1_bases (build it from that commit "
                 "and pass --parent-lib), or leave it out with --oneshot-sizes ''" % args.parent_lib)
    results = []
    for k in [int(x) for x in args.sizes.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(k), "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--oneshot-sizes", args.oneshot_sizes, "--parent-lib", args.parent_lib]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit("size 2^%d ran over its %d s: stopping here" % (k, args.step_timeout))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.exit("size 2^%d failed (exit %d): stopping here\n%s" % (k, r.returncode, r.stdout[-3000:]))
        results.append(json.loads(line[-1][7:]))
        print("2^%d done" % k, flush=True)
    text = report(results, args)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
