#!/usr/bin/env python3
"""Measure what starting from a key file costs against keygen from the mapping, on one GPU.

    python tools/measure_pk_load.py [--shape full] [--out profiles/pk_file_load.txt]

Two child processes, each under its own time limit, the second only if the first ended well; each initialises the device,
sets up the same SRS, and then times its FIRST call (a cold one: nothing of the key is cached on the device or in the
library), host wall clock around the blocking call and a device sync:

  keygen  builds the circuit of bench.py's --shape (configure, fixed assignment, copy constraints: also timed, it is the
          host work a process that starts from a key file does not repeat), ProvingKey(...) from Assembly.mapping, then
          pk.write() into a file.
  read    reads that file from disk, blob_info (pure host: the digest over the whole file), then amdzk_pk_read. No proof is
          made: the two keys are the same key (tests/test_gpu_pk_blob.py), so what follows costs the same.

The report goes to --out and to stdout.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S_INT = 0x0123456789ABCDEF0123456789ABCDEF  # the SRS secret and transcript_repr of bench.py
TR_INT = 0xA11CE
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def mont_limbs(v):
    import numpy as np
    return np.array([((v << 256) % R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def child(args):
    import ctypes as C

    import numpy as np

    import __graft_entry__ as ge
    pkg = ge.load_package()
    plonk, wl = pkg.plonk, pkg.workloads
    res = {"mode": args.child, "library": pkg.build_info()}
    ctx = pkg.Context(0)
    k = wl.SHAPES[args.shape]["k"]
    t0 = time.perf_counter()
    params = pkg.kzg.ParamsKZG.setup(ctx, k, mont_limbs(S_INT % R))
    ctx.sync()
    res["srs_setup_s"] = time.perf_counter() - t0
    if args.child == "keygen":
        t0 = time.perf_counter()
        c = wl.make(args.shape)
        res["circuit_host_s"] = time.perf_counter() - t0  # configure + fixed assignment + copy constraints, in Python
        lim = wl.canon_limbs(c.fixed)
        buf = ctx.alloc(lim.nbytes).upload(lim)
        ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, buf.ptr, lim.size // 4))
        fixed = buf.download(lim.shape)
        buf.free()
        ctx.sync()
        t0 = time.perf_counter()
        pk = plonk.ProvingKey(ctx, params, c.desc, fixed, c.assembly.mapping, mont_limbs(TR_INT))
        ctx.sync()
        res["keygen_from_mapping_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        blob = pk.write()
        res["write_s"] = time.perf_counter() - t0
        with open(args.file, "wb") as f:
            f.write(blob)
        res.update(blob_bytes=len(blob), num_fixed=c.desc["num_fixed"], num_perm_columns=len(c.desc["permutation_columns"]), k=k)
    else:
        t0 = time.perf_counter()
        blob = np.fromfile(args.file, dtype=np.uint8)
        res["file_from_disk_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        shape = plonk.blob_info(blob)
        res["blob_info_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_pk_read(ctx.h, params.h, blob.ctypes.data, blob.size, plonk._env_keygen_flags(), C.byref(h)))
        ctx.sync()
        res["amdzk_pk_read_s"] = time.perf_counter() - t0
        ctx.L.amdzk_pk_free(ctx.h, h)
        t0 = time.perf_counter()
        pk = plonk.ProvingKey.read(ctx, params, blob)  # the second read of this process: the Python mirror's own share on top
        ctx.sync()
        res["ProvingKey_read_second_s"] = time.perf_counter() - t0
        res.update(blob_bytes=int(blob.size), **shape)
    pk.free()
    params.free()
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="full")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pk_file_load.txt"))
    ap.add_argument("--child", choices=["keygen", "read"])
    ap.add_argument("--file")
    ap.add_argument("--limit", type=int, default=240, help="seconds per child")
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "key.pk")
        for mode in ("keygen", "read"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--child", mode, "--file", path],
                               capture_output=True, text=True, timeout=args.limit)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit("the %s child ended with status %d: nothing more is started" % (mode, p.returncode))
            results.append(json.loads(line[0][7:]))
    kg, rd = results
    lines = ["key file against keygen from the mapping, --shape %s (k = %d, %d fixed + %d permutation columns), library %s" %
             (args.shape, kg["k"], kg["num_fixed"], kg["num_perm_columns"], kg["library"].get("src")),
             "one cold call per process (the first after amdzk_init and the SRS), host wall clock, seconds",
             "",
             "key file                          %d bytes (%.1f MB)" % (kg["blob_bytes"], kg["blob_bytes"] / 1e6),
             "process 1: circuit on the host    %.3f   (configure, fixed assignment, copy constraints; Python)" % kg["circuit_host_s"],
             "process 1: keygen from mapping    %.3f   (ProvingKey(...), cold)" % kg["keygen_from_mapping_s"],
             "process 1: pk.write()             %.3f" % kg["write_s"],
             "process 2: file from disk         %.3f   (page cache warm: just written)" % rd["file_from_disk_s"],
             "process 2: blob_info              %.3f   (host only: BLAKE2b over the file)" % rd["blob_info_s"],
             "process 2: amdzk_pk_read          %.3f   (cold; parse + digest + keygen's tail + commitment check)" % rd["amdzk_pk_read_s"],
             "process 2: ProvingKey.read again  %.3f   (warm, with the Python mirror's desc rebuilt from the header)" % rd["ProvingKey_read_second_s"],
             "SRS setup (both)                  %.3f / %.3f" % (kg["srs_setup_s"], rd["srs_setup_s"]),
             "",
             json.dumps(results)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
