"""CPU: the ABI of amdzk_check_witness — the header, the library, the ctypes binding and the Python signature agree.
No device is needed: nothing here computes."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "amdzk.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
  printf("amdzk_check_failure %zu\n", sizeof(amdzk_check_failure));
  F(amdzk_check_failure, kind); F(amdzk_check_failure, index); F(amdzk_check_failure, first_row); F(amdzk_check_failure, reserved);
  F(amdzk_check_failure, count);
  printf("amdzk_check_opts %zu\n", sizeof(amdzk_check_opts));
  F(amdzk_check_opts, size); F(amdzk_check_opts, theta_seed); F(amdzk_check_opts, challenges); F(amdzk_check_opts, num_challenges);
  printf("kinds %d %d %d\n", AMDZK_CHECK_GATE, AMDZK_CHECK_LOOKUP, AMDZK_CHECK_COPY);
  return 0;
}
"""


def test_header_library_and_binding_have_the_symbol(pkg):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "amdzk.h")).read(), flags=re.S)
    L = pkg.lib()
    assert re.search(r"\bamdzk_check_witness\s*\(", text), "amdzk_check_witness is not declared in include/amdzk.h"
    assert hasattr(L, "amdzk_check_witness"), "libamdzk.so does not export amdzk_check_witness"
    assert len(L._amdzk_sig["amdzk_check_witness"][1]) == 10
    assert L.amdzk_version() >= 1007
    assert "typedef struct amdzk_check_failure" in text and "typedef struct amdzk_check_opts" in text


def test_ctypes_structs_match_a_compiled_probe(pkg, tmp_path):
    """sizeof and every field's offset and size of amdzk_check_failure and amdzk_check_opts as a C compiler lays them out
    = ffi.CheckFailure and ffi.CheckOpts; the kind constants = plonk.CHECK_*."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    out = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    ffi = pkg.ffi
    for cname, ct, names in (("amdzk_check_failure", ffi.CheckFailure, ["kind", "index", "first_row", "reserved", "count"]),
                             ("amdzk_check_opts", ffi.CheckOpts, ["size", "theta_seed", "challenges", "num_challenges"])):
        assert int(out[cname]) == C.sizeof(ct), cname
        assert [f[0] for f in ct._fields_] == names
        for f in names:
            off, size = (int(v) for v in out["%s.%s" % (cname, f)].split())
            d = getattr(ct, f)
            assert (d.offset, d.size) == (off, size), (cname, f)
    assert C.sizeof(ffi.CheckFailure) == 24
    plonk = pkg.plonk
    assert [int(v) for v in out["kinds"].split()] == [plonk.CHECK_GATE, plonk.CHECK_LOOKUP, plonk.CHECK_COPY] == [0, 1, 2]


def test_python_signature_defaults(pkg):
    sig = inspect.signature(pkg.plonk.check_witness)
    assert list(sig.parameters)[:7] == ["ctx", "pk", "instances", "d_advice", "theta_seed", "challenges", "advice_stride"]
    assert sig.parameters["theta_seed"].default == 0
    assert sig.parameters["challenges"].default is None and sig.parameters["advice_stride"].default is None
    rep = pkg.plonk.WitnessReport([])
    assert rep.ok and rep.failures == []
    bad = pkg.plonk.WitnessReport([pkg.plonk.CheckFailure(0, 1, 2, 3)])
    assert not bad.ok and bad.failures[0].first_row == 2 and bad.failures[0]._fields == ("kind", "index", "first_row", "count")
