"""CPU: the ABI of amdzk_create_proof_batch — the header, the library, the ctypes binding and the C++ mirror agree.
No device is needed: nothing here computes."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
NEW = ("amdzk_create_proof_batch", "amdzk_msm_g1_cols_dev")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "amdzk.h")).read(), flags=re.S)


def test_header_library_and_binding_have_the_new_symbols(pkg):
    text = header_text()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in include/amdzk.h" % name
        assert hasattr(L, name), "libamdzk.so does not export %s" % name
        assert name in L._amdzk_sig
    assert len(L._amdzk_sig["amdzk_create_proof_batch"][1]) == 12
    assert L.amdzk_version() >= 1004
    assert "typedef struct amdzk_batch_opts" in text


def test_integration_md_block_has_the_new_entries():
    """The generated FFI block (tests/test_capi_symbols.py checks it against the generator) spells the new struct and calls."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as g

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index(g.BEGIN):doc.index(g.END)]
    assert "pub struct AmdzkBatchOpts {" in block and "pub scalars: *const *const u64," in block
    assert "pub fn amdzk_create_proof_batch(ctx: *mut Ctx, pks: *const *mut Pk, n_proofs: usize," in block
    assert "opts: *const AmdzkBatchOpts" in block and "statuses: *mut c_int) -> c_int;" in block
    assert "pub fn amdzk_msm_g1_cols_dev(ctx: *mut Ctx, srs: *const Srs, basis: c_int, d_cols: *const *const c_void," in block


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "amdzk.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
  printf("amdzk_batch_opts %zu\n", sizeof(amdzk_batch_opts));
  F(amdzk_batch_opts, size); F(amdzk_batch_opts, transcript_kind); F(amdzk_batch_opts, rng_seeds); F(amdzk_batch_opts, scalars);
  F(amdzk_batch_opts, scalar_count);
  printf("amdzk_proof_opts %zu\n", sizeof(amdzk_proof_opts));
  return 0;
}
"""


def test_ctypes_struct_matches_a_compiled_probe(pkg, tmp_path):
    """sizeof and every field's offset and size of amdzk_batch_opts as a C compiler lays it out = ffi.BatchOpts (and the
    size of amdzk_proof_opts = ffi.ProofOpts, the struct beside it)."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    out = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    ffi = pkg.ffi
    assert int(out["amdzk_batch_opts"]) == C.sizeof(ffi.BatchOpts)
    assert int(out["amdzk_proof_opts"]) == C.sizeof(ffi.ProofOpts)
    names = [f[0] for f in ffi.BatchOpts._fields_]
    assert names == ["size", "transcript_kind", "rng_seeds", "scalars", "scalar_count"]
    for f in names:
        off, size = (int(v) for v in out["amdzk_batch_opts." + f].split())
        d = getattr(ffi.BatchOpts, f)
        assert (d.offset, d.size) == (off, size), f


MIRROR = r"""
#include "amdzk_halo2.hpp"
using namespace amdzk::halo2;
// instantiated, never run: this test has no device
std::vector<BatchProof> prove_all(const Context& ctx, const ProvingKey& pk, const ProvingKey& clone, const void* w0, const void* w1, size_t n) {
  std::vector<std::vector<std::vector<Fr>>> inst(2);
  return create_proof_batch(ctx, {&pk, &clone}, inst, {w0, w1}, n, {1, 2}, Transcript::Keccak256Evm, Multiopen::Gwc);
}
int main(int argc, char**) {
  auto fn = &prove_all;
  std::vector<BatchProof> none;
  return argc > 100 ? (int)(size_t)fn : (int)none.size();
}
"""


def test_cpp_mirror_compiles_with_create_proof_batch(tmp_path):
    """include/amdzk_halo2.hpp with a caller of create_proof_batch builds the way tests/test_cpp_mirror.py builds the
    mirror's checker (g++ -std=c++17 -Wall -Werror against libamdzk.so) and the program loads and runs."""
    src, exe = tmp_path / "mirror.cpp", tmp_path / "mirror"
    src.write_text(MIRROR)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src), "-L", LIBDIR, "-lamdzk",
                           "-Wl,-rpath," + LIBDIR])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_python_mirror_signature(pkg):
    import inspect
    sig = inspect.signature(pkg.plonk.create_proof_batch)
    assert list(sig.parameters)[:5] == ["ctx", "pks", "instances_list", "d_advice_list", "seeds"]
    assert sig.parameters["scalars"].default is None and sig.parameters["transcript"].default == pkg.plonk.TRANSCRIPT_BLAKE2B
