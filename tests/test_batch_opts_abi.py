"""CPU: the ABI of amdzk_create_proof_batch_opts — the header, the library, the ctypes binding and the C++ mirror agree.
No device is needed: nothing here computes."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
FIELDS = ["size", "transcript_kind", "rng_seeds", "scalars", "scalar_count", "transcripts", "phase_fn", "phase_user"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "amdzk.h")).read(), flags=re.S)


def test_header_library_and_binding_have_the_new_symbol(pkg):
    text = header_text()
    L = pkg.lib()
    name = "amdzk_create_proof_batch_opts"
    assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared in include/amdzk.h" % name
    assert hasattr(L, name), "libamdzk.so does not export %s" % name
    assert len(L._amdzk_sig[name][1]) == 12
    assert L._amdzk_sig[name] == L._amdzk_sig["amdzk_create_proof_batch"]  # the same arguments, another options struct
    assert L.amdzk_version() >= 1015 and pkg.ffi.build_info()["abi"] == L.amdzk_version()
    assert "typedef struct amdzk_batch_proof_opts" in text and "(*amdzk_batch_phase_fn)(" in text
    # the callback: user, phase, n_proofs, wanted, challenges, challenge_stride, proof_rc, hip_stream -> int
    assert len(pkg.ffi.BATCH_PHASE_FN._argtypes_) == 8 and pkg.ffi.BATCH_PHASE_FN._restype_ is C.c_int


def test_integration_md_block_has_the_new_entries():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_rust_ffi as g

    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index(g.BEGIN):doc.index(g.END)]
    assert "pub struct AmdzkBatchProofOpts {" in block and "pub transcripts: *const *const AmdzkTranscript," in block
    assert "pub fn amdzk_create_proof_batch_opts(ctx: *mut Ctx, pks: *const *mut Pk, n_proofs: usize," in block
    assert "opts: *const AmdzkBatchProofOpts" in block


PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "amdzk.h"
#define F(T, f) printf(#T "." #f " %zu %zu\n", offsetof(T, f), sizeof(((T*)0)->f))
int main(void) {
  printf("amdzk_batch_proof_opts %zu\n", sizeof(amdzk_batch_proof_opts));
  F(amdzk_batch_proof_opts, size); F(amdzk_batch_proof_opts, transcript_kind); F(amdzk_batch_proof_opts, rng_seeds);
  F(amdzk_batch_proof_opts, scalars); F(amdzk_batch_proof_opts, scalar_count); F(amdzk_batch_proof_opts, transcripts);
  F(amdzk_batch_proof_opts, phase_fn); F(amdzk_batch_proof_opts, phase_user);
  printf("amdzk_batch_opts %zu\n", sizeof(amdzk_batch_opts));
  return 0;
}
"""


def test_ctypes_struct_matches_a_compiled_probe(pkg, tmp_path):
    """sizeof and every field's offset and size of amdzk_batch_proof_opts as a C compiler lays it out = ffi.BatchProofOpts;
    amdzk_batch_opts beside it is unchanged."""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    out = dict(ln.split(" ", 1) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    ffi = pkg.ffi
    assert int(out["amdzk_batch_proof_opts"]) == C.sizeof(ffi.BatchProofOpts)
    assert int(out["amdzk_batch_opts"]) == C.sizeof(ffi.BatchOpts)
    assert [f[0] for f in ffi.BatchProofOpts._fields_] == FIELDS
    for f in FIELDS:
        off, size = (int(v) for v in out["amdzk_batch_proof_opts." + f].split())
        d = getattr(ffi.BatchProofOpts, f)
        assert (d.offset, d.size) == (off, size), f


MIRROR = r"""
#include <cstdio>
#include <cstring>
#include "amdzk_halo2.hpp"
using namespace amdzk::halo2;
struct Quiet : TranscriptWrite {
  void common_point(const G1Affine&) override {}
  void common_scalar(const Fr&) override {}
  void write_point(const G1Affine&) override {}
  void write_scalar(const Fr&) override {}
  Fr squeeze_challenge() override { return Fr(); }
};
// instantiated, never run: this test has no device
std::vector<BatchProof> prove_all(const Context& ctx, const ProvingKey& big, const ProvingKey& small, const void* w0, const void* w1, size_t n) {
  std::vector<std::vector<std::vector<Fr>>> inst(2);
  Quiet mine;
  BatchSynthesize syn = [](uint32_t, const std::vector<uint8_t>& wanted, const std::vector<std::vector<Fr>>& challenges, void*) {
    return std::vector<int>(wanted.size() + challenges.size(), 0);
  };
  return create_proof_batch(ctx, {&big, &small}, inst, {w0, w1}, n, {1, 2}, {nullptr, &mine}, syn, Transcript::Keccak256Evm, Multiopen::Gwc);
}
int main(int argc, char**) {
  auto fn = &prove_all;
  if (argc > 100) return (int)(size_t)fn;
  // without a device there is no ctx: the entry point refuses, and says so for every proof
  amdzk_batch_proof_opts opts;
  std::memset(&opts, 0, sizeof(opts));
  opts.size = sizeof(opts);
  size_t lens[2] = {7, 7};
  int st[2] = {1, 1};
  const int rc = amdzk_create_proof_batch_opts(nullptr, nullptr, 2, nullptr, nullptr, nullptr, 0, &opts, nullptr, 0, lens, st);
  std::printf("%d\n", rc);
  return rc == AMDZK_E_INVALID ? 0 : 1;
}
"""


def test_cpp_mirror_compiles_and_refuses_without_a_device(tmp_path):
    """include/amdzk_halo2.hpp with a caller of the create_proof_batch overload (per-proof transcripts, a batch synthesize
    functor) builds with g++ -std=c++17 -Wall -Werror against libamdzk.so; the program loads, and the C entry point refuses
    a call without a ctx."""
    src, exe = tmp_path / "mirror.cpp", tmp_path / "mirror"
    src.write_text(MIRROR)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src), "-L", LIBDIR, "-lamdzk",
                           "-Wl,-rpath," + LIBDIR])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_python_mirror_signature(pkg):
    sig = inspect.signature(pkg.plonk.create_proof_batch_opts)
    assert list(sig.parameters) == ["ctx", "pks", "instances_list", "d_advice_list", "seeds", "scalars", "transcript", "synthesize",
                                    "transcript_objects", "advice_stride", "opts_size", "proof_stride"]
    assert sig.parameters["seeds"].default is None and sig.parameters["transcript"].default == pkg.plonk.TRANSCRIPT_BLAKE2B
