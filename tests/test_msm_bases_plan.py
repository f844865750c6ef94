"""CPU: the table-free MSM (amdzk_msm_g1_bases*, best_multiexp over caller-supplied bases) as far as it can be held
without a device: the plan every call follows (window bits, windows, workspace bytes — host code), the refusals, and the
register / scratch / multiply-add figures of the level-1 kernel the new driver shares with the prover."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anon-aadhaar-halo2_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

E_INVALID, E_UNSUPPORTED = -2, -5
LENS = [0, 1, 2, 3, 1000] + [1 << k for k in range(10, 27)]
NCOLS = [1, 7, 141]


def plan(pkg, ncols, length):
    c, w, b = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    rc = pkg.lib().amdzk_msm_g1_bases_plan(ncols, length, C.byref(c), C.byref(w), C.byref(b))
    return rc, c.value, w.value, b.value


def test_plan_needs_no_device_and_is_well_formed(pkg):
    for ncols in NCOLS:
        for n in LENS:
            rc, c, w, b = plan(pkg, ncols, n)
            assert rc == 0, (ncols, n)
            assert 8 <= c <= 16, (ncols, n, c)
            assert w == -(-255 // c), (ncols, n, c, w)
            assert b >= 64 * n, "the workspace holds a copy of the bases"
            assert plan(pkg, ncols, n) == (rc, c, w, b), "the same answer on a second call"
            d = pkg.arithmetic.multiexp_bases_plan(ncols, n)
            assert (d["window_bits"], d["windows"], d["scratch_bytes"]) == (c, w, b)


def test_plan_workspace_grows_with_the_shape(pkg):
    for ncols in NCOLS:
        sizes = [plan(pkg, ncols, n)[3] for n in LENS]
        assert sizes == sorted(sizes), "scratch_bytes must not decrease in len (ncols = %d): %r" % (ncols, sizes)
    for n in LENS:
        sizes = [plan(pkg, ncols, n)[3] for ncols in NCOLS]
        assert sizes == sorted(sizes), "scratch_bytes must not decrease in ncols (len = %d): %r" % (n, sizes)


def test_plan_window_bits_do_not_depend_on_the_batch(pkg):
    """The width is a property of the length: a column commits to the same windows alone and in a batch."""
    for n in LENS:
        assert len({plan(pkg, ncols, n)[1] for ncols in NCOLS}) == 1


def test_plan_refuses_what_the_calls_refuse(pkg):
    assert plan(pkg, 0, 1024)[0] == E_INVALID
    assert plan(pkg, 1, 1 << 31)[0] in (E_INVALID, E_UNSUPPORTED)
    for n in (0, 1024, 1 << 20):
        w = plan(pkg, 1, n)[2]
        assert plan(pkg, 65535 // w, n)[0] == 0
        assert plan(pkg, 65535 // w + 1, n)[0] in (E_INVALID, E_UNSUPPORTED), "ncols * windows > 65535 (grid.y)"
    with pytest.raises(pkg.AmdzkError):
        pkg.arithmetic.multiexp_bases_plan(0, 5)
    # null output pointers are allowed: only the status is wanted
    assert pkg.lib().amdzk_msm_g1_bases_plan(3, 77, None, None, None) == 0


def test_null_context_is_refused_without_a_crash(pkg):
    L = pkg.lib()
    buf = (C.c_uint64 * 64)()
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    assert L.amdzk_msm_g1_bases(None, buf, buf, 1, buf) == E_INVALID
    assert L.amdzk_msm_g1_bases_batch(None, ptrs, 1, buf, 1, buf) == E_INVALID
    assert L.amdzk_msm_g1_bases_dev(None, buf, 1, 1, 1, buf, buf) == E_INVALID


def test_python_layer_has_the_four_entry_points(pkg):
    for name in ("best_multiexp_bases", "best_multiexp_bases_batch", "best_multiexp_bases_dev", "multiexp_bases_plan"):
        assert callable(getattr(pkg.arithmetic, name))
    assert pkg.lib().amdzk_version() >= 1002


# ---- code generation: the table-free driver runs the prover's level-1 kernel as it is. These are the figures of
# msm_accum_seg_kernel<true> (hipcc -O3, gfx950, the library's flags) on the commit before this feature; a change means the
# hot kernel of every commitment was touched: measure the benchmark before accepting new numbers.
L1_KERNEL = "msm_accum_seg_kernelILb1E"
L1_VGPRS, L1_MADS = 152, 2542  # parent commit: 152 VGPRs, 0 bytes of scratch, 0 spills, 2,542 v_mad_u64_u32


def _kernels(asm):
    """mangled name -> (vgprs, scratch bytes, spills, v_mad_u64_u32 in the body) for every kernel of the file."""
    out = {}
    for ent in re.split(r"\n  - \.", asm[asm.index("amdhsa.kernels:"):]):
        nm = re.search(r"\.name:\s+(\S+)", ent)
        if not nm:
            continue
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(nm.group(1)), asm, re.S | re.M)
        assert body, nm.group(1)
        key = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, ent).group(1))
        out[nm.group(1)] = (key("vgpr_count"), key("private_segment_fixed_size"), key("vgpr_spill_count"),
                            sum(1 for ln in body.group(1).splitlines() if ln.strip().startswith("v_mad_u64_u32")))
    return out


@pytest.fixture(scope="module")
def msm_asm(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc is needed: the library itself is built with it"
    out = str(tmp_path_factory.mktemp("msm_asm") / "msm.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-DAMDZK_ASM_PRODUCT", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    "--cuda-device-only", "-S", os.path.join(CSRC, "msm.hip"), "-o", out], check=True, timeout=1200,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def test_level1_kernel_is_the_prover_s_unchanged(msm_asm):
    (vgprs, scratch, spills, mads), = [v for k, v in _kernels(msm_asm).items() if L1_KERNEL in k]
    print("msm_accum_seg_kernel<true>: %d VGPRs, %d bytes scratch, %d spills, %d v_mad_u64_u32" % (vgprs, scratch, spills, mads))
    assert (scratch, spills) == (0, 0)
    assert (vgprs, mads) == (L1_VGPRS, L1_MADS)


def test_new_kernels_use_no_scratch(msm_asm):
    new = {k: v for k, v in _kernels(msm_asm).items() if "msm_digit_win_kernel" in k or "msm_window_combine_kernel" in k}
    assert len(new) == 2 * 9 + 1, "histogram and scatter for the widths 8..16, and the window combine"
    for name, (_, scratch, spills, _) in new.items():
        assert (scratch, spills) == (0, 0), name
