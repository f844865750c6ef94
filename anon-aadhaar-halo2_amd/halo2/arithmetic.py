"""Mirror of halo2_proofs::arithmetic (v2023_01_20 [UP]) for the functions on the hot path.

Field elements are numpy uint64 arrays of shape (n, 4): halo2curves' in-memory Montgomery limbs.
"""
import ctypes as C

import numpy as np

from ..ffi import _ptr, as_fr_array

NTT_SCALE_NINV = 1


def best_fft(ctx, a, omega, log_n, flags=0):
    """arithmetic::best_fft(a, omega, log_n): in-place NTT of one host column (returns the array)."""
    a = as_fr_array(a)
    assert a.shape[0] == 1 << log_n, "best_fft: a.len() != 1 << log_n"
    omega = np.ascontiguousarray(omega, dtype=np.uint64).reshape(4)
    ctx._chk(ctx.L.amdzk_ntt_fr(ctx.h, _ptr(a), log_n, _ptr(omega), flags))
    return a


def best_fft_dev(ctx, dbuf, omega, log_n, ncols=1, col_stride=None, flags=0):
    """Same on `ncols` device-resident columns."""
    omega = np.ascontiguousarray(omega, dtype=np.uint64).reshape(4)
    if col_stride is None:
        col_stride = 1 << log_n
    ctx._chk(ctx.L.amdzk_ntt_fr_dev(ctx.h, dbuf.ptr, log_n, _ptr(omega), flags, ncols, col_stride))


def best_fft_batch(ctx, columns, omega, log_n, flags=0):
    """Several host columns of 1 << log_n in one submission (amdzk_ntt_fr_batch), each transformed in place; returns them."""
    cols = [as_fr_array(c) for c in columns]
    assert all(c.shape[0] == 1 << log_n for c in cols), "best_fft_batch: a.len() != 1 << log_n"
    omega = np.ascontiguousarray(omega, dtype=np.uint64).reshape(4)
    ptrs = (C.c_void_p * max(1, len(cols)))(*[c.ctypes.data for c in cols])
    ctx._chk(ctx.L.amdzk_ntt_fr_batch(ctx.h, ptrs, len(cols), log_n, _ptr(omega), flags))
    return cols


def fr_from_raw_dev(ctx, dbuf, n):
    """Fr::from_raw on n resident elements in place (amdzk_fr_from_raw_dev): canonical 4 x u64 below r -> Montgomery."""
    ctx._chk(ctx.L.amdzk_fr_from_raw_dev(ctx.h, dbuf.ptr if dbuf is not None else None, n))


def fr_to_repr_dev(ctx, dbuf, n):
    """Fr::to_repr on n resident elements in place (amdzk_fr_to_repr_dev): Montgomery -> canonical 4 x u64."""
    ctx._chk(ctx.L.amdzk_fr_to_repr_dev(ctx.h, dbuf.ptr if dbuf is not None else None, n))


def best_multiexp(ctx, srs, basis, coeffs):
    """arithmetic::best_multiexp(coeffs, bases) with bases = srs.{g|g_lagrange}[..len].
    Returns the normalised Jacobian point as (12,) uint64 (x, y, z=1 | identity (0,1,0))."""
    coeffs = as_fr_array(coeffs)
    out = np.zeros(12, dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1(ctx.h, srs, basis, _ptr(coeffs), coeffs.shape[0], _ptr(out)))
    return out


def best_multiexp_batch(ctx, srs, basis, columns):
    cols = [as_fr_array(c) for c in columns]
    n = cols[0].shape[0]
    assert all(c.shape[0] == n for c in cols)
    ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    out = np.zeros((len(cols), 12), dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_batch(ctx.h, srs, basis, ptrs, len(cols), n, _ptr(out)))
    return out


def best_multiexp_dev(ctx, srs, basis, dbuf, ncols, length, col_stride=None):
    if col_stride is None:
        col_stride = length
    out = np.zeros((ncols, 12), dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_dev(ctx.h, srs, basis, dbuf.ptr, ncols, length, col_stride, _ptr(out)))
    return out


def best_multiexp_cols_dev(ctx, srs, basis, col_ptrs, length, max_scratch_bytes=0):
    """amdzk_msm_g1_cols_dev: one MSM per column over srs.{g|g_lagrange}[..length], column c read from the device address
    col_ptrs[c] (ints) — columns in different buffers, one submission, no copy. max_scratch_bytes > 0 bounds one
    submission's workspace (the columns are then cut into runs). Returns (ncols, 12) uint64 normalised Jacobian points."""
    tab = (C.c_void_p * len(col_ptrs))(*[int(p) for p in col_ptrs])
    out = np.zeros((len(col_ptrs), 12), np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_cols_dev(ctx.h, srs, basis, tab, len(col_ptrs), length, max_scratch_bytes, _ptr(out)))
    return out


def as_g1_array(bases):
    """(n, 8) uint64 C-contiguous: n G1Affine, x then y, Montgomery limbs; (0, 0) is the identity."""
    b = np.ascontiguousarray(bases, dtype=np.uint64)
    if b.ndim == 1:
        b = b.reshape(-1, 8)
    assert b.shape[-1] == 8
    return b


def best_multiexp_bases(ctx, coeffs, bases):
    """arithmetic::best_multiexp(coeffs, bases) over the caller's own points: no ParamsKZG, no window table, any length.
    Returns the normalised Jacobian point as (12,) uint64."""
    coeffs, bases = as_fr_array(coeffs), as_g1_array(bases)
    assert coeffs.shape[0] == bases.shape[0], "best_multiexp: coeffs.len() != bases.len()"
    out = np.zeros(12, dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_bases(ctx.h, _ptr(coeffs), _ptr(bases), coeffs.shape[0], _ptr(out)))
    return out


def best_multiexp_bases_batch(ctx, columns, bases):
    """Several scalar columns over the same caller-supplied bases in one submission: (ncols, 12) uint64."""
    cols = [as_fr_array(c) for c in columns]
    bases = as_g1_array(bases)
    n = bases.shape[0]
    assert all(c.shape[0] == n for c in cols)
    ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    out = np.zeros((len(cols), 12), dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_bases_batch(ctx.h, ptrs, len(cols), _ptr(bases), n, _ptr(out)))
    return out


def best_multiexp_bases_dev(ctx, dbuf, d_bases, ncols, length, col_stride=None):
    """The same on resident data: `dbuf` holds the scalar columns (column c at c * col_stride elements), `d_bases` the
    `length` points (read only)."""
    if col_stride is None:
        col_stride = length
    out = np.zeros((ncols, 12), dtype=np.uint64)
    ctx._chk(ctx.L.amdzk_msm_g1_bases_dev(ctx.h, dbuf.ptr, ncols, length, col_stride, d_bases.ptr, _ptr(out)))
    return out


def multiexp_bases_plan(ncols, length):
    """amdzk_msm_g1_bases_plan: what best_multiexp_bases* does for this shape, as {"window_bits", "windows", "scratch_bytes"}.
    Needs no device and no Context; a refused shape raises AmdzkError with the call's status."""
    from ..ffi import AmdzkError, lib
    c, w, b = C.c_uint32(), C.c_uint32(), C.c_size_t()
    rc = lib().amdzk_msm_g1_bases_plan(ncols, length, C.byref(c), C.byref(w), C.byref(b))
    if rc != 0:
        raise AmdzkError(rc, "msm_bases_plan: shape (ncols = %d, len = %d) is refused" % (ncols, length))
    return {"window_bits": c.value, "windows": w.value, "scratch_bytes": b.value}


def g_to_lagrange(ctx, g, k):
    """arithmetic::g_to_lagrange(g_projective, k): (n, 8) uint64 affine points in the monomial basis ->
    the Lagrange-basis points (1/n)·FFT_{omega^-1}(g), affine."""
    g = np.ascontiguousarray(g, dtype=np.uint64)
    assert g.shape == (1 << k, 8)
    out = np.zeros_like(g)
    ctx._chk(ctx.L.amdzk_g_to_lagrange(ctx.h, _ptr(g), k, _ptr(out)))
    return out


# ---- the PLONK layer's helpers, function by function (include/amdzk.h "function by function"); host arrays in,
# host arrays out: each call uploads, runs the device kernel create_proof itself uses, and downloads.
def _dev_cols(ctx, cols):
    cols = [as_fr_array(c) for c in cols]
    n = cols[0].shape[0]
    assert all(c.shape[0] == n for c in cols)
    buf = ctx.alloc(max(1, len(cols) * n * 32))
    buf.upload(np.ascontiguousarray(np.stack(cols)) if n else np.zeros((0, 4), np.uint64))
    return buf, n


def batch_invert(ctx, a):
    """ff::BatchInvert: inverses of the non-zero elements, zeros stay zero."""
    a = as_fr_array(a)
    buf = ctx.alloc(max(1, a.nbytes)).upload(a)
    ctx._chk(ctx.L.amdzk_batch_invert_dev(ctx.h, buf.ptr, a.shape[0]))
    out = buf.download(a.shape)
    buf.free()
    return out


def batch_invert_assigned(ctx, numerators, denominators=None, in_place=False):
    """poly::batch_invert_assigned: Assigned::Rational(num, den) cells -> num * den^-1 (zero where den = 0); denominators=None:
    every cell Trivial."""
    num = as_fr_array(numerators)
    n = num.shape[0]
    d_num = ctx.alloc(max(1, num.nbytes)).upload(num)
    d_den = None
    if denominators is not None:
        den = as_fr_array(denominators)
        assert den.shape[0] == n
        d_den = ctx.alloc(max(1, den.nbytes)).upload(den)
    d_out = d_num if in_place else ctx.alloc(max(1, num.nbytes))
    ctx._chk(ctx.L.amdzk_batch_invert_assigned_dev(ctx.h, d_num.ptr, d_den.ptr if d_den is not None else None, n, d_out.ptr))
    out = d_out.download(num.shape)
    if not in_place:
        assert np.array_equal(d_num.download(num.shape), num)  # the numerators are read, not written
        d_out.free()
    d_num.free()
    if d_den is not None:
        d_den.free()
    return out


def grand_product(ctx, cols, chain=False, chain_row=0):
    """Running products z[0] = 1, z[i] = z[i-1] * f[i-1] of every column (permutation / lookup commit_product);
    chain: z_c[0] = z_{c-1}[chain_row]."""
    buf, n = _dev_cols(ctx, cols)
    ctx._chk(ctx.L.amdzk_grand_product_dev(ctx.h, buf.ptr, len(cols), n, n, 1 if chain else 0, chain_row))
    out = buf.download((len(cols), n, 4))
    buf.free()
    return out


def eval_polynomial(ctx, polys, points):
    """arithmetic::eval_polynomial(poly, point) for a list of (poly, point) pairs."""
    buf, n = _dev_cols(ctx, polys)
    pts = as_fr_array(points)
    assert pts.shape[0] == len(polys)
    ptrs = (C.c_void_p * len(polys))(*[buf.ptr.value + i * n * 32 for i in range(len(polys))])
    out = np.zeros((len(polys), 4), np.uint64)
    ctx._chk(ctx.L.amdzk_eval_poly_dev(ctx.h, ptrs, _ptr(pts), len(polys), n, _ptr(out)))
    buf.free()
    return out


def poly_axpy(ctx, polys, coefs):
    """sum_j coefs[j] * polys[j]."""
    buf, n = _dev_cols(ctx, polys)
    cf = as_fr_array(coefs)
    ptrs = (C.c_void_p * len(polys))(*[buf.ptr.value + i * n * 32 for i in range(len(polys))])
    out = ctx.alloc(max(1, n * 32))
    ctx._chk(ctx.L.amdzk_poly_axpy_dev(ctx.h, ptrs, _ptr(cf), len(polys), out.ptr, n, 0))
    res = out.download((n, 4))
    buf.free()
    out.free()
    return res


def kate_division(ctx, polys, roots):
    """arithmetic::kate_division(a, root) for each pair: (a(X) - a(root)) / (X - root), n - 1 coefficients."""
    buf, n = _dev_cols(ctx, polys)
    rt = as_fr_array(roots)
    ptrs = (C.c_void_p * len(polys))(*[buf.ptr.value + i * n * 32 for i in range(len(polys))])
    ctx._chk(ctx.L.amdzk_kate_div_dev(ctx.h, ptrs, _ptr(rt), len(polys), n))
    out = buf.download((len(polys), n, 4))
    buf.free()
    assert not out[:, n - 1].any(), "kate_division: top coefficient must be zero"
    return out[:, : n - 1]


def permute_expression_pair(ctx, inputs, tables, usable):
    """lookup::prover::permute_expression_pair for a list of (input, table) column pairs of n rows: returns
    (A', S') as (L, n, 4) arrays, rows >= usable zero (the caller blinds them)."""
    a_buf, n = _dev_cols(ctx, inputs)
    t_buf, n2 = _dev_cols(ctx, tables)
    assert n == n2 and len(inputs) == len(tables)
    s_buf = ctx.alloc(len(inputs) * n * 32)
    try:
        ctx._chk(ctx.L.amdzk_permute_expression_pair_dev(ctx.h, a_buf.ptr, t_buf.ptr, s_buf.ptr, len(inputs), n, usable))
        return a_buf.download((len(inputs), n, 4)), s_buf.download((len(inputs), n, 4))
    finally:
        a_buf.free(); t_buf.free(); s_buf.free()
