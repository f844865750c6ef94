"""Mirror of halo2_proofs::poly::kzg::commitment::ParamsKZG (v2023_01_20 [UP]) — the resident part."""
import ctypes as C
import secrets

import numpy as np

from .. import ffi as _ffi
from ..ffi import _ptr
from . import arithmetic

BASIS_G = 0
BASIS_G_LAGRANGE = 1
BASIS_G_LAGRANGE_PREFIX = 2  # prefix sums of g_lagrange: resident once a key with permutation columns exists (MSM only)


class ParamsKZG:
    """Holds {k, n, g, g_lagrange} on the device. `g`/`g_lagrange`: (n, 8) uint64 affine points."""

    def __init__(self, ctx, k, g=None, g_lagrange=None):
        self.ctx, self.k, self.n = ctx, k, 1 << k
        for a in (g, g_lagrange):
            if a is not None:
                assert a.shape == (self.n, 8) and a.dtype == np.uint64
        self._g = None if g is None else np.ascontiguousarray(g)
        self._gl = None if g_lagrange is None else np.ascontiguousarray(g_lagrange)
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_srs_upload(ctx.h, None if g is None else _ptr(self._g),
                                        None if g_lagrange is None else _ptr(self._gl), k, C.byref(h)))
        self.h = h

    @classmethod
    def setup(cls, ctx, k, s, want_host_copy=False):
        """ParamsKZG::setup(k, rng) with the trapdoor `s` ((4,) uint64 Montgomery Fr) given explicitly
        (test / benchmark SRS, as unsafe as upstream's setup). Bases are generated on the device."""
        self = cls.__new__(cls)
        self.ctx, self.k, self.n = ctx, k, 1 << k
        s = np.ascontiguousarray(s, dtype=np.uint64).reshape(4)
        self._g = np.zeros((self.n, 8), np.uint64) if want_host_copy else None
        self._gl = np.zeros((self.n, 8), np.uint64) if want_host_copy else None
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_srs_setup(ctx.h, k, _ptr(s), C.byref(h), None if self._g is None else _ptr(self._g),
                                       None if self._gl is None else _ptr(self._gl)))
        self.h = h
        return self

    def write(self, g2=bytes(64), s_g2=bytes(64)):
        """ParamsKZG::write: serialized parameters as bytes (g2 / s_g2 are passed through)."""
        size = self.ctx.L.amdzk_srs_serialized_size(self.k)
        buf = (C.c_uint8 * size)()
        a, b = (C.c_uint8 * 64)(*g2), (C.c_uint8 * 64)(*s_g2)
        self.ctx._chk(self.ctx.L.amdzk_srs_write(self.ctx.h, self.h, a, b, buf, size))
        return bytes(buf)

    @classmethod
    def read(cls, ctx, data):
        """ParamsKZG::read: returns (params, g2 bytes, s_g2 bytes)."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self.k = int.from_bytes(data[:4], "little")
        self.n = 1 << self.k
        self._g = self._gl = None
        h = C.c_void_p()
        g2, s_g2 = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
        raw = (C.c_uint8 * len(data)).from_buffer_copy(data)
        ctx._chk(ctx.L.amdzk_srs_read(ctx.h, raw, len(data), C.byref(h), g2, s_g2))
        self.h = h
        return self, bytes(g2), bytes(s_g2)

    def check(self, g2, s_g2, seed=None, rho=None, checks=0):
        """amdzk_srs_check: is this SRS an SRS? g2, s_g2: (16,) uint64 points, e.g. g2_from_bytes of the file's fields.
        checks: SRS_CHECK_* bits, 0 = all. rho ((4,) uint64 Montgomery Fr, < r) wins over seed; seed=None draws 64 bits from
        the OS generator (`secrets`). Returns the report (ffi.SrsReport): consistent iff report.failed == 0 and report.ran
        covers what was asked; report.points holds A, B, C, E as four G1Affine."""
        g2 = np.ascontiguousarray(g2, dtype=np.uint64).reshape(16)
        s_g2 = np.ascontiguousarray(s_g2, dtype=np.uint64).reshape(16)
        r = None if rho is None else np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        opts = _ffi.SrsCheckOpts(C.sizeof(_ffi.SrsCheckOpts), checks, secrets.randbits(64) if seed is None else seed,
                                 None if r is None else r.ctypes.data)
        rep = _ffi.SrsReport()
        self.ctx._chk(self.ctx.L.amdzk_srs_check(self.ctx.h, self.h, _ptr(g2), _ptr(s_g2), C.byref(opts), C.byref(rep)))
        return rep

    def downsize(self, k):
        """ParamsKZG::downsize(k): shrink in place to 2^k — g truncated, g_lagrange recomputed on the
        device with g_to_lagrange."""
        h = C.c_void_p()
        self.ctx._chk(self.ctx.L.amdzk_srs_downsize(self.ctx.h, self.h, k, C.byref(h)))
        self.ctx.L.amdzk_srs_free(self.ctx.h, self.h)
        self.h, self.k, self.n = h, k, 1 << k
        self._g = None if self._g is None else np.ascontiguousarray(self._g[: self.n])
        self._gl = None if self._gl is None else self.get_g_lagrange()

    def get_g(self):
        """ParamsKZG::get_g(): (n, 8) uint64 affine points."""
        out = np.zeros((self.n, 8), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_srs_get(self.ctx.h, self.h, BASIS_G, _ptr(out)))
        return out

    def get_g_lagrange(self):
        out = np.zeros((self.n, 8), np.uint64)
        self.ctx._chk(self.ctx.L.amdzk_srs_get(self.ctx.h, self.h, BASIS_G_LAGRANGE, _ptr(out)))
        return out

    def commit(self, poly_coeff):
        """ParamsKZG::commit(poly, _blind): MSM with g[..len] (the blind is ignored for KZG)."""
        return arithmetic.best_multiexp(self.ctx, self.h, BASIS_G, poly_coeff)

    def commit_lagrange(self, poly_lagrange):
        """ParamsKZG::commit_lagrange(poly, _blind): MSM with g_lagrange[..len]."""
        return arithmetic.best_multiexp(self.ctx, self.h, BASIS_G_LAGRANGE, poly_lagrange)

    def free(self):
        if self.h:
            self.ctx.L.amdzk_srs_free(self.ctx.h, self.h)
            self.h = None


# ---- the G2 side and the pairing (include/amdzk.h "pairing"; conventions: csrc/fq12.cuh)
PAIRING_MAX_M = 16  # AMDZK_PAIRING_MAX_M
SRS_CHECK_G2, SRS_CHECK_CURVE, SRS_CHECK_POWERS, SRS_CHECK_LAGRANGE = 1, 2, 4, 8  # AMDZK_SRS_CHECK_*
SRS_CHECK_ALL = 15
# amdzk_g2_check's statuses
G2_IN_GROUP, G2_COORD_TOO_LARGE, G2_OFF_TWIST, G2_IDENTITY, G2_OUTSIDE_SUBGROUP = range(5)
_G2_STATUS = ("in G2", "a coordinate is not below the modulus", "not on the twist", "the identity", "on the twist, outside the order-r subgroup")


def _g2_codec(fn, arg):
    msg = C.create_string_buffer(256)
    rc = fn(arg, msg)
    if rc != 0:
        raise _ffi.AmdzkError(rc, msg.value.decode())


def g2_to_bytes(q):
    """G2Affine::to_bytes (halo2curves' G2Compressed, the g2 / s_g2 fields of the ParamsKZG file): (16,) uint64 -> 64 bytes.
    Host only, no Context. Refused: a coordinate >= q, a point off the twist. The identity is 64 zero bytes."""
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(16)
    out = (C.c_uint8 * 64)()
    _g2_codec(lambda a, msg: _ffi.lib().amdzk_g2_compress(a, out, msg, 256), _ptr(q))
    return bytes(out)


def g2_from_bytes(b):
    """G2Affine::from_bytes: 64 bytes -> (16,) uint64 (all zero = the identity). Host only. Refused: x >= q, x = 0 with the
    sign bit set, an x no point of the twist has. The point is on the twist; membership in G2 is g2_check's business."""
    if len(b) != 64:
        raise _ffi.AmdzkError(-2, "g2_decompress: %d bytes given, 64 needed" % len(b))
    raw = (C.c_uint8 * 64).from_buffer_copy(bytes(b))
    q = np.zeros(16, np.uint64)
    _g2_codec(lambda a, msg: _ffi.lib().amdzk_g2_decompress(a, _ptr(q), msg, 256), raw)
    return q


def g2_check(q):
    """amdzk_g2_check: G2_IN_GROUP (0), G2_COORD_TOO_LARGE, G2_OFF_TWIST, G2_IDENTITY or G2_OUTSIDE_SUBGROUP. Host only."""
    q = np.ascontiguousarray(q, dtype=np.uint64).reshape(16)
    st = C.c_int(-1)
    rc = _ffi.lib().amdzk_g2_check(_ptr(q), C.byref(st))
    if rc != 0:
        raise _ffi.AmdzkError(rc, "g2_check: null argument")
    return st.value


class G2Prepared:
    """halo2curves' G2Prepared: ONE finite G2 point ((16,) uint64: x.c0, x.c1, y.c0, y.c1, Montgomery) as the line
    coefficients of the Miller loop, resident on the ctx's device. Refused: a coordinate >= q, a point off the twist, the
    identity. Subgroup membership is not checked."""

    def __init__(self, ctx, q):
        self.ctx = ctx
        q = np.ascontiguousarray(q, dtype=np.uint64).reshape(16)
        h = C.c_void_p()
        ctx._chk(ctx.L.amdzk_g2_prepare(ctx.h, _ptr(q), C.byref(h)))
        self.h = h

    def free(self):
        if self.h:
            self.ctx.L.amdzk_g2_free(self.ctx.h, self.h)
            self.h = None


def g2_setup(ctx, s):
    """The G2 half of ParamsKZG::setup with the trapdoor `s` ((4,) uint64 Montgomery Fr; as unsafe as ParamsKZG.setup):
    (g2, s_g2), (16,) uint64 each."""
    s = np.ascontiguousarray(s, dtype=np.uint64).reshape(4)
    g2, s_g2 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
    ctx._chk(ctx.L.amdzk_g2_setup(ctx.h, _ptr(s), _ptr(g2), _ptr(s_g2)))
    return g2, s_g2


def pairing_products(ctx, qs, g1, want_gt=True):
    """amdzk_pairing_products: qs = m G2Prepared, g1 = (n, m, 8) or (n * m, 8) uint64 G1Affine ((0, 0) = identity, factor 1).
    Returns (is_one (n,) bool, gt (n, 48) uint64 or None): gt[i] = prod_j e(g1[i, j], qs[j]) as halo2curves' Fq12."""
    m = len(qs)
    g1 = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 8)
    assert m and g1.shape[0] % m == 0
    n = g1.shape[0] // m
    handles = (C.c_void_p * m)(*[q.h for q in qs])
    one = np.zeros(max(1, n), np.uint8)
    gt = np.zeros((max(1, n), 48), np.uint64) if want_gt else None
    ctx._chk(ctx.L.amdzk_pairing_products(ctx.h, handles, m, _ptr(g1), n, _ptr(one), None if gt is None else _ptr(gt)))
    return one[:n].astype(bool), None if gt is None else gt[:n]


class ParamsVerifierKZG:
    """The verifier's part of ParamsKZG: the prepared [1]_2 and [s]_2 ((16,) uint64 points, e.g. from g2_setup or from a
    verifying-key file, plonk.VerifyingKey.read). `points` keeps the two as given, for VerifyingKey.write."""

    def __init__(self, ctx, g2, s_g2):
        self.ctx = ctx
        self.points = tuple(np.array(p, dtype=np.uint64).reshape(16) for p in (g2, s_g2))
        self.g2 = G2Prepared(ctx, g2)
        try:
            self.s_g2 = G2Prepared(ctx, s_g2)
        except Exception:
            self.g2.free()
            raise

    @classmethod
    def setup(cls, ctx, s):
        return cls(ctx, *g2_setup(ctx, s))

    @classmethod
    def from_bytes(cls, ctx, g2_bytes, s_g2_bytes):
        """From the two 64-byte fields of a ParamsKZG file (ParamsKZG.read): both are decompressed and must be in G2
        (g2_check status 0) — the zero fields of a file written without G2 points are refused as the identity."""
        pts = []
        for name, b in (("g2", g2_bytes), ("s_g2", s_g2_bytes)):
            q = g2_from_bytes(b)
            st = g2_check(q)
            if st != G2_IN_GROUP:
                raise _ffi.AmdzkError(-2, "ParamsVerifierKZG.from_bytes: %s is %s" % (name, _G2_STATUS[st]))
            pts.append(q)
        return cls(ctx, *pts)

    def free(self):
        self.g2.free()
        self.s_g2.free()


# ---- poly::kzg::multiopen: the opening arguments over the caller's polynomials (amdzk_multiopen_dev)
MULTIOPEN_SHPLONK = 0
MULTIOPEN_GWC = 0x100


def index_queries(queries):
    """[(polynomial, point)] -> (polynomials, points (P, 4) uint64, amdzk_open_query array). A polynomial is a device buffer
    (anything with .ptr, or an address); its identity is its address, as upstream's PolynomialPointer compares. A point is
    (4,) uint64 Montgomery; equal words share an index."""
    polys, poly_of, points, point_of = [], {}, [], {}
    q = np.zeros(len(queries), dtype=_ffi.OPEN_QUERY)
    for i, (poly, point) in enumerate(queries):
        addr = getattr(poly, "ptr", poly)
        addr = int(getattr(addr, "value", addr) or 0)
        if addr not in poly_of:
            poly_of[addr] = len(polys)
            polys.append(addr)
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(4)
        key = pt.tobytes()
        if key not in point_of:
            point_of[key] = len(points)
            points.append(pt)
        q[i] = (poly_of[addr], point_of[key])
    return polys, np.array(points, dtype=np.uint64).reshape(-1, 4), q


def multiopen_plan(points, queries, n_polys, k, scheme=MULTIOPEN_SHPLONK):
    """amdzk_multiopen_plan (host only, no device): points (P, 4) uint64 Montgomery, queries [(polynomial index, point
    index)] or an amdzk_open_query array. Returns {"n_sets", "n_out", "scratch_bytes", "set_of_poly"}; raises AmdzkError
    with the call's status for a shape amdzk_multiopen_dev refuses."""
    L = _ffi.lib()
    pts = None if points is None else np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
    if queries is not None and not (isinstance(queries, np.ndarray) and queries.dtype == _ffi.OPEN_QUERY):
        queries = np.array([tuple(int(v) for v in qq) for qq in queries], dtype=_ffi.OPEN_QUERY).reshape(-1)
    n_sets, n_out, scratch = C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    sop = np.zeros(max(1, n_polys), np.uint32)
    rc = L.amdzk_multiopen_plan(None if pts is None else _ptr(pts), 0 if pts is None else pts.shape[0],
                                None if queries is None else _ptr(queries), 0 if queries is None else queries.shape[0], n_polys, k, scheme,
                                C.byref(n_sets), C.byref(n_out), C.byref(scratch), _ptr(sop))
    if rc != 0:
        raise _ffi.AmdzkError(rc, "multiopen: the plan refuses this shape")
    return {"n_sets": n_sets.value, "n_out": n_out.value, "scratch_bytes": scratch.value, "set_of_poly": sop[:n_polys].copy()}


class _ProverMultiopen:
    """poly::commitment::Prover for KZG: create_proof(transcript, queries) writes the opening proof to the caller's
    transcript object (write_point takes (8,) uint64 affine Montgomery words, squeeze_challenge returns (4,)) and returns
    the written points, (n_out, 8) uint64."""
    scheme = MULTIOPEN_SHPLONK

    def __init__(self, params):
        self.params = params

    def create_proof(self, transcript, queries, evals=None, **kw):
        """queries: [(device buffer of 2^k coefficients, point (4,) uint64)] in upstream's order. evals: None (computed
        on the device) or (len(queries), 4) uint64, the evaluation each query claims — trusted, not checked."""
        polys, points, q = index_queries(queries)
        return multiopen(self.params, polys, points, q, transcript, self.scheme, evals=evals, **kw)


def multiopen(params, polys, points, queries, transcript, scheme=MULTIOPEN_SHPLONK, evals=None, want_points=True, out_cap=None, opts_size=None):
    """amdzk_multiopen_dev over indexed queries: polys = device addresses (or buffers with .ptr), points (P, 4) uint64
    below r (a point, a supplied evaluation or a squeezed challenge that is not raises AmdzkError, AMDZK_E_INVALID),
    queries = amdzk_open_query array or [(polynomial index, point index)]. Returns the written points (n_out, 8), or
    their number with want_points=False. out_cap / opts_size: what to report to the library (tests)."""
    from . import plonk  # the transcript trampolines (late: plonk imports this module)
    ctx = params.ctx
    addrs = []
    for p in polys:
        p = getattr(p, "ptr", p)
        addrs.append(int(getattr(p, "value", p) or 0) or None)
    d_polys = (C.c_void_p * max(1, len(addrs)))(*addrs)
    points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 4)
    if not (isinstance(queries, np.ndarray) and queries.dtype == _ffi.OPEN_QUERY):
        queries = np.array([tuple(int(v) for v in qq) for qq in queries], dtype=_ffi.OPEN_QUERY).reshape(-1)
    errors = []
    _phase, tr, keep = plonk._trampolines(None, transcript, errors)
    ev = None if evals is None else np.ascontiguousarray(evals, dtype=np.uint64).reshape(len(queries), 4)
    opts = _ffi.MultiopenOpts(C.sizeof(_ffi.MultiopenOpts) if opts_size is None else opts_size, scheme,
                              C.pointer(tr) if tr is not None else None, None if ev is None else ev.ctypes.data)
    cap = (2 if scheme == MULTIOPEN_SHPLONK else max(1, len(points))) if out_cap is None else out_cap
    out = np.zeros((max(1, cap), 8), np.uint64)
    n_out = C.c_size_t(0)
    rc = ctx.L.amdzk_multiopen_dev(ctx.h, params.h, d_polys, len(addrs), _ptr(points) if len(points) else None, len(points),
                                   _ptr(queries) if len(queries) else None, len(queries), C.byref(opts), _ptr(out) if want_points else None, cap,
                                   C.byref(n_out))
    del keep
    if errors and rc != 0:
        raise errors[0]
    ctx._chk(rc)
    return out[: n_out.value].copy() if want_points else n_out.value


class ProverSHPLONK(_ProverMultiopen):
    """poly::kzg::multiopen::ProverSHPLONK."""
    scheme = MULTIOPEN_SHPLONK


class ProverGWC(_ProverMultiopen):
    """poly::kzg::multiopen::ProverGWC."""
    scheme = MULTIOPEN_GWC


# ---- poly::kzg::multiopen: the opening arguments verified over the caller's commitments (amdzk_multiopen_verify / _decide)
def index_commitment_queries(queries):
    """[(commitment (8,) uint64, point (4,) uint64, eval (4,) uint64)] in upstream's VerifierQuery order -> (commitments (n, 8),
    points (P, 4), amdzk_open_query array, evals (Q, 4)). A commitment's identity is its words, as upstream compares
    CommitmentReference::Commitment; equal point words share an index."""
    coms, com_of, points, point_of = [], {}, [], {}
    q = np.zeros(len(queries), dtype=_ffi.OPEN_QUERY)
    evals = np.zeros((len(queries), 4), np.uint64)
    for i, (com, point, ev) in enumerate(queries):
        cm = np.ascontiguousarray(com, dtype=np.uint64).reshape(8)
        pt = np.ascontiguousarray(point, dtype=np.uint64).reshape(4)
        ci = com_of.setdefault(cm.tobytes(), len(coms))
        if ci == len(coms):
            coms.append(cm)
        pi = point_of.setdefault(pt.tobytes(), len(points))
        if pi == len(points):
            points.append(pt)
        q[i] = (ci, pi)
        evals[i] = np.ascontiguousarray(ev, dtype=np.uint64).reshape(4)
    return np.array(coms, dtype=np.uint64).reshape(-1, 8), np.array(points, dtype=np.uint64).reshape(-1, 4), q, evals


def multiopen_verify(ctx, g, commitments, points, queries, evals, transcript, scheme=MULTIOPEN_SHPLONK, vparams=None, opts_size=None):
    """amdzk_multiopen_verify (vparams None: returns (lhs, rhs), (8,) uint64 each, valid iff e(lhs, [s]_2) = e(rhs, [1]_2)) or
    amdzk_multiopen_decide (vparams a ParamsVerifierKZG: returns the verdict). g: (8,) uint64, the SRS's g[0]; commitments
    (n, 8); points (P, 4); queries an amdzk_open_query array or [(commitment index, point index)]; evals (Q, 4); transcript: the
    caller's TranscriptRead object (read_point() -> (8,) uint64, squeeze_challenge() -> (4,)). A refused call raises; an
    exception inside the transcript is re-raised."""
    arr = lambda a, w: None if a is None else np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, w)
    g, commitments, points, evals = arr(g, 8), arr(commitments, 8), arr(points, 4), arr(evals, 4)
    if queries is not None and not (isinstance(queries, np.ndarray) and queries.dtype == _ffi.OPEN_QUERY):
        queries = np.array([tuple(int(v) for v in qq) for qq in queries], dtype=_ffi.OPEN_QUERY).reshape(-1)
    errors = []
    tr, keep = (None, None) if transcript is None else _ffi.read_transcript(transcript, errors)
    opts = _ffi.MultiopenVerifyOpts(C.sizeof(_ffi.MultiopenVerifyOpts) if opts_size is None else opts_size, scheme,
                                    C.pointer(tr) if tr is not None else None)
    p = lambda a: None if a is None else _ptr(a)
    n = lambda a: 0 if a is None else a.shape[0]
    args = (ctx.h, p(g), p(commitments), n(commitments), p(points), n(points), p(queries), p(evals), n(queries), C.byref(opts))
    if vparams is None:
        pair = np.zeros(16, np.uint64)
        rc = ctx.L.amdzk_multiopen_verify(*args, _ptr(pair))
    else:
        verdict = C.c_uint8(0)
        rc = ctx.L.amdzk_multiopen_decide(*args, vparams.s_g2.h, vparams.g2.h, C.byref(verdict))
    del keep
    if errors and rc != 0:
        raise errors[0]
    ctx._chk(rc)
    return (pair[:8].copy(), pair[8:].copy()) if vparams is None else bool(verdict.value)


class _VerifierMultiopen:
    """poly::commitment::Verifier for KZG over the caller's commitments: verify_proof(transcript, queries) reads the opening
    proof from the caller's TranscriptRead object and returns the guard's pair (lhs, rhs); decide(...) pairs it too."""
    scheme = MULTIOPEN_SHPLONK

    def __init__(self, ctx, g):
        self.ctx, self.g = ctx, np.ascontiguousarray(g, dtype=np.uint64).reshape(8)

    def verify_proof(self, transcript, queries, vparams=None):
        """queries: [(commitment (8,) uint64, point (4,), eval (4,))] in upstream's order."""
        coms, points, q, evals = index_commitment_queries(queries)
        return multiopen_verify(self.ctx, self.g, coms, points, q, evals, transcript, self.scheme, vparams=vparams)

    def decide(self, transcript, queries, vparams):
        return self.verify_proof(transcript, queries, vparams=vparams)


class VerifierSHPLONK(_VerifierMultiopen):
    """poly::kzg::multiopen::VerifierSHPLONK."""
    scheme = MULTIOPEN_SHPLONK


class VerifierGWC(_VerifierMultiopen):
    """poly::kzg::multiopen::VerifierGWC."""
    scheme = MULTIOPEN_GWC
