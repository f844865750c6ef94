"""Reference for amdzk_multiopen_verify in Python integers: the two G1 sums (L, R) of the opening argument verified alone,
with "valid <=> e(L, [tau]_2) = e(R, [1]_2)", i.e. tau * L == R for a test SRS of known tau — restated from the tail of
oracle/plonk_ref.py::verify_proof_multi (as tests/verify_ref.py restates the whole verifier) with the caller's commitments
in the place of a proof's, tau taken out of the final equation and no h(X) expansion:
  SHPLONK  L = z_0(u) h2      R = sum_i v^i z_i(u) sum_j y^j (C_ij - r_ij(u) G) - Z_T(u) h1 + u z_0(u) h2
  GWC      L = sum_i u^i W_i  R = sum_i u^i (z_i W_i + sum_j v^j (C_ij - e_ij G))
Grouping is the oracle's own (intermediate_sets, gwc_point_sets) over (commitment index, point VALUE): equal point values
are one point; SHPLONK takes the first query of every (commitment, point value) pair, GWC every query's own.
tests/test_opening_verify_ref.py holds this file to the oracle's shplonk_prove / gwc_prove."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402

R = PR.R


def n_read(scheme, point_vals, queries):
    """Points the verifier reads: 2, or one per distinct queried point value."""
    return 2 if scheme == "shplonk" else len({point_vals[z] for _, z in queries})


def read(scheme, T, point_vals, queries):
    """The verifier's read order on a read transcript (squeeze_challenge / read_point in ints): (challenges, points)."""
    if scheme == "shplonk":
        y, v = T.squeeze_challenge(), T.squeeze_challenge()
        h1 = T.read_point()
        u = T.squeeze_challenge()
        return (y, v, u), [h1, T.read_point()]
    v = T.squeeze_challenge()
    ws = [T.read_point() for _ in range(n_read(scheme, point_vals, queries))]
    return (v, T.squeeze_challenge()), ws


def pair(scheme, coms, point_vals, queries, evals, challenges, points, g=P.G1_GEN):
    """coms: affine points (None = the identity); queries: [(commitment index, point index)]; evals: one int per query;
    challenges / points: what read() returned. (L, R) as affine points, None = the identity."""
    if scheme == "gwc":
        v, u = challenges
        sets = PR.gwc_point_sets([((c, e), point_vals[z]) for (c, z), e in zip(queries, evals)])
        assert len(sets) == len(points)
        lhs = rhs = None
        up = 1
        for (z, items), w in zip(sets, points):
            cb, eb, vp = None, 0, 1
            for c, e in items:
                cb = P.g1_add(cb, P.g1_mul(coms[c], vp)) if coms[c] is not None else cb
                eb = (eb + vp * e) % R
                vp = vp * v % R
            term = P.g1_add(cb, P.g1_neg(P.g1_mul(g, eb))) if eb else cb
            rhs = P.g1_add(rhs, P.g1_mul(P.g1_add(term, P.g1_mul(w, z) if z else None), up))
            lhs = P.g1_add(lhs, P.g1_mul(w, up))
            up = up * u % R
        return lhs, rhs
    y, v, u = challenges
    h1, h2 = points
    keyed = [(c, point_vals[z]) for c, z in queries]
    evmap = {}
    for key, e in zip(keyed, evals):
        evmap.setdefault(key, e)  # the first query of a (commitment, point value) pair
    rot_com, super_points = PR.intermediate_sets(keyed)
    zt = 1
    for p in super_points:
        zt = zt * (u - p) % R
    rhs, vp, z0 = None, 1, None
    for pts, keys in rot_com:
        zi = 1
        for p in super_points:
            if p not in pts:
                zi = zi * (u - p) % R
        if z0 is None:
            z0 = zi
        yp = 1
        for key in keys:
            low = PR.lagrange_interpolate(list(pts), [evmap[(key, p)] for p in pts])
            r_u = P.eval_polynomial(low, u)
            coef = vp * zi % R * yp % R
            term = P.g1_neg(P.g1_mul(g, r_u)) if r_u else None
            if coms[key] is not None:
                term = P.g1_add(coms[key], term)
            if coef and term is not None:
                rhs = P.g1_add(rhs, P.g1_mul(term, coef))
            yp = yp * y % R
        vp = vp * v % R
    if zt:
        rhs = P.g1_add(rhs, P.g1_neg(P.g1_mul(h1, zt)))
    if z0 == 0:
        return None, rhs
    return P.g1_mul(h2, z0), P.g1_add(rhs, P.g1_mul(h2, u * z0 % R))


def holds(lr, tau):
    """tau * L == R, and neither is the identity."""
    L, Rr = lr
    return L is not None and Rr is not None and P.g1_mul(L, tau) == Rr


def opening_of(case, scheme, tau, transcript_cls=PR.Blake2bWrite):
    """A tests/multiopen_cases.py Case as the verifier sees it: (commitments over the test SRS of `tau`, one evaluation per
    query, the bytes the oracle's prover wrote)."""
    coms = [PR.commit_tau(p, tau) for p in case.polys]
    evals = [P.eval_polynomial(case.polys[p], case.point_vals[z]) for p, z in case.queries]
    _pts, proof, _next = case.oracle(scheme, transcript_cls)
    return coms, evals, proof
