"""Reference for amdzk_verify_proofs in Python integers: for ONE proof the two G1 sums (L_b, R_b) with
"valid <=> e(L_b, [tau]_2) = e(R_b, [1]_2)", i.e. tau * L_b == R_b for the test SRS of known tau — restated from
oracle/plonk_ref.py::verify_proof_multi with tau taken out of the final equation (the oracle multiplies one side by tau
and compares; here both sides are returned) — and a reference decode of a proof's bytes to (status, offset).

The transcript classes are looked up on the oracle module at call time, so tests/phased_oracle.py's install() (phase-major
advice commitments, challenges squeezed in between) applies to pair() exactly as it applies to the oracle's verifier: for a
phased key call pair_phased()."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import pyref as P  # noqa: E402

R, Q = PR.R, PR.Q
WELL_FORMED, BAD_LENGTH, BAD_POINT, BAD_SCALAR, BAD_INSTANCE = 0, 1, 2, 3, 4


def pair(pk, instances_list, proof, transcript="blake2b", multiopen="shplonk"):
    """(L_b, R_b) as affine points (None = identity). pk: an oracle key (its tau is not read)."""
    desc, d, n = pk.desc, pk.domain, pk.n
    bf = desc["blinding_factors"]
    N = len(instances_list)
    T = PR.Blake2bRead(proof) if transcript == "blake2b" else PR.Keccak256Read(proof)
    T.common_scalar(pk.transcript_repr)
    for instances in instances_list:
        for col in instances:
            for v in col:
                T.common_scalar(v)
    adv_c = [[T.read_point() for _ in range(desc["num_advice"])] for _ in range(N)]
    theta = T.squeeze_challenge()
    lk_c = [[(T.read_point(), T.read_point()) for _ in desc["lookups"]] for _ in range(N)]
    beta = T.squeeze_challenge()
    gamma = T.squeeze_challenge()
    chunk = desc["cs_degree"] - 2
    ncols = len(desc["permutation_columns"])
    nsets = (ncols + chunk - 1) // chunk
    z_c = [[T.read_point() for _ in range(nsets)] for _ in range(N)]
    lz_c = [[T.read_point() for _ in desc["lookups"]] for _ in range(N)]
    rand_c = T.read_point()
    y = T.squeeze_challenge()
    h_c = [T.read_point() for _ in range(d.quotient_poly_degree)]
    x = T.squeeze_challenge()
    xn = pow(x, n, R)
    adv_e = [[T.read_scalar() for _ in desc["advice_queries"]] for _ in range(N)]
    fix_e = [T.read_scalar() for _ in desc["fixed_queries"]]
    rand_e = T.read_scalar()
    sig_e = [T.read_scalar() for _ in range(ncols)]
    z_e = []
    for _ in range(N):
        ze = []
        for s in range(nsets):
            e = {0: T.read_scalar(), 1: T.read_scalar()}
            if s + 1 < nsets:
                e[-(bf + 1)] = T.read_scalar()
            ze.append(e)
        z_e.append(ze)
    lk_e = [[{("lz", 0): T.read_scalar(), ("lz", 1): T.read_scalar(), ("la", 0): T.read_scalar(), ("la", -1): T.read_scalar(),
              ("ls", 0): T.read_scalar()} for _ in desc["lookups"]] for _ in range(N)]
    lb = PR.lagrange_basis_at(d, n, [0, n - bf - 1] + list(range(n - bf, n)), x)
    l0, l_last = lb[0], lb[n - bf - 1]
    l_blind = sum(lb[i] for i in range(n - bf, n)) % R
    fq = {q: e for q, e in zip([tuple(q) for q in desc["fixed_queries"]], fix_e)}
    acc = 0
    for ci_ in range(N):
        instances = instances_list[ci_]

        def inst_eval(i, rot, instances=instances):
            col = instances[i]
            if not col:
                return 0
            basis = PR.lagrange_basis_at(d, n, range(len(col)), d.rotate_omega(x, rot))
            return sum(v * basis[j] for j, v in enumerate(col)) % R
        aq = {q: e for q, e in zip([tuple(q) for q in desc["advice_queries"]], adv_e[ci_])}

        def get(kind, i, rot, aq=aq, inst_eval=inst_eval, ci_=ci_):
            if kind == "advice":
                return aq[(i, rot)]
            if kind == "fixed":
                return fq[(i, rot)]
            if kind == "instance":
                return inst_eval(i, rot)
            if kind == "sigma":
                return sig_e[i]
            if kind == "z":
                return z_e[ci_][i][rot]
            if kind in ("lz", "la", "ls"):
                return lk_e[ci_][i][(kind, rot)]
            return {"l0": l0, "l_last": l_last, "l_active": (1 - (l_last + l_blind)) % R}[kind]

        for vv in PR.h_constraints(desc, d, get, beta, gamma, theta, x, nsets, len(desc["lookups"])):
            acc = (acc * y + vv) % R
    expected_h = acc * pow(xn - 1, -1, R) % R
    h_commit = None
    for c in reversed(h_c):
        h_commit = P.g1_add(P.g1_mul(h_commit, xn) if h_commit else None, c)
    queries = []
    Qv = lambda key, com, rot, e: queries.append((key, com, d.rotate_omega(x, rot), e))
    for ci_ in range(N):
        for (c, r), e in zip(desc["advice_queries"], adv_e[ci_]):
            Qv(("a", ci_, c), adv_c[ci_][c], r, e)
        for s in range(nsets):
            Qv(("z", ci_, s), z_c[ci_][s], 0, z_e[ci_][s][0])
            Qv(("z", ci_, s), z_c[ci_][s], 1, z_e[ci_][s][1])
        for s in reversed(range(nsets - 1)):
            Qv(("z", ci_, s), z_c[ci_][s], -(bf + 1), z_e[ci_][s][-(bf + 1)])
        for li in range(len(desc["lookups"])):
            e = lk_e[ci_][li]
            Qv(("lz", ci_, li), lz_c[ci_][li], 0, e[("lz", 0)])
            Qv(("la", ci_, li), lk_c[ci_][li][0], 0, e[("la", 0)])
            Qv(("ls", ci_, li), lk_c[ci_][li][1], 0, e[("ls", 0)])
            Qv(("la", ci_, li), lk_c[ci_][li][0], -1, e[("la", -1)])
            Qv(("lz", ci_, li), lz_c[ci_][li], 1, e[("lz", 1)])
    for (c, r), e in zip(desc["fixed_queries"], fix_e):
        Qv(("f", c), pk.fixed_commitments[c], r, e)
    for i in range(ncols):
        Qv(("s", i), pk.permutation_commitments[i], 0, sig_e[i])
    Qv(("h",), h_commit, 0, expected_h)
    Qv(("r",), rand_c, 0, rand_e)
    if multiopen == "gwc":
        v = T.squeeze_challenge()
        sets = PR.gwc_point_sets([((com, e), pt) for _, com, pt, e in queries])
        ws = [T.read_point() for _ in sets]
        u = T.squeeze_challenge()
        assert T.pos == len(T.data), "trailing bytes in proof"
        lhs = rhs = None
        up = 1
        for (z, items), w in zip(sets, ws):
            cb, eb, vp = None, 0, 1
            for com, e in items:
                cb = P.g1_add(cb, P.g1_mul(com, vp))
                eb = (eb + vp * e) % R
                vp = vp * v % R
            term = P.g1_add(cb, P.g1_neg(P.g1_mul(P.G1_GEN, eb)))
            rhs = P.g1_add(rhs, P.g1_mul(P.g1_add(term, P.g1_mul(w, z)), up))
            lhs = P.g1_add(lhs, P.g1_mul(w, up))  # the oracle multiplies by tau here
            up = up * u % R
        return lhs, rhs
    coms = {k_: c for k_, c, _, _ in queries}
    evmap = {(k_, pt): e for k_, _, pt, e in queries}
    rot_com, super_points = PR.intermediate_sets([(k_, pt) for k_, _, pt, _ in queries])
    yy = T.squeeze_challenge()
    v = T.squeeze_challenge()
    h1 = T.read_point()
    u = T.squeeze_challenge()
    h2 = T.read_point()
    assert T.pos == len(T.data), "trailing bytes in proof"
    zt = 1
    for p in super_points:
        zt = zt * (u - p) % R
    rhs = None
    vp = 1
    z0 = None
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
            term = P.g1_add(coms[key], P.g1_neg(P.g1_mul(P.G1_GEN, r_u)))
            rhs = P.g1_add(rhs, P.g1_mul(term, vp * zi % R * yp % R))
            yp = yp * yy % R
        vp = vp * v % R
    rhs = P.g1_add(rhs, P.g1_neg(P.g1_mul(h1, zt)))
    # the oracle compares h2 * (tau - u) z0 with rhs: tau * (z0 h2) == rhs + u z0 h2
    return P.g1_mul(h2, z0), P.g1_add(rhs, P.g1_mul(h2, u * z0 % R))


def pair_phased(monkeypatch, vk, desc, instances_list, proof, challenges, transcript="blake2b", multiopen="shplonk"):
    """pair() for a key with challenge phases, through tests/phased_oracle.py's verifier order (as its verify_proof). A
    verifier evaluates the expressions at the challenges IT squeezes: when the proof's bytes make the reader squeeze other
    values than `challenges` (a mutated proof), the pair is the one of the description specialised to the squeezed values —
    they depend on the bytes in front of them only, not on the specialisation, so a second pass is consistent."""
    import phased_oracle as PO

    def run(values):
        squeezed = []
        PO.install(monkeypatch, desc, len(instances_list), transcript, squeezed)
        try:
            out = pair(PO._with_desc(vk, PO.specialise(desc, values)), instances_list, proof, transcript=transcript, multiopen=multiopen)
        finally:
            PO.uninstall(monkeypatch)
        got = dict(squeezed)
        assert sorted(got) == list(range(len(values))) and len(squeezed) == len(values), "not every challenge was squeezed once"
        return out, [got[i] for i in range(len(values))]

    out, got = run(list(challenges))
    if got != [v % R for v in challenges]:
        out, again = run(got)
        assert again == got
    return out


def holds(lr, tau):
    """tau * L == R, and neither is the identity (a pair of identities would pass every tau)."""
    L, Rr = lr
    return L is not None and Rr is not None and P.g1_mul(L, tau) == Rr


def combine(pairs, rhos):
    """sum_b rho_b (L_b, R_b)."""
    L = Rr = None
    for (l, r), rho in zip(pairs, rhos):
        L, Rr = P.g1_add(L, P.g1_mul(l, rho)), P.g1_add(Rr, P.g1_mul(r, rho))
    return L, Rr


# ------------------------------------------------------------------------------------ reference decode
def element_kinds(desc, N, multiopen="shplonk"):
    """'p' / 's' per element of a proof in read order (a function of the circuit, N and the opening scheme alone)."""
    A, L = desc["num_advice"], len(desc["lookups"])
    chunk = desc["cs_degree"] - 2
    ncols = len(desc["permutation_columns"])
    nsets = (ncols + chunk - 1) // chunk
    bf = desc["blinding_factors"]
    points = N * (A + 3 * L + nsets) + 1 + (desc["cs_degree"] - 1)
    scalars = N * (len(desc["advice_queries"]) + (3 * nsets - 1 if nsets else 0) + 5 * L) + len(desc["fixed_queries"]) + 1 + ncols
    if multiopen == "gwc":
        n = 1 << desc["k"]
        rots = {r % n for _, r in desc["advice_queries"]} | {r % n for _, r in desc["fixed_queries"]} | {0}
        if nsets:
            rots |= {1}
        if nsets > 1:
            rots |= {(-(bf + 1)) % n}
        if L:
            rots |= {1, (-1) % n}
        nopen = len(rots)
    else:
        nopen = 2
    return "p" * points + "s" * scalars + "p" * nopen


def decode(desc, N, instances_list, proof, transcript="blake2b", multiopen="shplonk"):
    """(status, offset) as amdzk_verify_proofs reports them for this proof."""
    kinds = element_kinds(desc, N, multiopen)
    evm = transcript != "blake2b"
    psz = 64 if evm else 32
    if len(proof) != sum(psz if k == "p" else 32 for k in kinds):
        return BAD_LENGTH, 0
    usable = (1 << desc["k"]) - (desc["blinding_factors"] + 1)
    for instances in instances_list:
        for ci, col in enumerate(instances):
            if len(col) > usable or any(not 0 <= v < R for v in col):
                return BAD_INSTANCE, ci
    off = 0
    for k in kinds:
        if k == "p" and evm:
            x, y = int.from_bytes(proof[off:off + 32], "big"), int.from_bytes(proof[off + 32:off + 64], "big")
            if not (x < Q and y < Q and (y * y - x * x * x - 3) % Q == 0):
                return BAD_POINT, off
        elif k == "p":
            b = bytearray(proof[off:off + 32])
            b[31] &= 0x7F
            x = int.from_bytes(b, "little")
            rhs = (x * x * x + 3) % Q
            if not (x < Q and any(proof[off:off + 32]) and pow(rhs, (Q - 1) // 2, Q) == 1):
                return BAD_POINT, off
        else:
            if int.from_bytes(proof[off:off + 32], "big" if evm else "little") >= R:
                return BAD_SCALAR, off
        off += psz if k == "p" else 32
    return WELL_FORMED, 0
