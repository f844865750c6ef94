"""CPU: the multiopen argument's shared host arithmetic (csrc/opening.hpp) alone, in a stand-alone program (tests/native/
opening_check.cpp, plain g++): the grouping against oracle/plonk_ref.py's intermediate_sets / gwc_point_sets, R_i against
lagrange_interpolate coefficient by coefficient, and c_it, the division table, z_i(u), Z_T(u), the Lagrange weights at u, the
scaled coefficients and the constant term against direct products — equal as field elements, no tolerance. Once more in a
build with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import os
import random
import subprocess

import pytest

import multiopen_cases as MC
from test_multiopen_plan import random_case

PR = MC.PR
R = PR.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "opening_check.cpp")
SEEDS = 300


class Case:
    """queries: (commitment, point id); pts: the values by id; evals: one claimed evaluation per query."""

    def __init__(self, name, n_coms, pts, queries, evals, y, v, u):
        self.name, self.n_coms, self.pts, self.queries, self.evals, self.y, self.v, self.u = name, n_coms, pts, queries, evals, y, v, u

    def text(self):
        h = lambda a: "%064x" % a
        return "\n".join(["%d %d %d" % (self.n_coms, len(self.pts), len(self.queries))] + ["%d %d" % q for q in self.queries] +
                         [h(a) for a in self.pts + self.evals + [self.y, self.v, self.u]]) + "\n"


def with_ids(name, rng, n_coms, point_vals, queries, ranks, evals=None):
    """Point ids as the stand-alone call assigns them (ranks of the distinct queried values, ascending) or as the proof
    path and the verifier do (first seen first); random claimed evaluations unless the caller has real ones."""
    seen = list(dict.fromkeys(point_vals[z] for _, z in queries))
    pts = sorted(seen) if ranks else seen
    qs = [(p, pts.index(point_vals[z])) for p, z in queries]
    if evals is None:
        evals = [rng.randrange(R) for _ in qs]  # a repeated (commitment, point) claims another value: the first one counts
    return Case(name, n_coms, pts, qs, evals, rng.randrange(R), rng.randrange(R), rng.randrange(R))


def make_cases():
    rng = random.Random(20261)
    out = []
    for seed in range(SEEDS):
        n_polys, point_vals, queries = random_case(random.Random(seed))
        out.append(with_ids("random %d" % seed, rng, n_polys, point_vals, queries, ranks=seed % 2 == 0))
    for name in ("shared", "17 sets"):
        c = MC.make_case(name)
        evals = [PR.P.eval_polynomial(c.polys[p], c.point_vals[z]) for p, z in c.queries]
        out.append(with_ids(name, rng, len(c.polys), c.point_vals, c.queries, ranks=True, evals=evals))
        out.append(with_ids(name + ", first seen", rng, len(c.polys), c.point_vals, c.queries, ranks=False, evals=evals))
    # ids first seen first over values that are NOT ascending (and whose Montgomery words order differently again)
    vals = [R - 1, 5, 1 << 200, 2, (1 << 253) + 7]
    out.append(with_ids("descending ids", rng, 3, vals, [(0, 0), (0, 1), (1, 2), (0, 3), (1, 0), (2, 4), (2, 3), (1, 3), (0, 2)], ranks=False))
    # one point next to a five-point set: R_0 is padded to maxm = 5; and a single point alone, maxm = 1
    vals = [rng.randrange(R) for _ in range(5)]
    out.append(with_ids("1 and 5 points", rng, 2, vals, [(0, 2)] + [(1, z) for z in (4, 0, 3, 1, 2)], ranks=False))
    out.append(with_ids("one point alone", rng, 1, vals, [(0, 1)], ranks=True))
    # u on a point outside the first set: z_0(u) = 0 is reported, not failed
    c = with_ids("z0 = 0", rng, 2, vals, [(0, 0), (1, 1), (1, 0)], ranks=False)
    c.u = c.pts[1]
    out.append(c)
    # degenerate challenges on the "shared" sets: y = 0 keeps the first commitment of a set alone, v = 0 the first set alone,
    # u = 0 is a point like any other (no point of the case is 0: z_0(u) != 0)
    c = MC.make_case("shared")
    evals = [PR.P.eval_polynomial(c.polys[p], c.point_vals[z]) for p, z in c.queries]
    for what in ("y", "v", "u"):
        d = with_ids("shared, %s = 0" % what, rng, len(c.polys), c.point_vals, c.queries, ranks=what != "v", evals=evals)
        setattr(d, what, 0)
        out.append(d)
    # the point values 0, 1, r - 1 (under two indices), omega, z, -z, and 0 under a second index
    c = MC.make_case("edge points")
    evals = [PR.P.eval_polynomial(c.polys[p], c.point_vals[z]) for p, z in c.queries]
    out.append(with_ids("edge points", rng, len(c.polys), c.point_vals, c.queries, ranks=True, evals=evals))
    out.append(with_ids("edge points, first seen", rng, len(c.polys), c.point_vals, c.queries, ranks=False, evals=evals))
    return out


CASES = make_cases()
_results = {}


def results(tmp_path_factory, sanitized):
    """The program's output for every case, parsed: one build and one run per flavour."""
    if sanitized not in _results:
        from test_sanitizers import ENV, SAN
        d = tmp_path_factory.mktemp("opening_check")
        exe, cf = str(d / "opening_check"), str(d / "cases.txt")
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        with open(cf, "w") as f:
            f.write("".join(c.text() for c in CASES))
        p = subprocess.run([exe, cf], text=True, capture_output=True, env=ENV if sanitized else None, timeout=300)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
        lines = p.stdout.split("\n")
        assert lines[-2:] == ["ok", ""]
        got = []
        for ln in lines[:-2]:
            w = ln.split()
            if w[0] == "case":
                got.append({})
            elif w[0] in ("coms", "shape", "z0_zero"):
                got[-1][w[0]] = [int(a) for a in w[1:] if a != "|"]
            elif w[0] in ("com", "set", "gw", "order"):
                got[-1].setdefault(w[0], []).append([[int(a) for a in part.split()] for part in ln.split("|")[1:]])
            elif w[0] == "row":
                got[-1].setdefault("row", []).append((int(w[1]), [int(a, 16) for a in w[2:]]))
            else:
                got[-1].setdefault(w[0], []).append([int(a, 16) for a in w[2:]])
        assert len(got) == len(CASES)
        _results[sanitized] = got
    return _results[sanitized]


def prod(xs):
    out = 1
    for a in xs:
        out = out * a % R
    return out


def expected(c, _memo={}):
    """The oracle's sets and, per set, what the protocol defines over them (computed once per case)."""
    if c.name not in _memo:
        _memo[c.name] = _expected(c)
    return _memo[c.name]


def _expected(c):
    keyed = [(p, c.pts[z]) for p, z in c.queries]
    first = {}
    for i, key in enumerate(keyed):
        first.setdefault(key, c.evals[i])
    rot_com, super_pts = PR.intermediate_sets(keyed)
    sets = []
    for pts, keys in rot_com:
        low, E = [0] * len(pts), [0] * len(pts)
        for j, key in enumerate(keys):
            ev = [first[(key, p)] for p in pts]
            yj = pow(c.y, j, R)
            low = [(a + yj * b) % R for a, b in zip(low, PR.lagrange_interpolate(list(pts), ev))]
            E = [(a + yj * b) % R for a, b in zip(E, ev)]
        cit = [pow(prod(pts[t] - pts[s] for s in range(len(pts)) if s != t), -1, R) for t in range(len(pts))]
        w = [cit[t] * prod(c.u - pts[s] for s in range(len(pts)) if s != t) % R for t in range(len(pts))]
        z = prod(c.u - p for p in super_pts if p not in pts)
        sets.append({"pts": list(pts), "keys": keys, "low": low, "E": E, "c": cit, "w": w, "z": z})
    return keyed, sets, super_pts


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan+ubsan"])
def test_grouping_is_the_oracles(tmp_path_factory, sanitized):
    for c, got in zip(CASES, results(tmp_path_factory, sanitized)):
        keyed, sets, _ = expected(c)
        coms = got["coms"]
        assert coms == list(dict.fromkeys(p for p, _ in c.queries)), c.name
        for ci, (ids, firsts) in enumerate(got["com"]):
            assert ids == sorted({z for p, z in c.queries if p == coms[ci]}), c.name
            assert firsts == [c.queries.index((coms[ci], z)) for z in ids], c.name  # a second query of a pair is dropped
        assert len(got.get("set", [])) == len(sets), c.name
        for (ids, members), order, pts, want in zip(got["set"], got["order"], got["pts"], sets):
            assert ids == sorted(ids) and [c.pts[ids[o]] for o in order[0]] == want["pts"] == pts, c.name
            assert [coms[m] for m in members] == want["keys"], c.name
        assert got["shape"] == [sum(len(s["pts"]) for s in sets), max(len(s["pts"]) for s in sets)], c.name
        gw = [g[0] for g in got["gw"]]
        assert gw == [[i for i, (_, z) in enumerate(c.queries) if z == pid] for pid in range(len(c.pts))], c.name
        by_first = sorted((g for g in gw if g), key=lambda g: g[0])
        assert [(keyed[g[0]][1], [keyed[i][0] for i in g]) for g in by_first] == PR.gwc_point_sets(keyed), c.name
    assert any(o[0] != sorted(o[0]) for got in results(tmp_path_factory, sanitized) for o in got["order"])  # the per-set sort had work to do


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan+ubsan"])
def test_shplonk_scalars_up_to_h(tmp_path_factory, sanitized):
    for c, got in zip(CASES, results(tmp_path_factory, sanitized)):
        _, sets, _ = expected(c)
        maxm = max(len(s["pts"]) for s in sets)
        rows = []
        for i, s in enumerate(sets):
            assert got["c"][i] == s["c"] and got["E"][i] == s["E"] and got["low"][i] == s["low"], (c.name, i)
            rows += [(i, [p, pow(c.v, i, R) * ct % R] + s["low"] + [0] * (maxm - len(s["low"]))) for p, ct in zip(s["pts"], s["c"])]
        assert got["row"] == rows, c.name
    assert any(len({len(s) for s in got["low"]}) > 1 for got in results(tmp_path_factory, sanitized))  # some R_i was padded


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan+ubsan"])
def test_shplonk_scalars_behind_u(tmp_path_factory, sanitized):
    zero_seen = 0
    for c, got in zip(CASES, results(tmp_path_factory, sanitized)):
        _, sets, super_pts = expected(c)
        zt, z0 = prod(c.u - p for p in super_pts), sets[0]["z"]
        assert got["zt"] == [[zt]] and got["z0"] == [[z0]] and got["z0_zero"] == [int(z0 == 0)], c.name
        assert got["z"] == [[s["z"]] for s in sets] and got["w"] == [s["w"] for s in sets], c.name
        zero_seen += z0 == 0
        if z0 == 0:
            continue
        z0inv = pow(z0, -1, R)
        cf = [pow(c.v, i, R) * s["z"] * z0inv % R for i, s in enumerate(sets)]
        assert got["cf"] == [cf + [-zt * z0inv % R]], c.name
        assert got["cterm"] == [[sum(a * PR.P.eval_polynomial(s["low"], c.u) for a, s in zip(cf, sets)) % R]], c.name
        for s in sets:  # the weights interpolate: sum_t w_t E_t = R_i(u)
            assert sum(a * b for a, b in zip(s["w"], s["E"])) % R == PR.P.eval_polynomial(s["low"], c.u), c.name
    assert zero_seen == 1
