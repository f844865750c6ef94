"""CPU: amdzk_multiopen_plan — the host half of the stand-alone KZG multiopen (include/amdzk.h) — builds SHPLONK's and
GWC's sets exactly as the protocol oracle does (oracle/plonk_ref.py intermediate_sets / gwc_point_sets), reports the
documented scratch size, and refuses what the call refuses, all without a device."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402

E_INVALID, E_NOMEM = -2, -4
NONE = 0xFFFFFFFF


def random_case(rng):
    """1-12 polynomials, 1-9 point indices over 1-6 distinct values (so equal values under different indices occur),
    duplicate queries, and usually some polynomial no query names."""
    n_polys, n_points = rng.randint(1, 12), rng.randint(1, 9)
    values = [rng.randrange(zu.R) for _ in range(rng.randint(1, 6))]
    # a small and a large value side by side: numeric order differs from the order of the Montgomery words
    if rng.random() < 0.3:
        values[0] = rng.randint(0, 3)
    point_vals = [rng.choice(values) for _ in range(n_points)]
    queried = rng.sample(range(n_polys), rng.randint(1, n_polys))
    queries = [(rng.choice(queried), rng.randrange(n_points)) for _ in range(rng.randint(1, 30))]
    if rng.random() < 0.5:
        queries += [rng.choice(queries) for _ in range(rng.randint(1, 4))]
        rng.shuffle(queries)
    return n_polys, point_vals, queries


def expected(n_polys, point_vals, queries, k):
    """What the oracle's grouping says, and the header's scratch formulas evaluated on it."""
    keyed = [(p, point_vals[z]) for p, z in queries]
    n = 1 << k
    Q, E, Cq = len(keyed), len(set(keyed)), len({p for p, _ in keyed})
    rot_com, _super = PR.intermediate_sets(keyed)
    sop = [NONE] * n_polys
    for i, (_pts, keys) in enumerate(rot_com):
        for p in keys:
            sop[p] = i
    S, P, M = len(rot_com), sum(len(t) for t, _ in rot_com), max(len(t) for t, _ in rot_com)
    ptrs, frs = E + Cq + 2 * P + S + 2, 2 * E + Cq + 2 * P + P * M + S + 3
    shplonk = {"n_sets": S, "n_out": 2, "set_of_poly": sop, "scratch_bytes": (S + P + 1) * n * 32 + (ptrs * 8 + 255) // 256 * 256 + frs * 32}
    gsets = PR.gwc_point_sets(keyed)
    sop = [NONE] * n_polys
    for i, (_z, items) in reversed(list(enumerate(gsets))):
        for p in items:
            sop[p] = i
    S = len(gsets)
    ptrs, frs = E + Q + S, 2 * E + Q + 2 * S
    gwc = {"n_sets": S, "n_out": S, "set_of_poly": sop, "scratch_bytes": S * n * 32 + (ptrs * 8 + 255) // 256 * 256 + frs * 32}
    return shplonk, gwc


def test_plan_groups_queries_as_the_oracle_does(pkg):
    rng = random.Random(20260)
    kzg = pkg.kzg
    seen_shared_value = seen_unqueried = seen_duplicate = 0
    for case in range(200):
        n_polys, point_vals, queries = random_case(rng)
        k = rng.randint(1, 12)
        pts = zu.fr_array_from_ints(point_vals)
        want_s, want_g = expected(n_polys, point_vals, queries, k)
        used = {z for _, z in queries}
        seen_shared_value += len({point_vals[z] for z in used}) < len(used)
        seen_unqueried += len({p for p, _ in queries}) < n_polys
        seen_duplicate += len(set(queries)) < len(queries)
        for scheme, want in ((kzg.MULTIOPEN_SHPLONK, want_s), (kzg.MULTIOPEN_GWC, want_g)):
            got = kzg.multiopen_plan(pts, queries, n_polys, k, scheme)
            assert got["n_sets"] == want["n_sets"] and got["n_out"] == want["n_out"], (case, scheme, queries, point_vals)
            assert [int(v) for v in got["set_of_poly"]] == want["set_of_poly"], (case, scheme, queries, point_vals)
            assert got["scratch_bytes"] == want["scratch_bytes"], (case, scheme)
    assert seen_shared_value > 20 and seen_unqueried > 20 and seen_duplicate > 20  # the generator reaches what it is for


def test_plan_orders_points_by_canonical_value_not_by_their_words(pkg):
    """Two polynomials opened at {1, r - 1} written with the indices swapped are one SHPLONK set: sets are compared as
    sorted VALUES. (The Montgomery words of 1 are numerically larger than those of many larger values.)"""
    pts = zu.fr_array_from_ints([1, zu.R - 1, zu.R - 1, 1, 5])
    got = pkg.kzg.multiopen_plan(pts, [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 0)], 3, 4)
    assert got["n_sets"] == 2 and [int(v) for v in got["set_of_poly"]] == [0, 0, 1]


def test_plan_outputs_are_optional_and_untouched_on_refusal(pkg):
    L = pkg.lib()
    pts = zu.fr_array_from_ints([3, 4])
    q = np.array([(0, 0), (1, 1)], dtype=pkg.ffi.OPEN_QUERY)
    assert L.amdzk_multiopen_plan(pts.ctypes.data, 2, q.ctypes.data, 2, 2, 4, 0, None, None, None, None) == 0
    n_sets = C.c_uint32(77)
    assert L.amdzk_multiopen_plan(pts.ctypes.data, 2, q.ctypes.data, 2, 1, 4, 0, C.byref(n_sets), None, None, None) == E_INVALID
    assert n_sets.value == 77


@pytest.mark.parametrize("what", ["null points", "null queries", "no queries", "poly index", "point index", "scheme", "k"])
def test_plan_refuses_what_the_call_refuses(pkg, what):
    L = pkg.lib()
    pts = zu.fr_array_from_ints([3, 4])
    q = np.array([(0, 0), (1, 1)], dtype=pkg.ffi.OPEN_QUERY)
    a = {"points": pts.ctypes.data, "n_points": 2, "queries": q.ctypes.data, "n_queries": 2, "n_polys": 2, "k": 4, "scheme": 0}
    a.update({"null points": {"points": None}, "null queries": {"queries": None}, "no queries": {"n_queries": 0},
              "poly index": {"n_polys": 1}, "point index": {"n_points": 1}, "scheme": {"scheme": 1}, "k": {"k": 31}}[what])
    for scheme in ((a["scheme"],) if what == "scheme" else (0, pkg.kzg.MULTIOPEN_GWC)):
        rc = L.amdzk_multiopen_plan(a["points"], a["n_points"], a["queries"], a["n_queries"], a["n_polys"], a["k"], scheme, None, None, None, None)
        assert rc == E_INVALID, (what, scheme)


def test_plan_reports_sizes_past_any_device(pkg):
    """The limit is memory and the plan only reports it: three sets of one point at k = 30 are (3 + 3 + 1) 2^30 32 bytes
    of polynomials, 224 GiB, computed in 64 bits."""
    got = pkg.kzg.multiopen_plan(zu.fr_array_from_ints(range(1, 4)), [(0, 0), (1, 1), (2, 2)], 3, 30)
    assert (3 + 3 + 1) << 35 < got["scratch_bytes"] < ((3 + 3 + 1) << 35) + 4096


def test_python_mirror_indexes_queries_by_address_and_value(pkg):
    class Buf:
        def __init__(self, ptr):
            self.ptr = C.c_void_p(ptr)
    a, b = Buf(0x1000), Buf(0x2000)
    x, y = zu.fr_from_int(5), zu.fr_from_int(6)
    polys, points, q = pkg.kzg.index_queries([(a, x), (b, y), (Buf(0x1000), zu.fr_from_int(6)), (a, x)])
    assert polys == [0x1000, 0x2000] and points.shape == (2, 4)
    assert [(int(e["poly"]), int(e["point"])) for e in q] == [(0, 0), (1, 1), (0, 1), (0, 0)]
