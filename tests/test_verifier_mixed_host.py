"""CPU: the two pure host functions behind amdzk_verify_proofs_mixed (csrc/verifier.hpp) — group_items and mixed_layout — in a
stand-alone program (tests/native/verifier_mixed_check.cpp), built plainly and with ASan + UBSan and run as an executable
(nothing is loaded into Python). Groups are numbered first seen first; the device layout is restated here in Python and must
agree number for number; its regions are disjoint, in order and aligned, every item's staging offset is a multiple of 32, the
base array of the combined MSM is contiguous, and 2^20 one-element items lay out without overflow."""
import os
import random
import subprocess

import pytest

from verify_layout_model import FR, G1, REGIONS, RUN, TOTALS, restate  # the layout in Python, shared with test_workspace_layout.py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "verifier_mixed_check.cpp")
_exe = {}


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("verifier_mixed_check") / ("verifier_mixed_check_san" if sanitized else "verifier_mixed_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


@pytest.fixture(params=[False, True], ids=["plain", "asan_ubsan"])
def exe(request, tmp_path_factory):
    return build(tmp_path_factory, request.param), request.param


def call(exe, text):
    path, sanitized = exe
    env = None
    if sanitized:
        from test_sanitizers import ENV
        env = ENV
    p = subprocess.run([path], input=text, text=True, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.split("\n")
    assert lines[-2:] == ["ok", ""]
    return {ln.split(" ", 1)[0]: [int(v) for v in ln.split()[1:]] for ln in lines[:-2]}


def layout_text(shapes, items, n_keys, per_proof):
    return ("layout %d %d %d %d\n" % (len(shapes), len(items), n_keys, per_proof) + "\n".join(" ".join(map(str, s)) for s in shapes) + "\n" +
            " ".join("%d %d" % it for it in items) + "\n")


def check_properties(got, shapes, items, n_keys, per_proof):
    at, tot = dict(zip(REGIONS, got["regions"])), dict(zip(TOTALS, got["totals"]))
    n = len(items)
    sizes = {"staging": tot["staging_bytes"], "items": n * 32, "groups": len(shapes) * 16, "blocks": tot["n_blocks"] * 8, "elems": tot["n_elems"] * 8,
             "elems_raw": tot["n_elems"] * 8 if any(r for _, r in items) else 0, "status": n * 4, "key_g": n_keys * G1, "vk": tot["nvk"] * G1, "g": G1,
             "points": tot["n_points"] * G1, "scalars": tot["n_scalars"] * FR,
             "msm": 2 * tot["run"] * tot["run_len"] * FR if per_proof else 2 * (tot["nvk"] + 1 + tot["n_points"]) * FR,
             "run_bases": tot["run_len"] * G1 if per_proof else 0}
    # in order and disjoint; everything 32-byte aligned (16-byte loads, G1Affine and Fr stores), the tables at 256
    for a, b in zip(REGIONS, REGIONS[1:]):
        assert at[a] + sizes[a] <= at[b], (a, b)
    assert at["run_bases"] + sizes["run_bases"] <= tot["bytes"]
    assert all(at[r] % 32 == 0 for r in REGIONS) and all(at[r] % 256 == 0 for r in REGIONS[:9])
    # commitments | G | points: the base array of the combined MSM has no gap
    assert at["g"] == at["vk"] + sizes["vk"] and at["points"] == at["g"] + G1
    # one upload ends where G begins; one download from the status words to the MSM's scalars
    assert tot["up_bytes"] == at["g"] and tot["down_bytes"] == at["msm"] - at["status"]
    # items: staging offsets multiples of 32, back to back, each holding the form it carries
    st, sd = got["item_staging"], got["item_stride"]
    for b, (g, raw) in enumerate(items):
        assert st[b] % 32 == 0 and sd[b] % 32 == 0 and sd[b] >= shapes[g][5 if raw else 4]
        assert st[b] + sd[b] == (st[b + 1] if b + 1 < n else tot["staging_bytes"])
        assert got["item_points"][b] + shapes[g][1] == (got["item_points"][b + 1] if b + 1 < n else tot["n_points"])
        assert got["item_scalars"][b] + shapes[g][2] == (got["item_scalars"][b + 1] if b + 1 < n else tot["n_scalars"])


def test_groups_are_numbered_first_seen_first(exe):
    keys = [(0x7000, 1, 0), (0x1000, 1, 0), (0x7000, 1, 0), (0x7000, 2, 0), (0x1000, 1, 0x101), (0x1000, 1, 0), (0x7000, 1, 1), (0x7000, 2, 0), (0x10, 1, 0)]
    got = call(exe, "groups %d\n" % len(keys) + "\n".join("%d %d %d" % k for k in keys) + "\n")
    seen = []
    want = [seen.index(k) if k in seen else (seen.append(k), len(seen) - 1)[1] for k in keys]
    assert want == [0, 1, 0, 2, 3, 1, 4, 2, 5]  # neither sorted by handle nor by kind
    assert got["of"] == want and got["firsts"] == [keys.index(k) for k in seen]
    rng = random.Random(3)
    keys = [(rng.choice([8, 16, 24, 32]), rng.choice([1, 2]), rng.choice([0, 1, 0x100, 0x101])) for _ in range(300)]
    got = call(exe, "groups %d\n" % len(keys) + "\n".join("%d %d %d" % k for k in keys) + "\n")
    seen = []
    assert got["of"] == [seen.index(k) if k in seen else (seen.append(k), len(seen) - 1)[1] for k in keys]
    assert got["firsts"] == [keys.index(k) for k in seen] and len(seen) == 32
    assert call(exe, "groups 0\n") == {"of": [], "firsts": []}


# (E, NP, NS, nvk, proof_bytes, raw_bytes): a square-like key, a lookup key in the EVM form, element counts 63 / 64 / 65, a key
# without commitments
SHAPES = [(16, 9, 7, 3, 512, 800), (40, 17, 23, 9, 40 * 32 + 17 * 32, 17 * 64 + 23 * 32), (63, 30, 33, 5, 2016, 2976), (64, 30, 34, 5, 2048, 3008),
          (65, 31, 34, 6, 2080, 3072), (1, 1, 0, 0, 32, 64)]


@pytest.mark.parametrize("per_proof", [0, 1])
def test_the_layout_is_the_restatement_and_its_regions_are_disjoint_and_aligned(exe, per_proof):
    rng = random.Random(11 + per_proof)
    batches = [[(0, 0)], [(2, 0)], [(3, 1)], [(4, 0), (5, 0)], [(g % 4, 0) for g in range(40)], [(rng.randrange(6), rng.randrange(2)) for _ in range(53)],
               [(5, 1)] * 17, [(1, 0)] * 16 + [(0, 0)], [(rng.randrange(6), 0) for _ in range(32)]]
    for items in batches:
        n_keys = 1 + len({g for g, _ in items}) // 2
        got = call(exe, layout_text(SHAPES, items, n_keys, per_proof))
        assert got == restate(SHAPES, items, n_keys, per_proof), items
        check_properties(got, SHAPES, items, n_keys, per_proof)
    # a run's base list: the commitments of the groups PRESENT in it, once each
    got = call(exe, layout_text(SHAPES, [(0, 0)] * 16 + [(1, 0), (0, 0), (1, 0)], 2, 1))
    assert dict(zip(TOTALS, got["totals"]))["run_len"] == max(3 + 1 + 16 * 9, 3 + 9 + 1 + 9 + 2 * 17)


def test_two_to_the_twenty_one_element_items(exe):
    n = 1 << 20
    shapes = [(1, 1, 0, 0, 32, 64), (1, 0, 1, 2, 32, 32)]
    items = [(b & 1, 0) for b in range(n)]
    for per_proof in (0, 1):
        got = call(exe, layout_text(shapes, items, 2, per_proof))
        assert got == restate(shapes, items, 2, per_proof)
        tot = dict(zip(TOTALS, got["totals"]))
        assert tot["n_blocks"] == n and tot["n_points"] == n // 2 and tot["staging_bytes"] == 32 * n and tot["run"] == RUN
        assert got["item_staging"][-1] == 32 * (n - 1) and got["item_points"][-2] == n // 2 - 1 and got["item_points"][-1] == n // 2
        check_properties(got, shapes, items, 2, per_proof)


def test_offsets_do_not_wrap_at_four_gib(exe):
    """A batch may exceed 4 GiB although one proof stays below 2^30: staging offsets are size_t."""
    shapes = [(64, 30, 34, 5, (1 << 30) - 32, (1 << 30) - 32)]
    items = [(0, b & 1) for b in range(9)]
    got = call(exe, layout_text(shapes, items, 1, 0))
    assert got == restate(shapes, items, 1, 0)
    assert got["item_staging"][8] == 8 * ((1 << 30) - 32) > 1 << 32
