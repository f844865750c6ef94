"""The device layout of a verify call (csrc/verifier.hpp, mixed_layout) restated in Python, for the tests that drive the C++
through a stand-alone program: tests/test_verifier_mixed_host.py (many groups) and tests/test_workspace_layout.py (one)."""
G1, FR, RUN, BLOCK = 64, 32, 16, 64  # sizeof(G1Affine), sizeof(Fr), AMDZK_DECIDE_RUN, verifier::MIXED_BLOCK
REGIONS = "staging items groups blocks elems elems_raw status key_g vk g points scalars msm run_bases".split()
TOTALS = "bytes up_bytes down_bytes n_blocks n_elems n_points n_scalars nvk staging_bytes run run_len".split()
PER_ITEM = "item_staging item_stride item_points item_scalars".split()
PER_GROUP = "group_elems group_vk".split()


def up(v, a):
    return (v + a - 1) // a * a


def restate(shapes, items, n_keys, per_proof):
    """mixed_layout in Python: shapes[g] = (E, NP, NS, nvk, proof_bytes, raw_bytes), items[b] = (group, raw)."""
    out = {"group_elems": [], "group_vk": [], "item_staging": [], "item_stride": [], "item_points": [], "item_scalars": []}
    n_elems = nvk = 0
    for E, NP, NS, v, pb, rb in shapes:
        out["group_elems"].append(n_elems)
        out["group_vk"].append(nvk)
        n_elems, nvk = n_elems + E, nvk + v
    staging = points = scalars = blocks = 0
    for g, raw in items:
        E, NP, NS, v, pb, rb = shapes[g]
        stride = up(rb if raw else pb, 32)
        out["item_staging"].append(staging)
        out["item_stride"].append(stride)
        out["item_points"].append(points)
        out["item_scalars"].append(scalars)
        staging, points, scalars, blocks = staging + stride, points + NP, scalars + NS, blocks + (E + BLOCK - 1) // BLOCK
    n = len(items)
    run, run_len = min(n, RUN), 0
    for b0 in range(0, n if per_proof else 0, run):
        chunk = items[b0:b0 + run]
        run_len = max(run_len, 1 + sum(shapes[g][1] for g, _ in chunk) + sum(shapes[g][3] for g in {g for g, _ in chunk}))
    any_raw = any(raw for _, raw in items)
    off, at = 0, {}

    def take(name, size, pad=256):
        nonlocal off
        at[name] = off
        off = up(off + size, pad)
    take("staging", staging), take("items", n * 32), take("groups", len(shapes) * 16), take("blocks", blocks * 8), take("elems", n_elems * 8)
    take("elems_raw", n_elems * 8 if any_raw else 0), take("status", n * 4), take("key_g", n_keys * G1)
    take("vk", nvk * G1, 1), take("g", G1, 1), take("points", points * G1, 1), take("scalars", scalars * FR)
    if per_proof:
        take("msm", 2 * run * run_len * FR)
    else:
        take("msm", 2 * (nvk + 1 + points) * FR, 1)
    take("run_bases", run_len * G1 if per_proof else 0, 1)
    out["regions"] = [at[r] for r in REGIONS]
    out["totals"] = [off, at["g"], at["msm"] - at["status"], blocks, n_elems, points, scalars, nvk, staging, run, run_len]
    return out
