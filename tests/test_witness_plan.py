"""CPU: witness programs as far as they go without a device — amdzk_witness_plan (pure host code): the levels against the
reference's longest path on random DAGs, the launches against a restatement of the documented fusing rule, the workspace
against the documented formula, and every refusal of the description with its message prefix."""
import ctypes as C
import random

import numpy as np
import pytest

import witness_cases as WC
import witness_ref as WR

E_INVALID, E_UNSUPPORTED = -2, -5
R = WR.R


@pytest.fixture(scope="module")
def W(pkg):
    return pkg.witness.WitnessProgram


def test_levels_launches_and_workspace_on_random_dags(W):
    rng = random.Random(20260101)
    seen_depths = set()
    for t in range(200):
        p = WC.random_program(W, rng, n_nodes=rng.randrange(0, 400), n_inputs=rng.randrange(1, 9), near=rng.choice([0.0, 0.1, 0.5]),
                              recent=rng.choice([0.0, 0.3, 0.5]))
        for i in rng.sample(range(len(p.nodes)), min(3, len(p.nodes))):
            p.expose(i)
        if t % 2:
            p.assign(len(p.nodes) - 1, 0, 0)
        n_proofs = rng.choice([1, 2, 3, 7, 64, 65, 700])
        pl = p.plan(n_proofs)
        widths = WR.level_widths(p.nodes)
        assert pl["levels"] == len(widths) == max(WR.node_levels(p.nodes)) + 1, t
        assert pl["fused_width"] >= 64 and pl["fused_width"] % 64 == 0, "whole wavefronts"
        assert pl["launches"] == WR.launches(p, [n_proofs], pl["fused_width"]), t
        assert pl["scratch_bytes"] == WR.scratch_bytes(p, n_proofs), t
        seen_depths.add(pl["levels"])
    assert len(seen_depths) > 20, "the DAGs must differ in depth"


def test_fusing_rule_at_the_width_boundaries(W):
    fw = W(4, 1).plan(1)["fused_width"]
    for widths in ([1, 63, 64, 65, fw - 1, fw, fw + 1, 4 * fw + 3], [fw + 1, 1, fw + 1, 1, 1, fw + 1], [fw] * 5, [fw + 1] * 5, [1] * 50):
        p = WC.widths_program(W, widths)
        p.expose(0)
        for n_proofs in (1, 2, 3):
            pl = p.plan(n_proofs)
            assert pl["launches"] == WR.launches(p, [n_proofs], fw), (widths, n_proofs)
    # a 3000-level chain is ONE launch (plus the gather), whatever its depth
    p = WC.chain_program(W, 3000)
    p.expose(len(p.nodes) - 1)
    pl = p.plan(3)
    assert pl["levels"] == 3001 and pl["launches"] == 2


def test_an_empty_program_and_null_outputs(W, pkg):
    p = W(3, 1)
    assert p.plan(5) == {"levels": 0, "launches": 0, "fused_width": p.plan(1)["fused_width"], "scratch_bytes": 256}
    d, keep = p.desc()
    assert pkg.lib().amdzk_witness_plan(C.byref(d), 1, None, None, None, None, None, 0) == 0


def refused(pkg, p, n_proofs=1, size=None, mutate=None):
    d, keep = p.desc(size=size)
    if mutate:
        mutate(d, keep)
    msg = C.create_string_buffer(200)
    rc = pkg.lib().amdzk_witness_plan(C.byref(d), n_proofs, None, None, None, None, msg, len(msg))
    return rc, msg.value.decode()


def small(W):
    p = W(3, 2)
    a, b = p.input(), p.input()
    c = p.const(5)
    s = p.add(a, b)
    m = p.mul(s, c)
    p.bits(m, 3, 8)
    p.assign(s, 0, 0)
    p.assign(m, 1, 7)
    p.expose(m)
    return p


def test_every_refusal_of_the_description(W, pkg):
    assert refused(pkg, small(W)) == (0, "")

    def case(build, code=E_INVALID, **kw):
        p = small(W)
        if build:
            build(p)
        rc, msg = refused(pkg, p, **kw)
        assert rc == code and msg.startswith("witness:"), (rc, msg)
        return msg

    # null description, too-small size
    msg = C.create_string_buffer(200)
    assert pkg.lib().amdzk_witness_plan(None, 1, None, None, None, None, msg, len(msg)) == E_INVALID and msg.value.startswith(b"witness:")
    case(None, size=C.sizeof(pkg.ffi.WitnessDesc) - 1)
    case(None, size=0)
    # null arrays with a count
    for field in ("constants", "nodes", "cells", "publics"):
        case(None, mutate=lambda d, keep, f=field: setattr(d, f, None))
    # unknown op
    case(lambda p: p.nodes.append((14, 0, 0, 0)))
    case(lambda p: p.nodes.append((0xFFFFFFFF, 0, 0, 0)))
    # an operand >= its own index: itself, a later node, for every operand position
    n = len(small(W).nodes)
    case(lambda p: p.nodes.append((WR.ADD, n, 0, 0)))
    case(lambda p: p.nodes.append((WR.ADD, 0, n + 5, 0)))
    case(lambda p: p.nodes.append((WR.SELECT, 0, 0, n)))
    case(lambda p: p.nodes.append((WR.NEG, 0xFFFFFFFF, 0, 0)))
    case(lambda p: p.nodes.insert(0, (WR.NEG, 0, 0, 0)))
    # input / constant index out of range
    case(lambda p: p.nodes.append((WR.INPUT, 2, 0, 0)))
    case(lambda p: p.nodes.append((WR.CONST, 1, 0, 0)))
    # a constant >= r: r itself and 2^256 - 1 (the builder reduces, so the words are written behind its back)
    for bad in (R, (1 << 256) - 1):
        def put(d, keep, bad=bad):
            keep[0][0] = WR.raw_words([bad])[0]
        case(None, mutate=put)
    # BITS
    for lo, ln in ((0, 0), (0, 257), (1, 256), (255, 2), (256, 1), (0xFFFFFFFF, 2), (2, 0xFFFFFFFF)):
        case(lambda p, lo=lo, ln=ln: p.bits(0, lo, ln))
    # cells
    case(lambda p: p.assign(0, 2, 0))
    case(lambda p: p.assign(0, 0, 8))
    case(lambda p: p.assign(len(p.nodes), 0, 1))
    assert "twice" in case(lambda p: p.assign(1, 1, 7))
    # publics
    case(lambda p: p.expose(len(p.nodes)))
    # n_proofs = 0
    case(None, n_proofs=0)
    # sizes whose workspace arithmetic would overflow
    case(None, code=E_UNSUPPORTED, n_proofs=(1 << 64) - 1)
    case(None, code=E_UNSUPPORTED, n_proofs=1 << 60)


def test_more_than_the_default_workspace_is_cut_into_equal_runs(W):
    """16 GiB by default: a program of 2^20 nodes takes 32 MiB a proof, so 1000 proofs go as 2 runs of 500."""
    p = W(3, 1)
    x = p.input()
    nodes = np.zeros((1 << 20, 4), dtype=np.uint32)
    nodes[1:, 0] = WR.NEG  # node i = -node 0: one wide level
    p.nodes = [tuple(r) for r in nodes.tolist()]
    p.expose(x)
    pl = p.plan(1000)
    fit = ((16 << 30) - 256) // (((1 << 20) + 1) * 32)
    runs = WR.run_cut(1000, fit)
    assert len(runs) == 2 and runs == [500, 500]
    assert pl["scratch_bytes"] == WR.scratch_bytes(p, 500)
    assert pl["launches"] == WR.launches(p, runs, pl["fused_width"]) == 2 * 3
