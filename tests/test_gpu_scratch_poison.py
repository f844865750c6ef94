"""GPU: no result depends on what a workspace held before (csrc/workspace.hpp, WHAT CHECKS THE RULES).

A context created with AMDZK_WS_POISON=1 fills every reservation of scratch memory — the context's slots and pinned buffer,
the per-proof arenas of a key handle, the private buffers of the witness-program and Poseidon handles — with the 32-bit word
5 before its user gets it. A region read before it is written, an outer user that reads its region after an inner call
reserved the slot again, or a call that counts on what the last call left on a handle then computes a wrong answer. So on
such a context every entry point must still equal its reference EXACTLY.

The comparison tests do not restate references: each runs the body of the existing test of its entry point — the same
case builders, the same oracle, the same assertions — with the poisoned context in place of the session's `ctx`, and with
that module's own ctx-dependent fixtures (keys, rigs, parameters) rebuilt on the poisoned context (class Existing). The shapes
are therefore THE EXISTING TESTS' shapes: where a test is parametrised, the parameter nearest the smallest shape that reaches
the scratch in question (or one its body takes unchanged, such as k = 19 for the NTT); where it is not, whatever it uses —
the prefix-sum basis at k = 5, g_to_lagrange, downsize and write / read at test_gpu_msm's sizes, the pointer-table MSM at
k = 6, seven columns in the batch over caller-supplied bases, 35 ragged Poseidon lengths. Each reaches the same slot and the
same code path as a hand-picked shape would. The oracle's results are cached per process by the case modules, so they are
computed once.
Existing reads pytest's fixture definitions through attributes pytest does not document; a fixture it does not recognise
raises (request.getfixturevalue of an unknown name) instead of falling back to the session context.

The order tests run sequences the suite's incidental order may never produce — large, small, large in one slot; one key
handle under proofs and checks of different instance lengths; one Poseidon and one witness handle under calls of
different sizes — every result against the reference, never against an earlier result.
"""
import contextlib
import importlib
import inspect
import os

import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu
ENV = "AMDZK_WS_POISON"


def _fixture_parts(obj):
    """(function, scope) of a pytest fixture definition, None for anything else."""
    marker = getattr(obj, "_fixture_function_marker", None) or getattr(obj, "_pytestfixturefunction", None)
    if marker is None:
        return None
    fn = getattr(obj, "_fixture_function", None) or getattr(getattr(obj, "__pytest_wrapped__", None), "obj", None) or getattr(obj, "__wrapped__", None)
    return (fn, marker.scope) if callable(fn) else None


class Existing:
    """Runs test functions of other modules of this suite on ONE context. An argument is, in this order: a parameter the
    caller gives; `ctx`: the context; a fixture the test's module defines: that fixture's function, called with arguments
    resolved the same way (module-scoped: once per module, torn down by close(); function-scoped: per run); anything else
    (pkg, oracle, monkeypatch, tmp_path): the running test's own fixture."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.made = {}
        self.module_scope = contextlib.ExitStack()

    def _value(self, request, mod, name, per_run):
        if name == "ctx":
            return self.ctx
        parts = _fixture_parts(getattr(mod, name, None))
        if parts is None:
            return request.getfixturevalue(name)
        fn, scope = parts
        shared = scope != "function"
        cache, stack = (self.made, self.module_scope) if shared else per_run
        key = (mod.__name__, name)
        if key not in cache:
            args = {a: self._value(request, mod, a, per_run) for a in inspect.signature(fn).parameters}
            out = fn(**args)
            if inspect.isgenerator(out):
                gen, out = out, next(out)
                stack.callback(lambda g=gen: next(g, None))
            cache[key] = out
        return cache[key]

    def run(self, request, module, test, **params):
        mod = importlib.import_module(module)
        fn = getattr(mod, test)
        with contextlib.ExitStack() as run_scope:
            per_run = ({}, run_scope)
            args = {a: params[a] if a in params else self._value(request, mod, a, per_run) for a in inspect.signature(fn).parameters}
            assert set(params) <= set(args), "%s.%s takes no %s" % (module, test, sorted(set(params) - set(args)))
            fn(**args)

    def close(self):
        self.module_scope.close()


def poisoned_context(pkg, on=True):
    """A context created with (on) or without the variable; the environment is as it was when this returns."""
    before = os.environ.get(ENV)
    try:
        if on:
            os.environ[ENV] = "1"
        else:
            os.environ.pop(ENV, None)
        return pkg.Context(0)
    finally:
        if before is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = before


@pytest.fixture(scope="module")
def poisoned(pkg):
    ctx = poisoned_context(pkg)
    world = Existing(ctx)
    yield world
    world.close()
    ctx.close()


def fills(ctx):
    return ctx.prof_dump().get("ws_poison", (0, 0.0))[0]


@contextlib.contextmanager
def counting(ctx):
    ctx.prof_enable(True)
    ctx.prof_reset()
    try:
        yield
    finally:
        ctx.prof_enable(False)
        ctx.prof_reset()


# ---------------------------------------------------------------------------------------------- the switch itself
def scratch_users(pkg, oracle, ctx):
    """One call per kind of scratch, each returning its result: a two-step NTT (ZK_WS_NTT and, for the host form,
    ZK_WS_STAGING), a table MSM (ZK_WS_MSM, the pinned buffer), a batch inversion (ZK_WS_CALLS)."""
    k = 11
    a = zu.random_fr(1 << k, seed=100 + k)
    w = oracle.omega(k)
    yield "ntt", lambda: pkg.arithmetic.best_fft(ctx, a.copy(), w, k), lambda got: np.array_equal(got, oracle.best_fft(a.copy(), w, k))
    g = oracle.srs_powers(zu.fr_from_int(7777), 1 << 6)
    params = pkg.kzg.ParamsKZG(ctx, 6, g=g)
    s = zu.random_fr(1 << 6, seed=12)
    yield "msm", lambda: params.commit(s), lambda got: np.array_equal(zu.jac_to_affine_host(oracle, got), oracle.best_multiexp(s, g))
    params.free()
    b = zu.random_fr(129, seed=5)
    yield "batch_invert", lambda: pkg.arithmetic.batch_invert(ctx, b), lambda got: np.array_equal(got, oracle.batch_invert(b))


def test_a_context_created_without_the_variable_never_fills(pkg, oracle):
    ctx = poisoned_context(pkg, on=False)
    try:
        with counting(ctx):
            for name, call, right in scratch_users(pkg, oracle, ctx):
                assert right(call()), name
                assert "ws_poison" not in ctx.prof_dump(), name
    finally:
        ctx.close()


def test_a_poisoned_context_fills_at_least_once_per_call_that_uses_scratch(poisoned, pkg, oracle):
    ctx = poisoned.ctx
    with counting(ctx):
        for name, call, right in scratch_users(pkg, oracle, ctx):
            before = fills(ctx)
            assert right(call()), name
            assert fills(ctx) > before, "%s reserved scratch and nothing was filled" % name


def test_the_environment_is_as_it_was_and_the_session_context_follows_it(poisoned, ctx, pkg, oracle):
    """The module's fixture leaves the variable as it found it, so the session context of every other test is poisoned exactly
    when the whole suite is run under the switch."""
    expected = int(os.environ.get(ENV) or 0) != 0
    with counting(ctx):
        for name, call, right in scratch_users(pkg, oracle, ctx):
            assert right(call()), name
        assert ("ws_poison" in ctx.prof_dump()) == expected


def test_key_handles_witness_programs_and_poseidon_handles_fill_their_own_buffers(poisoned, pkg, oracle, request):
    """With per-kernel profiling on a proof runs on one stream, so every fill of a proof is counted on the context: a proof
    fills its handle's arenas (more than twenty buffers), a check fills them again, a witness run and a hash fill theirs."""
    ctx = poisoned.ctx
    with counting(ctx):
        poisoned.run(request, "test_gpu_check_witness", "test_checks_between_proofs_change_no_proof")
        assert fills(ctx) > 5 * 20, "three proofs and two checks on one handle"
    with counting(ctx):
        poisoned.run(request, "test_gpu_witness", "test_cells_stride_sentinel_and_zero_fill")
        assert fills(ctx) >= 2, "two runs"
    import poseidon_cases as PC
    import poseidon_ref as PR
    spec = PC.spec(3, 2, 2, 1, "random")
    P = pkg.poseidon.Poseidon(ctx, PC.pkg_spec(pkg, spec))
    try:
        with counting(ctx):
            x = PC.inputs(5, "poison-fill", edge=True)
            assert np.array_equal(P.hash_many([PC.to_words(x)]), PC.to_words([PR.sponge(spec, x)]))
            assert fills(ctx) >= 3, "the lengths, the staged inputs, the digests"
    finally:
        P.free()


# ---------------------------------------------------------------------------------------------- comparison tests
# (module, test, parameters): the existing test's body on the poisoned context. See the module's docstring.
A_CASES = {
    # NTT: k = 11 is the first two-step plan, k = 19 the first three-step plan (ZK_WS_NTT); 5 resident columns, stride n + 64
    "ntt k11": ("test_gpu_ntt", "test_ntt_matches_oracle", dict(k=11)),
    "ntt k19": ("test_gpu_ntt", "test_ntt_matches_oracle", dict(k=19)),
    "ntt 5 columns k14 strided": ("test_gpu_ntt", "test_ntt_batch_device_columns", {}),
    "domain j4 k9": ("test_gpu_domain", "test_domain_matches_oracle", dict(j=4, k=9)),
    # table MSM cut into runs by max_scratch_bytes (5 columns through a pointer table)
    "msm cols_dev in runs": ("test_gpu_batch", "test_pointer_table_msm_equals_the_strided_msm", dict(k=6)),
    # MSM over caller-supplied bases: either side of the window-width cut at 2^12 points, and a batch
    "msm bases n1000": ("test_gpu_msm_bases", "test_bases_uniform_matches_oracle", dict(n=1000)),
    "msm bases n5000": ("test_gpu_msm_bases", "test_bases_uniform_matches_oracle", dict(n=5000)),
    "msm bases batch": ("test_gpu_msm_bases", "test_bases_batch_columns_host_and_resident", {}),
    # host-pointer forms that stage through ZK_WS_STAGING
    "ntt_fr_batch": ("test_gpu_abi_entry_points", "test_ntt_batch_of_host_columns", dict(k=11, scale=True)),
    "msm_g1_batch": ("test_gpu_msm", "test_msm_batch_columns", {}),
    # SRS unit (ZK_WS_STARTUP; the check crosses STARTUP and STAGING)
    "srs setup k6": ("test_gpu_srs_unit", "test_setup_matches_oracle", dict(k=6, name="r_minus_2")),
    "srs g_to_lagrange": ("test_gpu_msm", "test_g_to_lagrange_matches_oracle", {}),
    "srs g_to_lagrange degenerate": ("test_gpu_srs_unit", "test_g_to_lagrange_all_equal_and_all_identity", {}),
    "srs downsize": ("test_gpu_msm", "test_params_downsize", {}),
    "srs write read": ("test_gpu_msm", "test_params_write_read_roundtrip", {}),
    "srs prefix basis k5": ("test_gpu_srs_unit", "test_prefix_sums_over_a_chosen_basis", dict(k=5)),
    "srs check honest k6": ("test_gpu_srs_check", "test_an_honest_srs_passes_every_check", dict(k=6)),
    "srs check swapped k6": ("test_gpu_srs_check", "test_two_swapped_entries_fail_the_check_that_reads_them", dict(k=6)),
    # opening kernels (ZK_WS_OPENING, ZK_WS_TABLES)
    "eval_poly n70000": ("test_gpu_plonk_ops", "test_eval_polynomial", dict(n=70000)),
    "poly_axpy 300x513": ("test_gpu_plonk_ops", "test_poly_axpy", dict(m=300, n=513)),
    "lincomb of no terms": ("test_gpu_plonk_operands", "test_lincomb_of_no_terms", {}),
    "kate_div n6000": ("test_gpu_plonk_ops", "test_kate_division", dict(n=6000)),
    "multiopen shared shplonk": ("test_gpu_multiopen", "test_points_and_transcript_equal_oracle", dict(name="shared", scheme="shplonk")),
    "multiopen shared gwc": ("test_gpu_multiopen", "test_points_and_transcript_equal_oracle", dict(name="shared", scheme="gwc")),
    "multiopen 17 sets shplonk": ("test_gpu_multiopen", "test_points_and_transcript_equal_oracle", dict(name="17 sets", scheme="shplonk")),
    "multiopen verify shared shplonk": ("test_gpu_multiopen_verify", "test_pair_equals_the_reference_and_only_the_oracles_opening_is_decided_valid", dict(name="shared", scheme="shplonk")),
    "multiopen verify shared gwc": ("test_gpu_multiopen_verify", "test_pair_equals_the_reference_and_only_the_oracles_opening_is_decided_valid", dict(name="shared", scheme="gwc")),
    "multiopen verify 17 sets shplonk": ("test_gpu_multiopen_verify", "test_pair_equals_the_reference_and_only_the_oracles_opening_is_decided_valid", dict(name="17 sets", scheme="shplonk")),
    "multiopen verify 17 sets gwc": ("test_gpu_multiopen_verify", "test_pair_equals_the_reference_and_only_the_oracles_opening_is_decided_valid", dict(name="17 sets", scheme="gwc")),
    "multiopen dev then decide shared gwc": ("test_gpu_multiopen_verify", "test_multiopen_dev_then_multiopen_decide_round_trips", dict(name="shared", scheme="gwc")),
    "multiopen dev then decide 17 sets shplonk": ("test_gpu_multiopen_verify", "test_multiopen_dev_then_multiopen_decide_round_trips", dict(name="17 sets", scheme="shplonk")),
    # PLONK-layer calls (ZK_WS_CALLS, ZK_WS_PERMUTE, the key's arenas)
    "batch_invert 4097": ("test_gpu_plonk_ops", "test_batch_invert", dict(n=4097)),
    "batch_invert_assigned 4097": ("test_gpu_plonk_ops", "test_batch_invert_assigned", dict(n=4097)),
    "grand_product 5000x3 chained": ("test_gpu_plonk_ops", "test_grand_product_plain_and_chained", dict(n=5000, ncols=3)),
    "permute pair n4096": ("test_gpu_plonk_ops", "test_permute_expression_pair_around_the_sort_tile", dict(n=4096)),
    "permute pair n8192": ("test_gpu_plonk_ops", "test_permute_expression_pair_around_the_sort_tile", dict(n=8192)),
    "quotient_eval both coset modes": ("test_gpu_quotient_operands", "test_quotient_pieces_equal_the_oracle_in_both_coset_modes",
                                       dict(name="lookup5", polyset="arbitrary0", chal="tbg_random.y_random")),
    # keys and proofs, byte-equal to the oracle
    "proof lookup k5": ("test_gpu_prover", "test_proof_bytes_equal_oracle", dict(name="lookup", k=5)),
    "proof rsa_sha256 small": ("test_gpu_prover", "test_rsa_sha256_shape_small_equals_oracle", {}),
    "proof high degree, generic recombination": ("test_gpu_prover", "test_high_degree_gate_bytes_equal_oracle", dict(power=9, flags=0)),
    "proof phased k5": ("test_gpu_phased", "test_phased_proof_bytes_equal_the_harness", dict(k=5)),
    "create_proof_multi N2": ("test_gpu_prover", "test_several_circuit_instances_in_one_proof", dict(k=7, ncirc=2, transcript="blake2b")),
    "create_proof_batch N3": ("test_gpu_batch", "test_three_witnesses_of_one_layout", dict(transcript="blake2b")),
    "create_proof_batch_opts two circuits": ("test_gpu_batch_opts", "test_mixed_circuits_on_one_srs", {}),
    # verification: three cases through the proving-key route, the verifying-key route and the mixed route
    "verify pk square": ("test_gpu_verify", "test_accepted_proofs_give_the_reference_pair", dict(name="square", N=1, transcript="blake2b", multiopen="shplonk")),
    "verify pk lookup x2 evm gwc": ("test_gpu_verify", "test_accepted_proofs_give_the_reference_pair", dict(name="lookup", N=2, transcript="evm", multiopen="gwc")),
    "verify pk rlc gwc": ("test_gpu_verify", "test_accepted_proofs_give_the_reference_pair", dict(name="rlc", N=1, transcript="blake2b", multiopen="gwc")),
    "decide pk square": ("test_gpu_verify_decide", "test_the_devices_valid_proof_is_decided_valid", dict(name="square", N=1, transcript="blake2b", multiopen="shplonk")),
    "decide pk lookup x2 evm gwc": ("test_gpu_verify_decide", "test_the_devices_valid_proof_is_decided_valid", dict(name="lookup", N=2, transcript="evm", multiopen="gwc")),
    "decide pk rlc gwc": ("test_gpu_verify_decide", "test_the_devices_valid_proof_is_decided_valid", dict(name="rlc", N=1, transcript="blake2b", multiopen="gwc")),
    "verify and decide vk square": ("test_gpu_vk", "test_every_case_verifies_the_same_without_the_proving_key_and_the_srs", dict(name="square", N=1, transcript="blake2b", multiopen="shplonk")),
    "verify and decide vk lookup x2 evm gwc": ("test_gpu_vk", "test_every_case_verifies_the_same_without_the_proving_key_and_the_srs", dict(name="lookup", N=2, transcript="evm", multiopen="gwc")),
    "verify and decide vk rlc gwc": ("test_gpu_vk", "test_every_case_verifies_the_same_without_the_proving_key_and_the_srs", dict(name="rlc", N=1, transcript="blake2b", multiopen="gwc")),
    "verify and decide mixed": ("test_gpu_verify_mixed", "test_mixed_batches_in_several_orders", {}),
    # witness programs: the 300-node program at 5 proofs in runs of 5, 2 + 2 + 1 and 1 x 5; run_dev; ZERO_FILL on and off
    "witness bounded workspace": ("test_gpu_witness", "test_a_bounded_workspace_cuts_the_batch_and_changes_nothing", {}),
    "witness run_dev": ("test_gpu_witness", "test_dev_form_equals_host_form_and_refuses_a_resident_input_above_the_modulus", {}),
    "witness zero fill": ("test_gpu_witness", "test_cells_stride_sentinel_and_zero_fill", {}),
    # Poseidon: 35 ragged sponges, host and resident; 33 states
    "poseidon hash and hash_dev ragged": ("test_gpu_poseidon", "test_sponge_rates_and_lengths_uniform_ragged_host_and_resident", dict(t=3, init=False)),
    "poseidon permute_dev 33 states": ("test_gpu_poseidon", "test_permutation_with_a_stride_leaves_the_gaps", dict(t=5)),
}


@pytest.mark.parametrize("case", sorted(A_CASES), ids=[c.replace(" ", "_") for c in sorted(A_CASES)])
def test_the_existing_test_of_the_entry_point_passes_on_a_poisoned_context(poisoned, request, case):
    module, test, params = A_CASES[case]
    poisoned.run(request, module, test, **params)


def test_multiopen_dev_on_17_sets_under_gwc(poisoned, request, pkg, oracle):
    """(The existing test of this case asserts SHPLONK's set count on the way: its comparison alone, under GWC.)"""
    M = importlib.import_module("test_gpu_multiopen")
    case, want = M.make_case("17 sets"), M.oracle_of("17 sets", "gwc")
    params_of = poisoned._value(request, M, "params_of", None)
    got = M.run_device(poisoned.ctx, pkg, oracle, params_of(case.k), case, "gwc")
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]


@pytest.mark.parametrize("m", ["m1", "m2", "m3"])
def test_pairing_products(poisoned, request, m):
    P = importlib.import_module("test_gpu_pairing")
    checks = {"m1": [[P.A1], [None]], "m2": [[P.A1, None], [None, P.A2]], "m3": [[None, P.A1, P.A2], [P.A1, None, P.A2], [P.A1, P.A2, None]]}[m]
    poisoned.run(request, "test_gpu_pairing", "test_gt_equals_the_reference_limb_for_limb", checks=checks)


@pytest.mark.parametrize("length", [1000, 1024])
def test_table_msm_at_k10_both_bases(poisoned, pkg, oracle, length):
    M = importlib.import_module("test_gpu_msm")
    n = 1 << 10
    srs = oracle.srs_powers(zu.fr_from_int(0xABCDEF12345), 2 * n)
    params = pkg.kzg.ParamsKZG(poisoned.ctx, 10, g=srs[:n].copy(), g_lagrange=srs[n:].copy())
    try:
        for basis in (0, 1):
            M.check(poisoned.ctx, pkg, oracle, params, srs[basis * n:], zu.random_fr(length, seed=40 + length + basis), basis=basis)
    finally:
        params.free()


# ---------------------------------------------------------------------------------------------- order tests
def in_order(poisoned, request, steps):
    for module, test, params in steps:
        poisoned.run(request, module, test, **params)


def test_ntt_large_small_large_in_one_slot(poisoned, request):
    big = ("test_gpu_ntt", "test_ntt_batch_device_columns", {})  # k = 14, five columns
    in_order(poisoned, request, [big, ("test_gpu_ntt", "test_ntt_matches_oracle", dict(k=11)), big])


def test_table_msm_large_small_large_in_one_slot(poisoned, request, pkg, oracle):
    M = importlib.import_module("test_gpu_msm")
    big = ("test_gpu_msm", "test_msm_batch_columns", {})  # k = 12, seven columns
    poisoned.run(request, *big[:2])
    srs = oracle.srs_powers(zu.fr_from_int(0xABCDEF12345), 1 << 12)
    params = pkg.kzg.ParamsKZG(poisoned.ctx, 12, g=srs.copy())
    try:
        M.check(poisoned.ctx, pkg, oracle, params, srs, zu.random_fr(3, seed=4))
    finally:
        params.free()
    poisoned.run(request, *big[:2])


def test_eval_poly_large_small_large_in_one_slot(poisoned, request):
    big = ("test_gpu_plonk_ops", "test_eval_polynomial", dict(n=70000))
    in_order(poisoned, request, [big, ("test_gpu_plonk_ops", "test_eval_polynomial", dict(n=2)), big])


def test_permute_expression_pair_large_small_large_in_one_slot(poisoned, request):
    big = ("test_gpu_plonk_ops", "test_permute_expression_pair_around_the_sort_tile", dict(n=8192))
    in_order(poisoned, request, [big, ("test_gpu_plonk_ops", "test_permute_expression_pair", dict(name="many_leftovers")), big])  # n = 64


@pytest.mark.parametrize("handle", ["key", "clone"])
def test_one_key_handle_under_proofs_and_checks_of_different_instance_lengths(poisoned, pkg, oracle, handle):
    """SquareCircuit's instance column is absorbed by the transcript and not constrained. Proof A: an instance column at full
    usable length; B: three values and another witness; A again; check_witness between and after them (the prover and the
    check share the handle's arenas, and each zeroes inst() on its own)."""
    import circuits
    import plonk_ref as PR
    import witness_check_ref as W

    K = importlib.import_module("test_gpu_check_witness")
    ctx = poisoned.ctx
    plonk = importlib.import_module("anon_aadhaar_halo2_amd.halo2.plonk")
    ca, cb = circuits.square_circuit(plonk, 4, signal=5), circuits.square_circuit(plonk, 4, signal=11)
    inst_a = [[(7 * i + 25) % zu.R for i in range(ca.usable)]]
    inst_b = [[121, 0, 7]]
    params = pkg.kzg.ParamsKZG.setup(ctx, ca.k, zu.fr_from_int(K.TAU))
    root = plonk.ProvingKey(ctx, params, ca.desc, K.fr_cols(oracle, ca.fixed, ca.n), ca.assembly.mapping, zu.fr_from_int(K.REPR))
    pk = root.clone_workspace() if handle == "clone" else root
    opk = PR.keygen(ca.desc, ca.fixed, ca.assembly.mapping, K.TAU, transcript_repr=K.REPR)
    d = {id(c): ctx.alloc(len(c.advice) * c.n * 32).upload(K.fr_cols(oracle, c.advice, c.n)) for c in (ca, cb)}

    def prove(c, inst, seed):
        assert plonk.create_proof(ctx, pk, K.fr_inst(oracle, inst), d[id(c)], seed=seed) == PR.create_proof(opk, inst, c.advice, seed=seed)

    def check(c, inst, advice=None):
        dev = d[id(c)] if advice is None else ctx.alloc(len(advice) * c.n * 32).upload(K.fr_cols(oracle, advice, c.n))
        rep = plonk.check_witness(ctx, pk, K.fr_inst(oracle, inst), dev)
        assert [tuple(f) for f in rep.failures] == W.report(c, advice=advice, instances=inst)
        if advice is not None:
            dev.free()
        return rep

    try:
        prove(ca, inst_a, 3)
        assert check(ca, inst_a).ok
        prove(cb, inst_b, 4)
        bad = [list(col) for col in cb.advice]
        bad[1][0] = (bad[1][0] + 1) % zu.R
        assert not check(cb, inst_b, advice=bad).ok
        prove(ca, inst_a, 3)
        assert check(cb, inst_b).ok
        prove(cb, [[]], 5)
    finally:
        for b in d.values():
            b.free()
        if pk is not root:
            pk.free()
        root.free()
        params.free()


def test_one_poseidon_handle_long_short_long(poisoned, pkg):
    """33 sponges of up to 40 inputs, then three of 0, 1 and 2 (the staged inputs keep the earlier stride's leftovers), then
    the 33 again."""
    import poseidon_cases as PC
    import poseidon_ref as PR

    spec = PC.spec(3, 2, 2, 1, "random")
    P = pkg.poseidon.Poseidon(poisoned.ctx, PC.pkg_spec(pkg, spec))
    long_ = [PC.inputs((7 * i + 3) % 41, "poison%d" % i, edge=True) for i in range(33)]
    short = [PC.inputs(n, "poison-short%d" % n, edge=True) for n in (0, 1, 2)]
    assert max(len(x) for x in long_) == 40
    want = {id(s): PC.to_words([PR.sponge(spec, x) for x in s]) for s in (long_, short)}
    try:
        for data in (long_, short, long_):
            assert np.array_equal(P.hash_many([PC.to_words(x) for x in data]), want[id(data)]), len(data)
    finally:
        P.free()


def test_one_witness_handle_65_proofs_then_1_then_3_in_single_proof_runs(poisoned, request):
    T = importlib.import_module("test_gpu_witness")
    prog, inputs, want = poisoned._value(request, T, "batch_case", None)
    per_proof = (len(prog.nodes) + len(prog.publics)) * 32
    cw = prog.compile(poisoned.ctx)
    try:
        for n, bound in ((65, 0), (1, 0), (3, per_proof + 256)):
            got = T.run_host(poisoned.ctx, cw, prog, inputs[:n], max_scratch_bytes=bound)
            assert np.array_equal(got, want[:n]), (n, bound)
    finally:
        cw.free()
