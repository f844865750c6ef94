"""ctypes binding of include/amdzk.h. One `Context` = one amdzk_ctx (one GPU, one host thread)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class AmdzkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("amdzk error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    return os.path.join(_HERE, "libamdzk.so")


def lib():
    """Load libamdzk.so (built in-tree by __graft_entry__.build()). Fails loudly if missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise AmdzkError(-1, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % p)
    L = C.CDLL(p)
    vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
    sig = {
        "amdzk_version": (i32, []),
        "amdzk_build_info": (C.c_char_p, []),
        "amdzk_init": (i32, [i32, C.POINTER(vp)]),
        "amdzk_destroy": (None, [vp]),
        "amdzk_last_error": (C.c_char_p, [vp]),
        "amdzk_set_stream": (i32, [vp, vp]),
        "amdzk_sync": (i32, [vp]),
        "amdzk_ctx_device": (i32, [vp]),
        "amdzk_ctx_check_affinity": (i32, [vp]),
        "amdzk_ptr_check_affinity": (i32, [vp, vp]),
        "amdzk_pk_check_affinity": (i32, [vp, vp]),
        "amdzk_dev_alloc": (i32, [vp, sz, C.POINTER(vp)]),
        "amdzk_dev_free": (i32, [vp, vp]),
        "amdzk_dev_upload": (i32, [vp, vp, vp, sz]),
        "amdzk_dev_download": (i32, [vp, vp, vp, sz]),
        "amdzk_dev_memset": (i32, [vp, vp, i32, sz]),
        "amdzk_host_alloc": (i32, [vp, sz, C.POINTER(vp)]),
        "amdzk_host_free": (i32, [vp, vp]),
        "amdzk_dev_upload_async": (i32, [vp, vp, vp, sz]),
        "amdzk_upload_fence": (i32, [vp]),
        "amdzk_srs_upload": (i32, [vp, vp, vp, u32, C.POINTER(vp)]),
        "amdzk_srs_setup": (i32, [vp, u32, vp, C.POINTER(vp), vp, vp]),
        "amdzk_srs_serialized_size": (sz, [u32]),
        "amdzk_srs_write": (i32, [vp, vp, vp, vp, vp, sz]),
        "amdzk_srs_read": (i32, [vp, vp, sz, C.POINTER(vp), vp, vp]),
        "amdzk_srs_free": (None, [vp, vp]),
        "amdzk_srs_downsize": (i32, [vp, vp, u32, C.POINTER(vp)]),
        "amdzk_srs_get": (i32, [vp, vp, i32, vp]),
        "amdzk_g_to_lagrange": (i32, [vp, vp, u32, vp]),
        "amdzk_msm_g1": (i32, [vp, vp, i32, vp, sz, vp]),
        "amdzk_msm_g1_batch": (i32, [vp, vp, i32, C.POINTER(vp), sz, sz, vp]),
        "amdzk_msm_g1_dev": (i32, [vp, vp, i32, vp, sz, sz, sz, vp]),
        "amdzk_msm_g1_cols_dev": (i32, [vp, vp, i32, C.POINTER(vp), sz, sz, sz, vp]),
        "amdzk_msm_g1_bases": (i32, [vp, vp, vp, sz, vp]),
        "amdzk_msm_g1_bases_batch": (i32, [vp, C.POINTER(vp), sz, vp, sz, vp]),
        "amdzk_msm_g1_bases_dev": (i32, [vp, vp, sz, sz, sz, vp, vp]),
        "amdzk_msm_g1_bases_plan": (i32, [sz, sz, C.POINTER(u32), C.POINTER(u32), C.POINTER(sz)]),
        "amdzk_ntt_fr": (i32, [vp, vp, u32, vp, u32]),
        "amdzk_ntt_fr_dev": (i32, [vp, vp, u32, vp, u32, sz, sz]),
        "amdzk_fr_from_raw_dev": (i32, [vp, vp, sz]),
        "amdzk_fr_to_repr_dev": (i32, [vp, vp, sz]),
        "amdzk_domain_new": (i32, [vp, u32, u32, C.POINTER(vp)]),
        "amdzk_domain_free": (None, [vp, vp]),
        "amdzk_domain_k": (u32, [vp]),
        "amdzk_domain_extended_k": (u32, [vp]),
        "amdzk_domain_constant": (i32, [vp, i32, vp]),
        "amdzk_lagrange_to_coeff_dev": (i32, [vp, vp, vp, sz, sz]),
        "amdzk_coeff_to_lagrange_dev": (i32, [vp, vp, vp, sz, sz]),
        "amdzk_coeff_to_extended_dev": (i32, [vp, vp, vp, sz, vp, sz, sz]),
        "amdzk_extended_to_coeff_dev": (i32, [vp, vp, vp, sz, sz]),
        "amdzk_divide_by_vanishing_dev": (i32, [vp, vp, vp, sz, sz]),
        "amdzk_set_host_wait": (i32, [vp, i32]),
        "amdzk_keygen": (i32, [vp, vp, vp, vp, vp, vp, C.POINTER(vp)]),
        "amdzk_keygen_ex": (i32, [vp, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
        "amdzk_keygen_phased": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
        "amdzk_keygen_sigma": (i32, [vp, vp, vp, vp, vp, vp, vp, u32, C.POINTER(vp)]),
        "amdzk_pk_export": (i32, [vp, vp, i32, vp, sz, C.POINTER(sz)]),
        "amdzk_pk_serialized_size": (sz, [vp]),
        "amdzk_pk_write": (i32, [vp, vp, vp, sz, C.POINTER(sz)]),
        "amdzk_pk_read": (i32, [vp, vp, vp, sz, u32, C.POINTER(vp)]),
        "amdzk_pk_blob_info": (i32, [vp, sz, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "amdzk_pk_blob_check": (i32, [vp, sz, vp, sz]),
        "amdzk_pk_free": (None, [vp, vp]),
        "amdzk_pk_commitments": (i32, [vp, vp, vp]),
        "amdzk_create_proof": (i32, [vp, vp, C.POINTER(vp), C.POINTER(sz), vp, sz, C.c_uint64, vp, sz, C.POINTER(sz)]),
        "amdzk_create_proof_ex": (i32, [vp, vp, C.POINTER(vp), C.POINTER(sz), vp, sz, C.c_uint64, i32, vp, sz, C.POINTER(sz)]),
        "amdzk_pk_clone_workspace": (i32, [vp, vp, C.POINTER(vp)]),
        "amdzk_create_proof_multi": (i32, [vp, C.POINTER(vp), sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), sz, C.c_uint64, i32,
                                           vp, sz, C.POINTER(sz)]),
        "amdzk_create_proof_opts": (i32, [vp, C.POINTER(vp), sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), sz, vp,
                                          vp, sz, C.POINTER(sz)]),
        "amdzk_create_proof_batch": (i32, [vp, C.POINTER(vp), sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), sz, vp,
                                           vp, sz, C.POINTER(sz), C.POINTER(i32)]),
        "amdzk_create_proof_batch_opts": (i32, [vp, C.POINTER(vp), sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), sz, vp,
                                                vp, sz, C.POINTER(sz), C.POINTER(i32)]),
        "amdzk_proof_size_multi": (sz, [vp, sz, i32]),
        "amdzk_proof_random_count": (sz, [vp]),
        "amdzk_proof_size": (sz, [vp, i32]),
        "amdzk_create_proof_scalars": (i32, [vp, vp, C.POINTER(vp), C.POINTER(sz), vp, sz, vp, sz, i32, vp, sz, C.POINTER(sz)]),
        "amdzk_ntt_fr_batch": (i32, [vp, C.POINTER(vp), sz, u32, vp, u32]),
        "amdzk_batch_invert_dev": (i32, [vp, vp, sz]),
        "amdzk_batch_invert_assigned_dev": (i32, [vp, vp, vp, sz, vp]),
        "amdzk_grand_product_dev": (i32, [vp, vp, sz, sz, sz, i32, sz]),
        "amdzk_perm_products_dev": (i32, [vp, vp, vp, vp, i32, vp, C.POINTER(sz), C.POINTER(i32)]),
        "amdzk_eval_poly_dev": (i32, [vp, C.POINTER(vp), vp, sz, u32, vp]),
        "amdzk_poly_axpy_dev": (i32, [vp, C.POINTER(vp), vp, sz, vp, sz, i32]),
        "amdzk_kate_div_dev": (i32, [vp, C.POINTER(vp), vp, sz, u32]),
        "amdzk_multiopen_dev": (i32, [vp, vp, C.POINTER(vp), sz, vp, sz, vp, sz, vp, vp, sz, C.POINTER(sz)]),
        "amdzk_multiopen_plan": (i32, [vp, sz, vp, sz, sz, u32, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(sz), vp]),
        "amdzk_permute_expression_pair_dev": (i32, [vp, vp, vp, vp, sz, u32, u32]),
        "amdzk_quotient_eval_dev": (i32, [vp, vp, vp, sz, vp, vp, vp, vp, vp]),
        "amdzk_pk_inspect": (i32, [vp, vp, i32, vp, sz, C.POINTER(sz)]),
        "amdzk_check_witness": (i32, [vp, vp, C.POINTER(vp), C.POINTER(sz), vp, sz, vp, vp, sz, C.POINTER(sz)]),
        "amdzk_verify_proofs": (i32, [vp, vp, sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), C.POINTER(sz), vp, vp, vp]),
        "amdzk_g2_prepare": (i32, [vp, vp, C.POINTER(vp)]),
        "amdzk_g2_free": (None, [vp, vp]),
        "amdzk_g2_setup": (i32, [vp, vp, vp, vp]),
        "amdzk_g2_compress": (i32, [vp, vp, vp, sz]),
        "amdzk_g2_decompress": (i32, [vp, vp, vp, sz]),
        "amdzk_g2_check": (i32, [vp, C.POINTER(i32)]),
        "amdzk_pairing_products": (i32, [vp, C.POINTER(vp), sz, vp, sz, vp, vp]),
        "amdzk_srs_check": (i32, [vp, vp, vp, vp, vp, vp]),
        "amdzk_verify_proofs_decide": (i32, [vp, vp, vp, vp, u32, sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), C.POINTER(sz),
                                             vp, vp, vp, C.POINTER(sz)]),
        "amdzk_multiopen_verify": (i32, [vp, vp, vp, sz, vp, sz, vp, vp, sz, vp, vp]),
        "amdzk_multiopen_decide": (i32, [vp, vp, vp, sz, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "amdzk_keygen_vk": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]),
        "amdzk_vk_from_pk": (i32, [vp, vp, C.POINTER(vp)]),
        "amdzk_vk_free": (None, [vp, vp]),
        "amdzk_vk_commitments": (i32, [vp, vp, vp]),
        "amdzk_vk_proof_size_multi": (sz, [vp, sz, i32]),
        "amdzk_vk_serialized_size": (sz, [vp, i32]),
        "amdzk_vk_write": (i32, [vp, vp, vp, vp, vp, sz, C.POINTER(sz)]),
        "amdzk_vk_read": (i32, [vp, vp, sz, C.POINTER(vp), vp, vp, C.POINTER(i32)]),
        "amdzk_vk_blob_info": (i32, [vp, sz, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(i32)]),
        "amdzk_vk_blob_check": (i32, [vp, sz, vp, sz]),
        "amdzk_verify_proofs_vk": (i32, [vp, vp, sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp), C.POINTER(sz), vp, vp, vp]),
        "amdzk_verify_proofs_decide_vk": (i32, [vp, vp, vp, vp, u32, sz, C.POINTER(C.POINTER(vp)), C.POINTER(C.POINTER(sz)), C.POINTER(vp),
                                                C.POINTER(sz), vp, vp, vp, C.POINTER(sz)]),
        "amdzk_verify_proofs_mixed": (i32, [vp, vp, sz, vp, vp, vp]),
        "amdzk_verify_proofs_decide_mixed": (i32, [vp, vp, vp, u32, vp, sz, vp, vp, vp, C.POINTER(sz)]),
        "amdzk_witness_plan": (i32, [vp, sz, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(sz), C.c_char_p, sz]),
        "amdzk_witness_compile": (i32, [vp, vp, C.POINTER(vp)]),
        "amdzk_witness_free": (None, [vp, vp]),
        "amdzk_witness_run": (i32, [vp, vp, sz, C.POINTER(vp), C.POINTER(vp), sz, u32, sz, vp]),
        "amdzk_witness_run_dev": (i32, [vp, vp, sz, vp, sz, C.POINTER(vp), sz, u32, sz, vp]),
        "amdzk_poseidon_check_desc": (i32, [vp, C.c_char_p, sz]),
        "amdzk_poseidon_compile": (i32, [vp, vp, C.POINTER(vp)]),
        "amdzk_poseidon_free": (None, [vp, vp]),
        "amdzk_poseidon_permute_dev": (i32, [vp, vp, vp, sz, sz]),
        "amdzk_poseidon_hash": (i32, [vp, vp, C.POINTER(vp), C.POINTER(sz), sz, vp]),
        "amdzk_poseidon_hash_dev": (i32, [vp, vp, vp, sz, C.POINTER(sz), sz, sz, vp, sz]),
        "amdzk_debug_limb_program": (i32, [vp, sz, vp, sz, C.POINTER(sz), C.POINTER(u32)]),
        "amdzk_pk_h_program": (i32, [vp, vp, sz, C.POINTER(sz)]),
        "amdzk_timer_start": (i32, [vp]),
        "amdzk_timer_stop": (i32, [vp, C.POINTER(C.c_float)]),
        "amdzk_prof_enable": (i32, [vp, i32]),
        "amdzk_prof_reset": (i32, [vp]),
        "amdzk_prof_get": (i32, [vp, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "amdzk_prof_dump": (sz, [vp, C.c_char_p, sz]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    L._amdzk_sig = sig
    _LIB = L
    return L


# include/amdzk.h: amdzk_phases, amdzk_phase_fn, amdzk_transcript, amdzk_proof_opts, amdzk_batch_opts, amdzk_batch_phase_fn,
# amdzk_batch_proof_opts
class Phases(C.Structure):
    _fields_ = [("num_challenges", C.c_uint32), ("advice_phase", C.c_void_p), ("challenge_phase", C.c_void_p)]


PHASE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p)
_T_IN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64))


class Transcript(C.Structure):
    _fields_ = [("user", C.c_void_p), ("common_point", _T_IN), ("common_scalar", _T_IN), ("write_point", _T_IN),
                ("write_scalar", _T_IN), ("squeeze_challenge", _T_IN)]


class ProofOpts(C.Structure):
    _fields_ = [("size", C.c_size_t), ("transcript_kind", C.c_int), ("transcript", C.POINTER(Transcript)), ("phase_fn", PHASE_FN),
                ("phase_user", C.c_void_p), ("rng_seed", C.c_uint64), ("scalars", C.c_void_p), ("scalar_count", C.c_size_t)]


class BatchOpts(C.Structure):
    _fields_ = [("size", C.c_size_t), ("transcript_kind", C.c_int), ("rng_seeds", C.c_void_p), ("scalars", C.POINTER(C.c_void_p)),
                ("scalar_count", C.c_size_t)]


BATCH_PHASE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.c_size_t,
                             C.POINTER(C.c_int), C.c_void_p)


class BatchProofOpts(C.Structure):
    _fields_ = [("size", C.c_size_t), ("transcript_kind", C.c_int), ("rng_seeds", C.c_void_p), ("scalars", C.POINTER(C.c_void_p)),
                ("scalar_count", C.c_size_t), ("transcripts", C.POINTER(C.POINTER(Transcript))), ("phase_fn", BATCH_PHASE_FN),
                ("phase_user", C.c_void_p)]


class MultiopenOpts(C.Structure):
    _fields_ = [("size", C.c_size_t), ("scheme", C.c_int), ("transcript", C.POINTER(Transcript)), ("evals", C.c_void_p)]


class CheckFailure(C.Structure):  # amdzk_check_failure
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("first_row", C.c_uint32), ("reserved", C.c_uint32), ("count", C.c_uint64)]


class CheckOpts(C.Structure):  # amdzk_check_opts
    _fields_ = [("size", C.c_size_t), ("theta_seed", C.c_uint64), ("challenges", C.c_void_p), ("num_challenges", C.c_uint32)]


class SrsCheckOpts(C.Structure):  # amdzk_srs_check_opts
    _fields_ = [("size", C.c_size_t), ("checks", C.c_uint32), ("seed", C.c_uint64), ("rho", C.c_void_p)]


class SrsReport(C.Structure):  # amdzk_srs_report
    _fields_ = [("ran", C.c_uint32), ("failed", C.c_uint32), ("g2_status", C.c_uint32 * 2), ("curve_basis", C.c_uint32), ("reserved", C.c_uint32),
                ("curve_index", C.c_uint64), ("points", C.c_uint64 * 32)]


class ProofStatus(C.Structure):  # amdzk_proof_status
    _fields_ = [("status", C.c_uint32), ("offset", C.c_uint32)]


class TranscriptRead(C.Structure):  # amdzk_transcript_read
    _fields_ = [("user", C.c_void_p), ("common_point", _T_IN), ("common_scalar", _T_IN), ("read_point", _T_IN), ("read_scalar", _T_IN),
                ("squeeze_challenge", _T_IN)]


class VerifyOpts(C.Structure):  # amdzk_verify_opts
    _fields_ = [("size", C.c_size_t), ("transcript_kind", C.c_int), ("n_circuits", C.c_uint32), ("combine_seed", C.c_uint64),
                ("combine_scalars", C.c_void_p), ("transcripts", C.POINTER(C.POINTER(TranscriptRead)))]


VERIFY_OPTS_LEGACY_SIZE = VerifyOpts.transcripts.offset  # the struct before `transcripts`: still accepted, means no transcripts


class VerifyItem(C.Structure):  # amdzk_verify_item
    _fields_ = [("pk", C.c_void_p), ("vk", C.c_void_p), ("transcript_kind", C.c_int), ("n_circuits", C.c_uint32),
                ("instances", C.POINTER(C.POINTER(C.c_void_p))), ("instance_lens", C.POINTER(C.POINTER(C.c_size_t))), ("proof", C.c_void_p),
                ("proof_len", C.c_size_t), ("transcript", C.POINTER(TranscriptRead))]


class VerifyMixedOpts(C.Structure):  # amdzk_verify_mixed_opts
    _fields_ = [("size", C.c_size_t), ("combine_seed", C.c_uint64), ("combine_scalars", C.c_void_p)]


class MultiopenVerifyOpts(C.Structure):  # amdzk_multiopen_verify_opts
    _fields_ = [("size", C.c_size_t), ("scheme", C.c_int), ("transcript", C.POINTER(TranscriptRead))]


def read_transcript(tobj, errors):
    """An amdzk_transcript_read around a Python object with upstream's TranscriptRead method names: common_point((8,) uint64),
    common_scalar((4,)), read_point() -> (8,), read_scalar() -> (4,), squeeze_challenge() -> (4,), all Montgomery words. An
    exception is kept in `errors` and turned into a non-zero return (nothing may unwind through the library). Returns
    (struct, keep-alive); a member the object lacks is a NULL member."""
    def guard(fn):
        def run(*a):
            try:
                return int(fn(*a) or 0)
            except BaseException as e:  # noqa: B902 - reported by the caller
                errors.append(e)
                return 1
        return run

    def taking(name, cnt):
        fn = getattr(tobj, name, None)
        if fn is None:
            return _T_IN()
        return _T_IN(guard(lambda _u, p: fn(np.array([p[i] for i in range(cnt)], dtype=np.uint64))))

    def giving(name, cnt):
        fn = getattr(tobj, name, None)
        if fn is None:
            return _T_IN()

        def give(_u, out):
            v = np.ascontiguousarray(fn(), dtype=np.uint64).reshape(cnt)
            for i in range(cnt):
                out[i] = int(v[i])
        return _T_IN(guard(give))

    cbs = [taking("common_point", 8), taking("common_scalar", 4), giving("read_point", 8), giving("read_scalar", 4), giving("squeeze_challenge", 4)]
    tr = TranscriptRead(None, *cbs)
    return tr, cbs + [tr]


class WitnessDesc(C.Structure):  # amdzk_witness_desc
    _fields_ = [("size", C.c_size_t), ("k", C.c_uint32), ("num_advice", C.c_uint32), ("n_inputs", C.c_uint32), ("n_constants", C.c_uint32),
                ("constants", C.c_void_p), ("n_nodes", C.c_uint32), ("nodes", C.c_void_p), ("n_cells", C.c_uint32), ("cells", C.c_void_p),
                ("n_publics", C.c_uint32), ("publics", C.c_void_p)]


class PoseidonDesc(C.Structure):  # amdzk_poseidon_desc
    _fields_ = [("size", C.c_size_t), ("t", C.c_uint32), ("rate", C.c_uint32), ("r_f", C.c_uint32), ("r_p", C.c_uint32),
                ("round_constants", C.c_void_p), ("mds", C.c_void_p), ("initial_state", C.c_void_p)]


WNODE = np.dtype([("op", np.uint32), ("a", np.uint32), ("b", np.uint32), ("c", np.uint32)])  # amdzk_wnode
WCELL = np.dtype([("node", np.uint32), ("column", np.uint32), ("row", np.uint32)])  # amdzk_wcell
OPEN_QUERY = np.dtype([("poly", np.uint32), ("point", np.uint32)])  # amdzk_open_query


def build_info():
    """amdzk_build_info(): "amdzk <abi> src=<hash> arch=gfx950" -> {"abi": .., "src": .., "arch": ..}."""
    txt = lib().amdzk_build_info().decode()
    parts = txt.split()
    out = {"text": txt, "abi": int(parts[1])}
    out.update(dict(kv.split("=", 1) for kv in parts[2:]))
    return out


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def as_fr_array(a):
    """(n,4) uint64 C-contiguous view/copy: n field elements, Montgomery limbs."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(-1, 4)
    assert a.shape[-1] == 4
    return a


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._chk(ctx.L.amdzk_dev_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.L.amdzk_dev_upload(self.ctx.h, self.ptr, _ptr(arr), arr.nbytes))
        return self

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.ctx._chk(self.ctx.L.amdzk_dev_download(self.ctx.h, _ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.ctx.L.amdzk_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class PinnedBuffer:
    """hipHostMalloc'd staging memory (amdzk_host_alloc), viewed as a numpy array."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        ctx._chk(ctx.L.amdzk_host_alloc(ctx.h, nbytes, C.byref(p)))
        self.ptr = p

    def array(self, shape, dtype=np.uint64):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.nbytes
        buf = (C.c_uint8 * n).from_address(self.ptr.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.ctx.L.amdzk_host_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """amdzk_ctx wrapper. Raises AmdzkError (never falls back to the CPU)."""

    def __init__(self, device_id=0):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.amdzk_init(device_id, C.byref(h))
        if rc != 0:
            raise AmdzkError(rc, "amdzk_init(%d) failed: no usable gfx950 device" % device_id)
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise AmdzkError(rc, self.L.amdzk_last_error(self.h).decode())

    def close(self):
        if self.h:
            self.L.amdzk_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self):
        self._chk(self.L.amdzk_sync(self.h))

    def set_host_wait(self, block):
        """amdzk_set_host_wait: block=True, host waits POLL a completion event (20 us of yielding, then 50-us sleeps: each
        wait ends up to ~50 us late, 8-10 waits per proof); False, they spin in hipStreamSynchronize (the default)."""
        self._chk(self.L.amdzk_set_host_wait(self.h, 1 if block else 0))

    def device(self):
        return self.L.amdzk_ctx_device(self.h)

    def check_affinity(self, pk=None, ptr=None):
        """Raise unless the ctx's stream / workspaces (and `pk`'s buffers, and `ptr`) live on the ctx's device."""
        self._chk(self.L.amdzk_ctx_check_affinity(self.h))
        if pk is not None:
            self._chk(self.L.amdzk_pk_check_affinity(self.h, pk))
        if ptr is not None:
            self._chk(self.L.amdzk_ptr_check_affinity(self.h, C.c_void_p(ptr)))

    def set_stream(self, stream_ptr):
        self._chk(self.L.amdzk_set_stream(self.h, C.c_void_p(stream_ptr)))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def alloc_pinned(self, nbytes):
        return PinnedBuffer(self, nbytes)

    def upload_async(self, dbuf, host_ptr, nbytes):
        """Start a host->device copy on the ctx's copy stream (host_ptr: address of pinned memory)."""
        self._chk(self.L.amdzk_dev_upload_async(self.h, dbuf.ptr, C.c_void_p(host_ptr), nbytes))

    def upload_async_at(self, dbuf, offset, host_ptr, nbytes):
        """upload_async into dbuf + offset (a witness sent as several copies)."""
        assert offset + nbytes <= dbuf.nbytes
        self._chk(self.L.amdzk_dev_upload_async(self.h, C.c_void_p(dbuf.ptr.value + offset), C.c_void_p(host_ptr), nbytes))

    def upload_fence(self):
        self._chk(self.L.amdzk_upload_fence(self.h))

    # ---- timing hooks
    def timer_start(self):
        self._chk(self.L.amdzk_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        self._chk(self.L.amdzk_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def prof_enable(self, on=True):
        self._chk(self.L.amdzk_prof_enable(self.h, 1 if on else 0))

    def prof_reset(self):
        self._chk(self.L.amdzk_prof_reset(self.h))

    def prof_dump(self):
        need = self.L.amdzk_prof_dump(self.h, None, 0)
        buf = C.create_string_buffer(need + 16)
        self.L.amdzk_prof_dump(self.h, buf, need + 16)
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms = line.split()
            out[name] = (int(n), float(ms))
        return out
