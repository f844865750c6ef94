"""An independent pure-Python encoder of the proving-key file (include/amdzk.h, amdzk_pk_write): the yardstick
amdzk_pk_write is held to byte for byte, in the role the Python SRS encoder of test_gpu_msm.py has for amdzk_srs_write.

Nothing here comes from the library's writer: the header is the arrays plonk.flatten_circuit / flatten_phases produce (what
keygen is called with), the columns and commitments are the protocol oracle's (plonk_ref.keygen), the digest is hashlib's."""
import hashlib
import struct

import numpy as np
import zkutil as zu

MAGIC = b"AMDZKPK\0"
VERSION = 1
PERSON = b"amdzk_pk_blob_v1"


def digest(body):
    return hashlib.blake2b(bytes(body), digest_size=64, person=PERSON).digest()


def seal(body):
    """body (everything before the digest) -> the file."""
    return bytes(body) + digest(body)


def header(plonk, desc):
    """magic .. phase table, from the flattened description."""
    cc, a = plonk.flatten_circuit(desc)
    u32 = lambda *v: struct.pack("<%dI" % len(v), *v)
    raw = lambda arr, dt: np.ascontiguousarray(arr, dtype=dt).tobytes()
    out = [MAGIC, u32(VERSION), u32(desc["k"], desc["num_fixed"], desc["num_advice"], desc["num_instance"], desc["blinding_factors"], desc["cs_degree"])]
    for key in ("aq", "fq", "iq"):
        out += [u32(len(a[key])), raw(a[key], "<i4")]
    out += [u32(len(desc["gates"]), len(desc["lookups"]), len(a["off"]) - 1), raw(a["shape"], "<u4"), raw(a["off"], "<u4"), raw(a["words"], "<u4")]
    out += [u32(len(a["consts"])), raw(a["consts"], "<u8"), u32(len(a["perm"])), raw(a["perm"], "<u4")]
    if "advice_column_phase" in desc:
        out += [b"\x01", u32(len(desc["challenge_phase"])), bytes(desc["advice_column_phase"]), bytes(desc["challenge_phase"])]
    else:
        out += [b"\x00"]
    return b"".join(out)


def encode(plonk, oracle, desc, opk, transcript_repr):
    """The file of the key plonk_ref.keygen returned as `opk` for `desc` (for a phased circuit: the description with its
    challenge words, and the oracle key of its specialisation — columns and commitments do not depend on the expressions)."""
    fr = lambda cols: b"".join(np.ascontiguousarray(zu.ints_to_fr(oracle, col), dtype="<u8").tobytes() for col in cols)
    pts = lambda ps: b"".join(np.ascontiguousarray(zu.point_from_ints(p), dtype="<u8").tobytes() for p in ps)
    body = header(plonk, desc) + np.ascontiguousarray(zu.fr_from_int(transcript_repr), dtype="<u8").tobytes()
    body += pts(opk.fixed_commitments) + pts(opk.permutation_commitments) + fr(opk.fixed_values) + fr(opk.permutations)
    return seal(body)


def shape(desc):
    return {"k": desc["k"], "num_fixed": desc["num_fixed"], "num_advice": desc["num_advice"],
            "num_perm_columns": len(desc["permutation_columns"]), "num_challenges": len(desc.get("challenge_phase", []))}


# byte offsets of the header's count fields, for tests that enlarge one: name -> offset, for a description `desc`
def count_offsets(plonk, desc):
    cc, a = plonk.flatten_circuit(desc)
    off = {"num_fixed": 16, "num_advice": 20, "num_instance": 24}
    pos = 12 + 24
    for key, name in (("aq", "num_advice_queries"), ("fq", "num_fixed_queries"), ("iq", "num_instance_queries")):
        off[name] = pos
        pos += 4 + a[key].nbytes
    off["num_gates"], off["num_lookups"], off["num_exprs"] = pos, pos + 4, pos + 8
    pos += 12 + a["shape"].nbytes
    off["expr_offsets_last"] = pos + a["off"].nbytes - 4
    pos += a["off"].nbytes + a["words"].nbytes
    off["num_constants"] = pos
    pos += 4 + a["consts"].nbytes
    off["num_perm_columns"] = pos
    pos += 4 + a["perm"].nbytes
    if "advice_column_phase" in desc:
        off["num_challenges"] = pos + 1
    return off
