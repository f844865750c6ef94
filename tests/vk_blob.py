"""An independent pure-Python encoder of the verifying-key file (include/amdzk.h, amdzk_vk_write): the yardstick
amdzk_vk_write is held to byte for byte, as tests/pk_blob.py is for amdzk_pk_write.

Nothing here comes from the library's writer: the circuit section is pk_blob.header's (the arrays keygen is called with),
the commitments are the protocol oracle's (plonk_ref.keygen), G and the G2 pair are the caller's, the digest is hashlib's."""
import hashlib
import struct

import numpy as np
import pairing_ref as PRF
import pk_blob
import zkutil as zu

MAGIC = b"AMDZKVK\0"
VERSION = 1
PERSON = b"amdzk_vk_blob_v1"


def digest(body):
    return hashlib.blake2b(bytes(body), digest_size=64, person=PERSON).digest()


def seal(body):
    """body (everything before the digest) -> the file."""
    return bytes(body) + digest(body)


def circuit_section(plonk, desc):
    """amdzk_circuit .. phase table: the pk file's header without its magic and version."""
    return pk_blob.header(plonk, desc)[12:]


def g1_bytes(p):
    """(x, y) ints, None for the identity, or 8 words -> 64 bytes."""
    if p is None or isinstance(p, tuple):
        p = zu.point_from_ints(p)
    return np.ascontiguousarray(p, dtype="<u8").reshape(8).tobytes()


def g2_bytes(q):
    """((x0, x1), (y0, y1)) ints or 16 words -> 128 bytes."""
    if isinstance(q, tuple):
        q = PRF.g2_words(q)
    return np.ascontiguousarray(np.array(q, dtype=np.uint64), dtype="<u8").reshape(16).tobytes()


def encode(plonk, desc, fixed_commitments, perm_commitments, transcript_repr, g, g2=None, s_g2=None):
    """The file of a key with these commitments (points as ints, None = the identity, or as words) over G = g."""
    assert (g2 is None) == (s_g2 is None)
    body = MAGIC + struct.pack("<I", VERSION) + circuit_section(plonk, desc)
    body += np.ascontiguousarray(zu.fr_from_int(transcript_repr), dtype="<u8").tobytes()
    body += b"".join(g1_bytes(p) for p in fixed_commitments) + b"".join(g1_bytes(p) for p in perm_commitments)
    body += g1_bytes(g)
    body += b"\x00" if g2 is None else b"\x01" + g2_bytes(g2) + g2_bytes(s_g2)
    return seal(body)


def offsets(plonk, desc, with_g2):
    """Byte offsets of the sections behind the circuit section."""
    o = {"transcript_repr": 12 + len(circuit_section(plonk, desc))}
    o["fixed_commitments"] = o["transcript_repr"] + 32
    o["perm_commitments"] = o["fixed_commitments"] + 64 * desc["num_fixed"]
    o["g"] = o["perm_commitments"] + 64 * len(desc["permutation_columns"])
    o["has_g2"] = o["g"] + 64
    o["digest"] = o["has_g2"] + 1
    if with_g2:
        o["g2"], o["s_g2"] = o["digest"], o["digest"] + 128
        o["digest"] += 256
    return o


def shape(desc, with_g2):
    return dict(pk_blob.shape(desc), has_g2=bool(with_g2))
