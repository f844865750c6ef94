"""GPU: proving keys that outlive the process — amdzk_pk_write / amdzk_pk_read / amdzk_keygen_sigma / amdzk_pk_export.

The file a key writes is held byte for byte to the independent Python encoder (tests/pk_blob.py: the flattened description,
the protocol oracle's columns and commitments, hashlib's BLAKE2b). A key read from the ENCODER's file — the key that was
made is freed first — has the oracle's commitments and proves the oracle's bytes; for phased keys through the route of
test_gpu_phased.py (tests/phased_oracle.py).

random_circuit(k=6, seed=1) has an h(X) piece that is zero: its commitment is the identity, which upstream's transcript
refuses to write ("cannot write points at infinity to the transcript"), and so do the oracle and the device
(tests/test_random_circuits.py has such a case for the same reason). The case stays: its file, columns and commitments are
checked like every other's, and where the others compare proof bytes it compares the refusal — REFUSED on both sides, from
every key, with the context proving the next case afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import circuits  # noqa: E402
import phased_circuits as PC  # noqa: E402
import phased_oracle as PO  # noqa: E402
import pk_blob  # noqa: E402
import plonk_ref as PR  # noqa: E402
from test_gpu_phased import Device  # noqa: E402

pytestmark = pytest.mark.gpu
TAU = 0x1234567890ABCDEF1234567
REPR = 123456789
_srs_cache, _case_cache = {}, {}
REFUSED = "refused: a commitment is the point at infinity"

CASES = {
    "square-k4": lambda p: circuits.square_circuit(p, 4),
    "lookup-k5": lambda p: circuits.lookup_circuit(p, 5, seed=2),
    "lookup-k7": lambda p: circuits.lookup_circuit(p, 7, seed=3),
    "high-degree-k5": lambda p: circuits.high_degree_circuit(p, 5),
    "random-k6-s0": lambda p: circuits.random_circuit(p, 6, seed=0),
    "random-k6-s1": lambda p: circuits.random_circuit(p, 6, seed=1),
    "random-k6-s2": lambda p: circuits.random_circuit(p, 6, seed=2),
    "rlc-k5": lambda p: PC.rlc_circuit(p, 5, seed=5),
    "rlc-k5-three": lambda p: PC.rlc_circuit(p, 5, seed=5, three_phases=True),
    "random-phased-k5-s0": lambda p: PC.random_phased_circuit(p, 5, seed=0),
    "random-phased-k5-s1": lambda p: PC.random_phased_circuit(p, 5, seed=1),
}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def srs(ctx, pkg, oracle, k, tau=TAU):
    if (k, tau) not in _srs_cache:
        _srs_cache[(k, tau)] = zu.test_srs(oracle, k, tau)
    g, gl = _srs_cache[(k, tau)]
    return pkg.kzg.ParamsKZG(ctx, k, g=g, g_lagrange=gl)


class Case:
    """A circuit, the oracle's key for it and the encoder's file: made once, shared by the tests, never modified."""

    def __init__(self, plonk, oracle, name):
        self.c = c = CASES[name](plonk)
        self.phased = "advice_column_phase" in c.desc
        odesc = PO.specialise(c.desc, [0] * len(c.desc["challenge_phase"])) if self.phased else c.desc
        self.opk = PR.keygen(odesc, c.fixed, c.assembly.mapping, TAU, transcript_repr=REPR)
        self.blob = pk_blob.encode(plonk, oracle, c.desc, self.opk, REPR)
        fr = lambda cols: np.stack([zu.ints_to_fr(oracle, col) for col in cols]) if cols else np.zeros((0, c.n, 4), np.uint64)
        self.fixed, self.sigma = fr(c.fixed), fr(self.opk.permutations)
        self.fixed_polys, self.sigma_polys = fr(self.opk.fixed_polys), fr(self.opk.permutation_polys)
        self.adv = fr(c.advice)
        self.inst = [zu.ints_to_fr(oracle, col) if col else np.zeros((0, 4), np.uint64) for col in c.instances]


def case(plonk, oracle, name):
    if name not in _case_cache:
        _case_cache[name] = Case(plonk, oracle, name)
    return _case_cache[name]


def device_for(ctx, pkg, plonk, oracle, c, pk):
    """test_gpu_phased.Device proving with a key that already exists: built by its own constructor (which makes a key from
    the mapping), then that key is freed and the key under test takes its place."""
    dev = Device(ctx, pkg, plonk, oracle, c, flags=0)
    dev.pk.free()
    dev.pk, dev.pks = pk, [pk]
    return dev


class Prover:
    """Proofs on any key of a case, and the oracle's bytes for them (computed once per (seed, transcript))."""

    def __init__(self, ctx, pkg, plonk, oracle, cs, monkeypatch):
        self.ctx, self.pkg, self.plonk, self.oracle, self.cs, self.mp = ctx, pkg, plonk, oracle, cs, monkeypatch
        self.d_adv = None if cs.phased else ctx.alloc(max(32, cs.adv.nbytes)).upload(cs.adv)
        self.want = {}

    def prove(self, pk, seed=7, transcript=0):
        if not self.cs.phased:
            try:
                return self.plonk.create_proof(self.ctx, pk, self.cs.inst, self.d_adv, seed=seed, transcript=transcript)
            except self.pkg.AmdzkError as e:
                if "points at infinity" not in str(e):
                    raise
                return REFUSED
        dev = device_for(self.ctx, self.pkg, self.plonk, self.oracle, self.cs.c, pk)
        try:
            got = dev.prove(seed=seed, transcript=transcript)
            self.last = (dev.adv, dev.challenges())
            return got
        finally:
            dev.d_adv[0].free()
            dev.params.free()

    def oracle_bytes(self, seed=7, transcript="blake2b", multiopen="shplonk"):
        """For a phased case: after prove() — the harness needs the challenges and the witness they led to."""
        key = (seed, transcript, multiopen)
        if key not in self.want:
            cs = self.cs
            if cs.phased:
                adv, ch = self.last
                self.want[key] = PO.create_proof(self.mp, cs.opk, cs.c.desc, [cs.c.instances], adv, seed, ch, transcript=transcript, multiopen=multiopen)
            else:
                try:
                    self.want[key] = PR.create_proof(cs.opk, cs.c.instances, cs.c.advice, seed=seed, transcript=transcript, multiopen=multiopen)
                except AssertionError as e:
                    if "points at infinity" not in str(e):
                        raise
                    self.want[key] = REFUSED
        return self.want[key]

    def free(self):
        if self.d_adv is not None:
            self.d_adv.free()


def commitments_are_the_oracles(pk, opk):
    f, p = pk.commitments()
    return [zu.point_to_ints(x) for x in f] == opk.fixed_commitments and [zu.point_to_ints(x) for x in p] == opk.permutation_commitments


@pytest.mark.parametrize("name", list(CASES))
def test_write_read_and_sigma_give_the_same_key(ctx, pkg, plonk, oracle, monkeypatch, name):
    cs = case(plonk, oracle, name)
    c = cs.c
    params = srs(ctx, pkg, oracle, c.k)
    P = Prover(ctx, pkg, plonk, oracle, cs, monkeypatch)
    # ---- a key made from the mapping: its file, its columns
    pk = plonk.ProvingKey(ctx, params, c.desc, cs.fixed, c.assembly.mapping, zu.fr_from_int(REPR), flags=0)
    blob = pk.write()
    assert len(blob) == ctx.L.amdzk_pk_serialized_size(pk.h) == len(cs.blob)
    assert blob == cs.blob, "amdzk_pk_write differs from the Python encoder"
    assert plonk.blob_info(blob) == pk_blob.shape(c.desc)
    clone = pk.clone_workspace()
    for what, want in enumerate((cs.fixed, cs.sigma, cs.fixed_polys, cs.sigma_polys)):
        got = pk.export(what)
        assert got.shape == want.shape and np.array_equal(got, want), "export(%d)" % what
        assert np.array_equal(clone.export(what), got), "export(%d) from a clone" % what
    assert clone.write() == blob
    made = P.prove(pk)
    assert made == P.oracle_bytes()
    assert (made == REFUSED) == (name == "random-k6-s1")
    clone.free()
    pk.free()
    # ---- the key read from the ENCODER's file; the key that was made is gone
    rk = plonk.ProvingKey.read(ctx, params, cs.blob, flags=0)
    assert commitments_are_the_oracles(rk, cs.opk)
    assert rk.desc["k"] == c.k and pk_blob.header(plonk, rk.desc) == pk_blob.header(plonk, c.desc)
    assert P.prove(rk) == made
    assert rk.write() == cs.blob, "write of a key that was read"
    rc = rk.clone_workspace()
    assert P.prove(rc) == made
    if not cs.phased:  # amdzk_create_proof_batch proves phase-0 keys only
        d2 = ctx.alloc(max(32, cs.adv.nbytes)).upload(cs.adv)
        two = plonk.create_proof_batch(ctx, [rk, rc], [cs.inst, cs.inst], [P.d_adv, d2], [7, 8])
        two = [p if isinstance(p, bytes) else REFUSED for p in two]  # a refused proof comes back as its AmdzkError
        assert two == [made, P.prove(rc, seed=8)] and two[1] == P.oracle_bytes(seed=8)
        d2.free()
    rc.free()
    rk.free()
    # ---- the key from the oracle's sigma columns
    sk = plonk.ProvingKey.from_sigma(ctx, params, c.desc, cs.fixed, cs.sigma, zu.fr_from_int(REPR), flags=0)
    assert commitments_are_the_oracles(sk, cs.opk)
    assert sk.write() == cs.blob
    assert P.prove(sk) == made
    sk.free()
    P.free()
    params.free()


@pytest.mark.parametrize("flags", [None, "serial", "full_cosets"])
def test_read_key_in_every_mode_transcript_and_multiopen(ctx, pkg, plonk, oracle, monkeypatch, flags):
    """One lookup circuit: a key read with flags None (the environment's), KEYGEN_SERIAL and KEYGEN_FULL_COSETS proves the
    oracle's bytes with Blake2b and Keccak/EVM, SHPLONK and GWC. The flags are not part of the file."""
    cs = case(plonk, oracle, "lookup-k5")
    params = srs(ctx, pkg, oracle, cs.c.k)
    P = Prover(ctx, pkg, plonk, oracle, cs, monkeypatch)
    fl = {None: None, "serial": plonk.KEYGEN_SERIAL, "full_cosets": plonk.KEYGEN_FULL_COSETS}[flags]
    rk = plonk.ProvingKey.read(ctx, params, cs.blob, flags=fl)
    assert rk.write() == cs.blob
    for tr, mo in (("blake2b", "shplonk"), ("evm", "shplonk"), ("blake2b", "gwc"), ("evm", "gwc")):
        tk = (plonk.TRANSCRIPT_KECCAK256_EVM if tr == "evm" else plonk.TRANSCRIPT_BLAKE2B) | (plonk.MULTIOPEN_GWC if mo == "gwc" else 0)
        assert P.prove(rk, seed=11, transcript=tk) == P.oracle_bytes(11, tr, mo), (flags, tr, mo)
    rk.free()
    P.free()
    params.free()


def test_refusals_leave_the_context_proving(ctx, pkg, plonk, oracle, monkeypatch):
    """Each refusal is AMDZK_E_INVALID with its message, and the same ctx then reads the good file and proves the oracle's bytes."""
    cs = case(plonk, oracle, "lookup-k5")
    c = cs.c
    params = srs(ctx, pkg, oracle, c.k)
    P = Prover(ctx, pkg, plonk, oracle, cs, monkeypatch)

    def still_proves():
        rk = plonk.ProvingKey.read(ctx, params, cs.blob, flags=0)
        assert P.prove(rk) == P.oracle_bytes()
        rk.free()

    def refused(match, fn):
        with pytest.raises(pkg.AmdzkError, match=match) as e:
            fn()
        assert e.value.code == -2
        still_proves()

    other_tau = srs(ctx, pkg, oracle, c.k, tau=TAU + 1)
    refused("pk_read: .*other parameters", lambda: plonk.ProvingKey.read(ctx, other_tau, cs.blob, flags=0))
    other_tau.free()
    other_k = srs(ctx, pkg, oracle, c.k + 1)
    refused("pk_read: the key is for k = 5, the parameters are for k = 6", lambda: plonk.ProvingKey.read(ctx, other_k, cs.blob, flags=0))
    other_k.free()
    bad = bytearray(cs.blob)
    bad[len(bad) - 64 - 32 * c.n * (len(cs.fixed) + len(cs.sigma)) + 5] ^= 0x10  # inside the first fixed column
    refused("pk_read: digest mismatch", lambda: plonk.ProvingKey.read(ctx, params, bytes(bad), flags=0))
    refused("pk_read: length mismatch", lambda: plonk.ProvingKey.read(ctx, params, cs.blob[:-1], flags=0))
    refused("pk_read: .*too few", lambda: plonk.ProvingKey.read(ctx, params, cs.blob[:40], flags=0))
    refused("pk_read: null argument", lambda: plonk.ProvingKey.read(ctx, params, None, flags=0))
    refused("pk_read: bad magic", lambda: plonk.ProvingKey.read(ctx, params, b"x" + cs.blob[1:], flags=0))
    refused("pk_read: keygen: unknown flags", lambda: plonk.ProvingKey.read(ctx, params, cs.blob, flags=64))
    refused("keygen: sigma_values is null", lambda: plonk.ProvingKey.from_sigma(ctx, params, c.desc, cs.fixed, None, zu.fr_from_int(REPR), flags=0))
    P.free()
    params.free()


def test_cpp_mirror_write_read_from_sigma(plonk, oracle, tmp_path):
    """include/amdzk_halo2.hpp: configure -> keygen -> write -> (key freed) -> read -> prove, from_sigma with the exported
    columns, a damaged file refused — driven from C++ (tests/native/pk_blob_roundtrip.cpp), built as test_cpp_mirror.py
    builds its host. Every proof is the oracle's, every file the encoder's."""
    from test_cpp_mirror import write_witness
    exe = str(tmp_path / "pk_blob_roundtrip")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "native", "pk_blob_roundtrip.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    c = circuits.lookup_circuit(plonk, 5, seed=3)
    wit = str(tmp_path / "witness.txt")
    write_witness(c, wit)
    opk = PR.keygen(c.desc, c.fixed, c.assembly.mapping, TAU, transcript_repr=0xC0FFEE)
    out = subprocess.check_output([exe, wit, "17", "%x" % TAU, "%x" % 0xC0FFEE], text=True, timeout=300)
    val = {ln.split()[0]: ln.split()[1] for ln in out.splitlines() if len(ln.split()) == 2}
    want = PR.create_proof(opk, c.instances, c.advice, seed=17)
    for tag in ("proof_made", "proof_read", "proof_read_clone", "proof_sigma", "proof_after_refusal"):
        assert bytes.fromhex(val[tag]) == want, tag
    blob = pk_blob.encode(plonk, oracle, c.desc, opk, 0xC0FFEE)
    for tag in ("file", "file_again", "file_sigma"):
        assert bytes.fromhex(val[tag]) == blob, tag
    assert "damaged refused -2 " in out and "pk_read: digest mismatch" in out
