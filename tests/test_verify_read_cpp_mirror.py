"""verify_proof / verify_proofs / decide_proof of the C++ mirror (include/amdzk_halo2.hpp) through a TranscriptRead of the
caller's, driven from C++ (tests/native/verify_read_mirror_check.cpp): the transcript replays what the oracle's reader hands
back for a proof the device prover made; the guard is the bytes route's word for word through both kinds of key, the proof is
decided valid, a throwing member is rethrown by the single-proof call and is BadTranscript with its offset in a batch."""
import os
import subprocess
import sys

import pytest
import zkutil as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import plonk_ref as PR  # noqa: E402
import verify_cases as VC  # noqa: E402
import verify_ref as VR  # noqa: E402


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vrmc") / "verify_read_mirror_check")
    libdir = os.path.join(ROOT, "anon-aadhaar-halo2_amd")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", out,
                           os.path.join(ROOT, "tests", "native", "verify_read_mirror_check.cpp"), "-L", libdir, "-lamdzk", "-Wl,-rpath," + libdir])
    return out


def test_cpp_mirror_compiles(exe):
    """CPU: the mirror with a caller of the TranscriptRead overloads builds with -Wall -Werror against libamdzk.so."""
    assert subprocess.run([exe], capture_output=True, timeout=120).returncode == 2  # usage


def replay_lines(case):
    """What a reader of the proof's bytes hands back, in the verifier's call order: the order of the bytes, with the
    challenges where tests/verify_ref.py's pair() squeezes them (a phase-0 circuit)."""
    T = (PR.Blake2bRead if case.transcript == "blake2b" else PR.Keccak256Read)(case.proof)
    lines = []

    class Tap:
        def __getattr__(self, name):
            fn = getattr(T, name)
            if name == "read_point":
                def f():
                    p = fn()
                    lines.append("p " + " ".join("%x" % int(w) for w in zu.point_from_ints(p)))
                    return p
                return f
            if name in ("read_scalar", "squeeze_challenge"):
                def f():
                    v = fn()
                    lines.append(("s " if name == "read_scalar" else "c ") + " ".join("%x" % int(w) for w in zu.fr_from_int(v)))
                    return v
                return f
            return fn
    with pytest.MonkeyPatch.context() as mp:
        tap = Tap()
        mp.setattr(PR, "Blake2bRead" if case.transcript == "blake2b" else "Keccak256Read", lambda proof: tap)
        assert VR.pair(case.opk, case.instances_list, case.proof, transcript=case.transcript, multiopen=case.multiopen) is not None
    return lines


def point(words):
    x, y = (zu.fq_to_int([int(w[i:i + 16], 16) for i in (48, 32, 16, 0)]) for w in words)
    return None if x == 0 and y == 0 else (x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("transcript,multiopen", [("blake2b", "shplonk"), ("evm", "gwc")])
def test_cpp_guard_through_a_read_transcript_is_the_bytes_routes(exe, ctx, pkg, oracle, tmp_path, transcript, multiopen):
    from test_gpu_verify import Rig
    plonk = pkg.plonk
    rig = Rig(ctx, pkg, plonk, oracle, "lookup", 1)
    try:
        case = rig.case(transcript, multiopen, seed=41)
        key = str(tmp_path / "key.pk")
        with open(key, "wb") as f:
            f.write(rig.pk.write())
        with open(key + ".inst", "w") as f:
            for col in rig.c.instances:
                f.write(" ".join("%x" % v for v in col) + "\n")
        proof, replay = str(tmp_path / "proof.bin"), str(tmp_path / "replay.txt")
        with open(proof, "wb") as f:
            f.write(case.proof)
        lines = replay_lines(case)
        with open(replay, "w") as f:
            f.write("\n".join(lines) + "\n")
        kinds = VR.element_kinds(case.desc, 1, multiopen)
        assert "".join(ln[0] for ln in lines if ln[0] != "c") == kinds
        out = subprocess.check_output([exe, str(rig.c.k), "%x" % VC.TAU, key, "0" if transcript == "blake2b" else "1",
                                       "0" if multiopen == "shplonk" else "1", proof, replay], text=True, timeout=120).splitlines()
        by = out[0].split()
        assert by[:3] == ["bytes", "0", "0"] and (point(by[3:5]), point(by[5:7])) == case.pair()
        assert out[1].split()[1:] == by[1:] and out[1].split()[0] == "read"
        assert out[2].split()[1:] == by[1:] and out[2].split()[0] == "read_vk"
        assert out[3] == "decide 1 1"
        n_inst = sum(len(col) for col in rig.c.instances)
        assert out[4] == "calls %d %d %d 0" % (1 + n_inst, len(kinds), sum(ln[0] == "c" for ln in lines))
        assert out[5] == "throwing: read failed"
        assert out[6:] == ["status 0 0", "status 5 3"]
    finally:
        rig.free()
