"""CPU: the host half of amdzk_verify_proofs (csrc/verifier.hpp) alone, in a stand-alone program (tests/native/
verifier_check.cpp, plain g++): key file from tests/pk_blob.py's encoder, read with pkblob::parse; the proof's elements
decoded here in Python; the printed table of (base, L scalar, R scalar) folded with the oracle's G1 arithmetic must give
tests/verify_ref.py's pair as group elements. Two of the cases once more in a build with ASan + UBSan (no sanitizer goes
on anything loaded into Python)."""
import os
import subprocess

import pytest

import pk_blob
import verify_cases as VC
import verify_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "verifier_check.cpp")
_exe = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("verifier_check") / ("verifier_check_san" if sanitized else "verifier_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def run(exe, plonk, oracle, case, tmp_path, rho=1, env=None):
    key, cf = str(tmp_path / "key.pk"), str(tmp_path / "case.bin")
    with open(key, "wb") as f:
        f.write(pk_blob.encode(plonk, oracle, case.desc, case.opk, VC.REPR))
    pts = VC.write_case_file(cf, case, rho=rho)
    p = subprocess.run([exe, key, cf], text=True, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[0].split()[0] == "plan" and lines[-2] == "ok"
    np_, ns, nbytes, nbases = (int(v) for v in lines[0].split()[1:])
    assert nbytes == len(case.proof) and np_ == len(pts) and nbases == np_ + len(case.opk.fixed_commitments) + len(case.opk.permutation_commitments) + 1
    table = [(int(a), int(b, 16), int(c, 16)) for a, b, c in (ln.split() for ln in lines[1:-2])]
    return pts, table, p


@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_host_half_table_folds_to_the_reference_pair(plonk, oracle, tmp_path, tmp_path_factory, name, N, transcript, multiopen):
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    pts, table, _ = run(build(tmp_path_factory, False), plonk, oracle, case, tmp_path)
    want = case.pair()
    assert want[0] is not None and want[1] is not None
    assert VC.fold_table(case, pts, table) == want


def test_the_weight_scales_both_sums(plonk, oracle, tmp_path, tmp_path_factory):
    case = VC.cpu_case(plonk, "lookup", 1, "blake2b", "shplonk")
    rho = 0x1D2C3B4A5968778695A4B3C2D1E0F123456789ABCDEF
    pts, table, _ = run(build(tmp_path_factory, False), plonk, oracle, case, tmp_path, rho=rho)
    assert VC.fold_table(case, pts, table) == VR.combine([case.pair()], [rho])


@pytest.mark.parametrize("name,N,transcript,multiopen", [("lookup", 2, "evm", "gwc"), ("rlc", 1, "blake2b", "shplonk")])
def test_host_half_is_clean_under_asan_and_ubsan(plonk, oracle, tmp_path, tmp_path_factory, name, N, transcript, multiopen):
    from test_sanitizers import ENV
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    pts, table, p = run(build(tmp_path_factory, True), plonk, oracle, case, tmp_path, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    assert VC.fold_table(case, pts, table) == case.pair()
