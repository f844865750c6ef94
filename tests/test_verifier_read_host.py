"""CPU: the host half of amdzk_verify_proofs (csrc/verifier.hpp) through the CALLER's read transcript, in a stand-alone
program (tests/native/verifier_read_check.cpp, plain g++): the callback adapter over recorded elements must give the
per-base scalars of the built-in route bit for bit (the program compares them itself), the printed table folded with the
oracle's G1 arithmetic must give tests/verify_ref.py's pair, and every callback failure point ends the walk where it
happened (a non-zero return of every call in turn, a challenge >= r at every squeeze, a NULL member). Two of the cases once
more in a build with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import os
import subprocess

import pytest

import pk_blob
import verify_cases as VC
import verify_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "verifier_read_check.cpp")
_exe = {}


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("verifier_read_check") / ("verifier_read_check_san" if sanitized else "verifier_read_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def run(exe, plonk, oracle, case, tmp_path, env=None):
    key, cf = str(tmp_path / "key.pk"), str(tmp_path / "case.bin")
    with open(key, "wb") as f:
        f.write(pk_blob.encode(plonk, oracle, case.desc, case.opk, VC.REPR))
    pts = VC.write_case_file(cf, case)
    p = subprocess.run([exe, key, cf], text=True, capture_output=True, env=env, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[0].split()[0] == "plan" and lines[-2] == "ok" and lines[-3].split()[0] == "failures" and lines[-4].split()[0] == "calls"
    table = [(int(a), int(b, 16), int(c, 16)) for a, b, c in (ln.split() for ln in lines[1:-4])]
    commons, reads, squeezes = (int(v) for v in lines[-4].split()[1:])
    kinds = VR.element_kinds(case.desc, case.N, case.multiopen)
    assert reads == len(kinds)
    assert commons == 1 + sum(len(col) for instances in case.instances_list for col in instances)
    # one failing return per call, and one oversized challenge per squeeze
    assert int(lines[-3].split()[1]) == commons + reads + 2 * squeezes and squeezes >= 7
    return pts, table, p


@pytest.mark.parametrize("name,N,transcript,multiopen", VC.CASE_IDS)
def test_callback_route_gives_the_builtin_scalars_and_the_reference_pair(plonk, oracle, tmp_path, tmp_path_factory, name, N, transcript, multiopen):
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    pts, table, _ = run(build(tmp_path_factory, False), plonk, oracle, case, tmp_path)
    assert VC.fold_table(case, pts, table) == case.pair()


@pytest.mark.parametrize("name,N,transcript,multiopen", [("lookup", 2, "evm", "gwc"), ("rlc", 1, "blake2b", "shplonk")])
def test_callback_route_is_clean_under_asan_and_ubsan(plonk, oracle, tmp_path, tmp_path_factory, name, N, transcript, multiopen):
    from test_sanitizers import ENV
    case = VC.cpu_case(plonk, name, N, transcript, multiopen)
    pts, table, p = run(build(tmp_path_factory, True), plonk, oracle, case, tmp_path, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    assert VC.fold_table(case, pts, table) == case.pair()
