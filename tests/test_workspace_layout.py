"""CPU: csrc/workspace.hpp's offset counter and the byte layouts built on it — verify_core's one reservation
(verifier::device_layout) and the pairing's image and per-call layouts (pairing.hpp) — through a stand-alone program
(tests/native/workspace_check.cpp, plain g++). Every offset is compared with the formulas the drivers carried before the
layouts had a type, restated here; nothing is compared with a second call into the code under test. Once more in a build
with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "workspace_check.cpp")
_exe = {}

G1, FR, FQ, UINT2, PTR = 64, 32, 32, 8, 8  # bytes of G1Affine, Fr, Fq, uint2, a pointer
FQ2X = 2 * 9 * 4  # an Fq2 of two stored-form Fq: nine 29-bit limbs each
DECIDE_RUN, PAIRING_MAX_M, CHUNK_LANES, K_COUNT = 16, 16, 16384, 17  # include/amdzk.h, pairing.hip as it was, pairing.hpp
NUM_LINES = 64 + bin(0x9D797039BE763BA8).count("1") + 2  # fq12.cuh: a line per doubling, per set bit of 6u + 2 below the top, two Frobenius lines


def pad256(v):
    return (v + 255) // 256 * 256


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("workspace_check") / ("workspace_check_san" if sanitized else "workspace_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def run(exe, commands, env=None):
    p = subprocess.run([exe], input="\n".join(commands) + "\n", text=True, capture_output=True, env=env, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = p.stdout.split("\n")
    assert lines[-2] == "ok" and len(lines) >= len(commands) + 2
    if env is not None:
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
    return [[int(t) for t in ln.split()] for ln in lines[:-2]]


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def ask(request, tmp_path_factory):
    """commands -> rows of integers, from the plain build and from the sanitized one"""
    exe = build(tmp_path_factory, request.param)
    env = None
    if request.param:
        from test_sanitizers import ENV
        env = ENV
    return lambda commands: run(exe, commands, env)


def test_take_advances_to_the_next_multiple_of_the_pad(ask):
    sizes = [0, 1, 255, 256, 257, (1 << 40) + 1]
    (row,) = ask(["take 256 " + " ".join(map(str, sizes))])
    off, want = 0, []
    for s in sizes:
        want += [off, pad256(off + s)]
        off = pad256(off + s)
    assert row == want
    assert row[:10] == [0, 0, 0, 256, 256, 512, 512, 768, 768, 1280] and row[-1] == 1280 + (1 << 40) + 256, "and by hand"


def test_a_region_taken_with_pad_1_is_followed_without_a_gap(ask):
    (row,) = ask(["take 1 5 p256 7 p1 3 p256 1 p1 0 p64 1"])
    #            take(5, 1)  take(7)   take(3, 1)  take(1)   take(0, 1)  take(1, 64)
    assert row == [0, 5,     5, 256,   256, 259,   259, 512, 512, 512,   512, 576]


def test_round_up_of_element_counts_to_four(ask):
    (row,) = ask(["round 4 " + " ".join(map(str, range(10)))])
    assert row == [0, 4, 4, 4, 4, 8, 8, 8, 8, 12]
    assert ask(["round 256 0 1 256 257", "round 1 0 1 7"]) == [[0, 256, 256, 512], [0, 1, 7]]


def verify_layout(n_proofs, psize, E, NP, NS, nvk, n_tr, per_proof):
    """verify_core's offsets as it computed them itself (a verifying key: its G goes up with its commitments)"""
    nbases = nvk + 1 + n_proofs * NP
    o_elems = pad256(n_proofs * psize)
    o_eraw = o_elems + pad256(E * UINT2)
    o_form = o_eraw + (pad256(E * UINT2) if n_tr else 0)
    o_status = o_form + (pad256(n_proofs) if n_tr else 0)
    o_vk = o_status + pad256(n_proofs * 4)
    o_g = o_vk + nvk * G1
    o_points = o_g + G1
    o_dsc = o_points + n_proofs * NP * G1
    run = min(n_proofs, DECIDE_RUN)
    run_len = nvk + 1 + run * NP
    o_msm = pad256(o_dsc + n_proofs * NS * 32)
    o_rb = pad256(o_msm + 2 * run * run_len * 32)
    total = o_rb + run_len * G1 if per_proof else o_msm + 2 * nbases * 32
    return {"staging": 0, "elems": o_elems, "elems_raw": o_eraw, "form": o_form, "status": o_status, "vk": o_vk, "g": o_g, "points": o_points,
            "scalars": o_dsc, "msm": o_msm, "run_bases": o_rb if per_proof else total, "bytes": total, "up_bytes": o_points,
            "down_bytes": o_msm - o_status, "run": run, "run_len": run_len}


VERIFY_CASES = [(1, 1984, 70, 40, 30, 12, 0, 0), (3, 4160, 70, 40, 30, 12, 1, 0), (17, 1984, 70, 40, 30, 12, 0, 1), (16, 64, 1, 1, 0, 0, 1, 1)]


def test_verify_layout_offsets_totals_and_what_the_kernels_rely_on(ask):
    rows = ask(["verify " + " ".join(map(str, c)) for c in VERIFY_CASES])
    for case, row in zip(VERIFY_CASES, rows):
        want = verify_layout(*case)
        got = dict(zip(want.keys(), row))
        assert len(row) == len(want) and got == want, case
        n, _stride, _E, NP, NS, nvk, _tr, _pp = case
        # commitments | G | points: the MSM's base array, no gap
        assert got["g"] == got["vk"] + nvk * G1 and got["points"] == got["g"] + G1 and got["scalars"] == got["points"] + n * NP * G1, case
        # the decoder and the MSM load points and scalars as 32-byte words
        for name in ("staging", "vk", "g", "points", "scalars", "msm", "run_bases"):
            assert got[name] % 32 == 0, (case, name)
        # the upload ends where the decoded regions begin; the download is status .. scalars, whole
        assert got["up_bytes"] == got["points"], case
        assert got["status"] + got["down_bytes"] == got["msm"] >= got["scalars"] + n * NS * FR, case
    assert verify_layout(*VERIFY_CASES[2])["run"] == DECIDE_RUN and VERIFY_CASES[2][0] == DECIDE_RUN + 1, "the case past one run"


def test_pairing_image_and_call_layouts(ask):
    consts, regs, image, *calls = ask(["consts", "image"] + ["call %d %d" % nm for nm in PAIRING_CASES])
    chunk_lanes, k_count, num_lines, miller_len, mul_len, fin_len, miller_regs, final_regs, fq2x, max_m = consts
    assert (chunk_lanes, k_count, num_lines, fq2x, max_m) == (CHUNK_LANES, K_COUNT, NUM_LINES, FQ2X, PAIRING_MAX_M)
    assert final_regs == max(regs) and min(miller_len, mul_len, fin_len) > 0 and miller_regs > 0
    # the image of a prepared point: constants | lines | the three programs (pairing.hip's Programs as it was)
    o_lines = pad256(K_COUNT * FQ2X)
    o_miller = o_lines + pad256(4 * NUM_LINES * FQ)
    o_mul = o_miller + pad256(miller_len * 4)
    o_fin = o_mul + pad256(mul_len * 4)
    assert image == [o_lines, o_miller, o_mul, o_fin, o_fin + pad256(fin_len * 4)]
    # one call (zk_pairing_products as it was)
    for (n, m), row in zip(PAIRING_CASES, calls):
        total, chunk = n * m, min(CHUNK_LANES // m, n)
        o_g1 = pad256(PAIRING_MAX_M * PTR)
        o_ms = o_g1 + pad256(total * G1)
        o_fs = o_ms + pad256(chunk * m * miller_regs * FQ2X)
        o_gt = o_fs + pad256(chunk * final_regs * FQ2X)
        o_one = o_gt + n * 12 * FQ
        assert row == [chunk, o_g1, o_ms, o_fs, o_gt, o_one, o_one + pad256(n)], (n, m)
    assert min(CHUNK_LANES // 16, 2000) < 2000, "the last case runs in more than one chunk"


PAIRING_CASES = [(1, 1), (1, 2), (5, 2), (2000, 16)]
