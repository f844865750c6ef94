"""CPU: csrc/workspace.hpp's offset counter and the byte layouts built on it — verify_core's one reservation
(verifier::mixed_layout, for a call of one group) and the pairing's image and per-call layouts (pairing.hpp) — through a
stand-alone program (tests/native/workspace_check.cpp, plain g++). Every offset is compared with formulas restated in Python
(the pairing's here, the verify call's in verify_layout_model.py); nothing is compared with a second call into the code under
test. Once more in a build with ASan + UBSan (no sanitizer goes on anything loaded into Python)."""
import os
import subprocess

import pytest

from verify_layout_model import FR, G1, PER_GROUP, PER_ITEM, REGIONS, TOTALS, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "workspace_check.cpp")
_exe = {}

FQ, PTR = 32, 8  # bytes of Fq, a pointer (G1Affine and Fr: verify_layout_model)
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


# (n_proofs, stride, E, NP, NS, nvk, read transcripts, per proof): one proof, a batch through read transcripts, one past a run of
# AMDZK_DECIDE_RUN, a run of one-point proofs, and element counts at and one past a decode block
VERIFY_CASES = [(1, 1984, 70, 40, 30, 12, 0, 0), (3, 4160, 70, 40, 30, 12, 1, 0), (17, 1984, 70, 40, 30, 12, 0, 1), (16, 64, 1, 1, 0, 0, 1, 1),
                (2, 2048, 64, 30, 34, 5, 0, 0), (2, 2080, 65, 31, 34, 6, 1, 1)]


def test_verify_layout_offsets_totals_and_what_the_kernels_rely_on(ask):
    """verify_core's one reservation for a call of ONE group, against the Python model of the layout (verify_layout_model,
    shared with test_verifier_mixed_host.py, which covers many groups)."""
    rows = ask(["verify " + " ".join(map(str, c)) for c in VERIFY_CASES])
    for case, row in zip(VERIFY_CASES, rows):
        n, stride, E, NP, NS, nvk, tr, pp = case
        want = restate([(E, NP, NS, nvk, stride, stride)], [(0, tr)] * n, 1, pp)
        fields = [(name, 1) for name in REGIONS + TOTALS] + [(name, n) for name in PER_ITEM] + [(name, 1) for name in PER_GROUP]
        assert len(row) == sum(count for _, count in fields), case  # every field printed, none skipped
        got, at = {}, 0
        for name, count in fields:
            got[name], at = row[at:at + count], at + count
        assert [got[r][0] for r in REGIONS] == want["regions"] and [got[t][0] for t in TOTALS] == want["totals"], case
        for name in PER_ITEM + PER_GROUP:
            assert got[name] == want[name], (case, name)
        got = {name: v[0] if name in REGIONS + TOTALS else v for name, v in got.items()}
        # commitments | G | points: the MSM's base array, no gap
        assert got["g"] == got["vk"] + nvk * G1 and got["points"] == got["g"] + G1 and got["scalars"] == got["points"] + n * NP * G1, case
        # the decoder and the MSM load points and scalars as 32-byte words: every region, and every proof in the staging area
        for name in REGIONS:
            assert got[name] % 32 == 0, (case, name)
        assert got["item_staging"] == [b * stride for b in range(n)] and stride % 32 == 0 and got["item_stride"] == [stride] * n, case
        assert got["item_points"] == [b * NP for b in range(n)] and got["item_scalars"] == [b * NS for b in range(n)], case
        # the upload ends where G begins (it follows device to device); the download is status .. scalars, whole
        assert got["up_bytes"] == got["g"] and got["staging"] == 0, case
        assert got["status"] + got["down_bytes"] == got["msm"] >= got["scalars"] + n * NS * FR, case
        assert got["bytes"] >= got["run_bases"] + (got["run_len"] * G1 if pp else 0) and got["run_bases"] >= got["msm"], case
        # one single-wave block per (proof, 64 elements)
        assert got["n_blocks"] == n * ((E + 63) // 64) and got["n_elems"] == E and got["n_points"] == n * NP and got["n_scalars"] == n * NS, case
        assert got["run"] == min(n, DECIDE_RUN) and got["run_len"] == (nvk + 1 + got["run"] * NP if pp else 0), case
    assert VERIFY_CASES[2][0] == DECIDE_RUN + 1 and VERIFY_CASES[2][7] == 1, "the case past one run"
    assert [(c[2] + 63) // 64 for c in VERIFY_CASES[3:]] == [1, 1, 2], "one element, a full block, one past it"


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
