"""CPU: csrc/g2codec.hpp in a stand-alone program (tests/native/g2_codec_check.cpp, the host compiler alone): its self-checks
(round trips, every refusal, membership) and the same answers as the Python-integer encoder of test_g2_codec.py on points of
tests/pairing_ref.py. Once plain and once in a build with ASan + UBSan (a stand-alone program: nothing here is loaded into
Python)."""
import os
import random
import subprocess

import pairing_ref as X
from test_g2_codec import ref_encode, small_x_candidates

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "g2_codec_check.cpp")
_exe = {}


def build(tmp_path_factory, sanitized):
    if sanitized not in _exe:
        from test_sanitizers import SAN
        exe = str(tmp_path_factory.mktemp("g2_codec_check") / ("g2_codec_check_san" if sanitized else "g2_codec_check"))
        flags = SAN if sanitized else ["-O2", "-std=c++17"]
        subprocess.check_call(["g++", *flags, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-o", exe, SRC])
        _exe[sanitized] = exe
    return _exe[sanitized]


def flat(q):
    return (0, 0, 0, 0) if q is None else (q[0][0], q[0][1], q[1][0], q[1][1])


def cases(n_points):
    rng = random.Random(0x686F7374)
    pts = [None, X.G2_GEN, X.g2_neg(X.G2_GEN)] + [X.g2_mul(X.G2_GEN, rng.randrange(1, X.R)) for _ in range(n_points)]
    lines, want = [], []
    for p in pts:
        h = " ".join("%x" % v for v in flat(p))
        b = ref_encode(p)
        lines += ["enc " + h, "dec " + b.hex(), "chk " + h]
        want += ["bytes " + b.hex(), "pt " + " ".join("%064x" % v for v in flat(p)), "status %d" % (3 if p is None else 0)]
        if p is not None:
            lines.append("dec " + (b[:63] + bytes([b[63] ^ 0x80])).hex())
            want.append("pt " + " ".join("%064x" % v for v in flat(X.g2_neg(p))))
    (x0, x1), (y0, y1) = X.G2_GEN
    lines += ["enc %x %x %x %x" % (x0, x1, (y0 + 1) % X.P, y1), "chk %x %x %x %x" % (x0, x1, (y0 + 1) % X.P, y1)]
    want += ["refused the point is not on the twist", "status 2"]
    lines += ["dec " + (X.P.to_bytes(32, "little") + x1.to_bytes(32, "little")).hex(), "dec " + (bytes(63) + b"\x80").hex()]
    want += ["refused x is not below the modulus (x >= q)", "refused x = 0 with the sign bit set is no point's encoding"]
    for x in [x for x, res in small_x_candidates() if not res][:4]:
        lines.append("dec " + ref_encode((x, (0, 0))).hex())
        want.append("refused x^3 + 3/xi is not a square: no point of the twist has this x")
    return lines, want


def run(exe, n_points, env=None):
    lines, want = cases(n_points)
    p = subprocess.run([exe], input="\n".join(lines) + "\n", text=True, capture_output=True, env=env, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    out = p.stdout.split("\n")
    assert out[0] == "selfcheck ok" and out[-2] == "ok", out[:3]
    assert out[1:-2] == want
    return p


def test_host_build_matches_the_reference(tmp_path_factory):
    run(build(tmp_path_factory, False), 12)


def test_host_build_is_clean_under_asan_and_ubsan(tmp_path_factory):
    from test_sanitizers import ENV
    p = run(build(tmp_path_factory, True), 3, env=ENV)
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-4000:]
