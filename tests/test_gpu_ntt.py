"""GPU parity: amdzk_ntt_fr* (HIP, gfx950) vs the oracle's best_fft restatement, bit-exact."""
import numpy as np
import pytest
import zkutil as zu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8, 10, 11, 12, 13, 15, 16, 17, 18, 20])
def test_ntt_matches_oracle(ctx, pkg, oracle, k):
    a = zu.random_fr(1 << k, seed=100 + k)
    w = oracle.omega(k)
    want = oracle.best_fft(a.copy(), w, k)
    got = pkg.arithmetic.best_fft(ctx, a.copy(), w, k)
    assert np.array_equal(got, want)


def test_ntt_golden_vectors(ctx, pkg, oracle):
    import json, os
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bn254_golden.json")))
    for v in G["ntt"]:
        a = zu.fr_array_from_ints([int(x, 16) for x in v["a"]])
        got = pkg.arithmetic.best_fft(ctx, a, oracle.omega(v["k"]), v["k"])
        assert zu.fr_array_to_ints(got) == [int(x, 16) for x in v["ntt"]]


@pytest.mark.parametrize("k", [4, 12, 16, 19])
def test_intt_roundtrip_and_scale(ctx, pkg, oracle, k):
    a = zu.random_fr(1 << k, seed=7 * k)
    w = oracle.omega(k)
    winv = oracle.fr_inv(w.reshape(1, 4)).reshape(4)
    f = pkg.arithmetic.best_fft(ctx, a.copy(), w, k)
    back = pkg.arithmetic.best_fft(ctx, f.copy(), winv, k, flags=pkg.arithmetic.NTT_SCALE_NINV)
    assert np.array_equal(back, a)


def test_ntt_batch_device_columns(ctx, pkg, oracle):
    k, ncols = 14, 5
    n = 1 << k
    stride = n + 64  # columns need not be packed
    w = oracle.omega(k)
    host = np.zeros((ncols, stride, 4), dtype=np.uint64)
    cols = [zu.random_fr(n, seed=900 + c) for c in range(ncols)]
    for c in range(ncols):
        host[c, :n] = cols[c]
    buf = ctx.alloc(host.nbytes).upload(host)
    pkg.arithmetic.best_fft_dev(ctx, buf, w, k, ncols=ncols, col_stride=stride)
    out = buf.download(host.shape)
    buf.free()
    for c in range(ncols):
        assert np.array_equal(out[c, :n], oracle.best_fft(cols[c].copy(), w, k))
        assert not out[c, n:].any()


def test_ntt_linearity_at_full_size(ctx, pkg, oracle):
    """Size-independent property at the k=22 stress size: NTT(a+b) = NTT(a)+NTT(b), and
    iNTT(NTT(a)) = a; spot-check 64 outputs against direct evaluation sum_i a_i w^(ij)."""
    k = 22
    n = 1 << k
    a, b = zu.random_fr(n, seed=1), zu.random_fr(n, seed=2)
    w = oracle.omega(k)
    fa = pkg.arithmetic.best_fft(ctx, a.copy(), w, k)
    fb = pkg.arithmetic.best_fft(ctx, b.copy(), w, k)
    fab = pkg.arithmetic.best_fft(ctx, oracle.fr_add(a, b), w, k)
    assert np.array_equal(fab, oracle.fr_add(fa, fb))
    winv = oracle.fr_inv(w.reshape(1, 4)).reshape(4)
    back = pkg.arithmetic.best_fft(ctx, fa.copy(), winv, k, flags=pkg.arithmetic.NTT_SCALE_NINV)
    assert np.array_equal(back, a)
    # full-size cross-check against the oracle itself (CPU, a few seconds)
    assert np.array_equal(fa, oracle.best_fft(a.copy(), w, k))


# ---------------------------------------------------------------------------------------------------------------------
# Extreme operands. ntt_step_kernel keeps its tile on 9 x 29-bit limbs, leaves sums unreduced for up to two rounds and
# makes differences non-negative by adding a fixed multiple of p; the bounds that make this safe are proved on the host
# and pinned per function (fp29_check, fp29_device_check). With uniform data a bound that is one bit too tight goes wrong
# with negligible probability, so the composed kernel is run here on Montgomery words written directly (no conversion:
# the word IS the operand), all below r: the largest word, the word with the most one-bits in its low limbs, and layouts
# that make every butterfly of a round a maximal sum, a maximal difference, or both at once.
# The builders live in zkutil.py (test_gpu_plonk_operands.py feeds the same columns to the PLONK-layer kernels).
from zkutil import PATTERNS, RM1, T232M1  # noqa: E402,F401

# One size per plan class and per parity of the sub-transform length s (odd s: the single-round prologue; s >= 2 ends in
# f29_dif4_last). One step: s = k. Two steps: 11 = 6 + 5, 14 = 7 + 7, 17 = 9 + 8, 18 = 9 + 9. Three steps: 19 = 7 + 6 + 6
# (the first size with the half twiddle table), 21 = 7 + 7 + 7. From k = 17 up three patterns per size, dealt so that
# every pattern meets a large size.
SMALL_K = [1, 2, 3, 4, 7, 9, 10, 11, 14]
LARGE = {17: ("const_rm1", "alt_rm1_0", "random_8th_rm1"), 18: ("const_t232m1", "half_rm1_0", "single_last"),
         19: ("const_rm1", "half_rm1_0", "random_8th_rm1"), 21: ("const_rm1", "alt_0_rm1", "random_8th_rm1")}
EXTREME_CASES = [(k, p) for k in SMALL_K for p in PATTERNS] + [(k, p) for k in sorted(LARGE) for p in LARGE[k]]
SCALED_CASES = [(k, p) for k in (4, 11) for p in PATTERNS] + [(19, p) for p in LARGE[19]]


@pytest.mark.parametrize("k,pattern", EXTREME_CASES)
def test_ntt_extreme_operands_match_oracle(ctx, pkg, oracle, k, pattern):
    a = PATTERNS[pattern](1 << k)
    w = oracle.omega(k)
    want = oracle.best_fft(a.copy(), w, k)
    got = pkg.arithmetic.best_fft(ctx, a.copy(), w, k)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k,pattern", SCALED_CASES)
def test_ntt_extreme_operands_scaled_match_oracle(ctx, pkg, oracle, k, pattern):
    """NTT_SCALE_NINV: every element leaves the last step through the F_OUT_MUL product instead of the weak reduction.
    Expected: the oracle's transform times 2^-k in the oracle's field arithmetic."""
    n = 1 << k
    a = PATTERNS[pattern](n)
    w = oracle.omega(k)
    want = oracle.fr_mul(oracle.best_fft(a.copy(), w, k), np.tile(zu.fr_from_int(pow(n, -1, zu.R)), (n, 1)))
    got = pkg.arithmetic.best_fft(ctx, a.copy(), w, k, flags=pkg.arithmetic.NTT_SCALE_NINV)
    assert np.array_equal(got, want)
