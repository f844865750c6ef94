"""Cases for the lookup argument's permutation (amdzk_permute_expression_pair_dev: the bitonic sort, lookup_mark, the two
flag scans, lookup_compact and lookup_assign of csrc/plonk_kernels.hip): key sets, orders of the input column, the
reference, a second judge written from the definition, and a Python copy of the launch rule. No GPU in here:
tests/test_lookup_permute_cases.py checks this module on the CPU, tests/test_gpu_lookup_permute.py runs it on the device.

All keys are canonical integers below r; the interface takes Montgomery form (zkutil.ints_to_fr converts). A case is
(name, inp, tab): `inp` the input multiset over u usable rows in ascending order, `tab` the table's u usable rows.
`ORDERS` rearranges `inp`; the expected A' and S' do not depend on the order."""
import os
import random
import sys

import zkutil as zu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import plonk_ref as PR  # noqa: E402

R = zu.R
SIZES = [2, 4, 8, 32, 64, 128, 256, 512, 2048, 4096, 16384]
SORT_TILE = 2048  # plonk_kernels.hip
INPUT_PAD = R - 1  # rows >= usable of every input column: the largest key there is
TABLE_PAD = (5 << 160) | 0xDEAD  # rows >= usable of every table column: a value no key set, filler or multiset holds


def limb(x, i):
    return (x >> (32 * i)) & 0xFFFFFFFF


def from_limbs32(ls):
    return sum(v << (32 * i) for i, v in enumerate(ls))


def filler(t):
    """Distinct values outside every key set below."""
    return (7 << 96) | (0xF1110000 + t)


# ------------------------------------------------------------------------------ key sets
def _ladder_pairs():
    """(i, j, low, high) for limb positions i < j: low has limb i = 2 and limb j = 1, high has limb i = 1 and limb j = 2.
    Limb j alone decides low < high; a comparator that ranks limb i above limb j, or walks the limbs upwards, says high < low."""
    out = []
    for i in range(8):
        for j in range(i + 1, 8):
            lo, hi = [0] * 8, [0] * 8
            lo[i], lo[j] = 2, 1
            hi[i], hi[j] = 1, 2
            out.append((i, j, from_limbs32(lo), from_limbs32(hi)))
    return out


LADDER_PAIRS = _ladder_pairs()
LADDER_CARRIES = [v for i in range(1, 8) for v in ((1 << (32 * i)) - 1, 1 << (32 * i))]  # all ones below limb i against limb i = 1


def _sign_pairs():
    """(i, low, high) for limbs 0...6: limb i is 0x7FFFFFFF in low and 0x80000000 in high, every other limb is 1 in both. As
    signed 32-bit numbers the two limbs compare the other way round."""
    out = []
    for i in range(7):
        base = [1] * 8
        lo, hi = list(base), list(base)
        lo[i], hi[i] = 0x7FFFFFFF, 0x80000000
        out.append((i, from_limbs32(lo), from_limbs32(hi)))
    return out


SIGN_PAIRS = _sign_pairs()
KEY_SETS = {
    "limb_ladder": [v for _, _, lo, hi in LADDER_PAIRS for v in (hi, lo)] + LADDER_CARRIES,  # 56 + 14 keys, pairs adjacent
    "sign_bits": [v for _, lo, hi in SIGN_PAIRS for v in (hi, lo)],
    "edges": [0, 1, R - 1, R - 2, (R >> 232 << 232) - 1, 1 << 253],
}


def signed_limb_less(a, b):
    """key_less with every limb read as a signed 32-bit number: the defect `sign_bits` is for."""
    s = lambda v: v - (1 << 32) if v & 0x80000000 else v
    for i in range(7, -1, -1):
        if limb(a, i) != limb(b, i):
            return s(limb(a, i)) < s(limb(b, i))
    return False


# ------------------------------------------------------------------------------ multisets over u usable rows
def _shuffled(vals, seed):
    vals = list(vals)
    random.Random(seed).shuffle(vals)
    return vals


def key_set_cases(name, u):
    """The key set `name` in chunks of at most u keys, each padded with distinct fillers to u rows: every input value once,
    the table the same set in a shuffled order. A' = S' = the sorted set: these cases are about the comparator, in the
    sort and in lookup_mark's binary search."""
    keys = KEY_SETS[name]
    out = []
    for c, at in enumerate(range(0, len(keys), u)):
        chunk = keys[at:at + u]
        vals = chunk + [filler(t) for t in range(u - len(chunk))]
        out.append(("%s[%d]" % (name, c), sorted(vals), _shuffled(vals, 1000 + c)))
    return out


def zero_one_splits(u):
    return sorted({s for s in (0, 1, u // 2, u - 1, u) if 0 <= s <= u})


def zero_one_case(u, split):
    """`split` zeros, then u - split ones; the table holds the values present once and distinct fillers."""
    inp = [0] * split + [1] * (u - split)
    present = sorted(set(inp))
    return "zero_one[%d]" % split, inp, _shuffled(present + [filler(t) for t in range(u - len(present))], 2000 + split)


# tests/test_gpu_plonk_ops.py: MULTISETS, for every u >= 1 (the same lists wherever those are defined, u >= 6)
MULTISETS = {
    "all_equal": lambda u: ([5] * u, [5] + list(range(100, 100 + u - 1))),
    "many_leftovers": lambda u: ([3, 3, 3, 9, 9, 1] * (u // 6) + [1] * (u % 6), ([1, 3, 9] + list(range(1000, 1000 + max(0, u - 3))))[:u]),
    "table_with_repeats": lambda u: ([i % 3 for i in range(u)], ([0, 1, 2] + [0] * max(0, u - 3))[:u]),
}


def multiset_case(name, u):
    inp, tab = MULTISETS[name](u)
    return name, sorted(inp), tab


def cases(u):
    """Every case over u >= 1 usable rows."""
    out = []
    for name in KEY_SETS:
        out += key_set_cases(name, u)
    out += [zero_one_case(u, s) for s in zero_one_splits(u)]
    out += [multiset_case(name, u) for name in MULTISETS]
    return out


def default_usable(n):
    """The usable rows the sizes run at: n - 6 as in the prover where that is positive, else n - 1 and n."""
    return [n - 6] if n > 6 else [n - 1, n]


# ------------------------------------------------------------------------------ orders of the input column
def _bit_reversed(u):
    bits = max(1, (u - 1).bit_length())
    rev = lambda i: int(format(i, "0%db" % bits)[::-1], 2)
    return [rev(i) for i in range(1 << bits) if rev(i) < u]


ORDERS = {
    # u -> the index into the ascending multiset that each row of the column takes
    "ascending": lambda u: list(range(u)),
    "descending": lambda u: list(range(u - 1, -1, -1)),
    "bit_reversed": _bit_reversed,
    "organ_pipe": lambda u: list(range(0, u, 2)) + list(range(1, u, 2))[::-1],
    "shuffle": lambda u: _shuffled(range(u), 77),
}


def ordered(inp, order):
    return [inp[i] for i in ORDERS[order](len(inp))]


# ------------------------------------------------------------------------------ the two judges
class ZeroRng:
    def fr(self):
        return 0


def reference(inp, tab, usable):
    """oracle/plonk_ref.py: permute_expression_pair with zero blinding rows (bf + 1 = 0), as tests/test_gpu_plonk_ops.py:
    ref_permute. AssertionError when an input is not in the table."""
    return PR.permute_expression_pair(list(inp), list(tab), usable, -1, ZeroRng())


def check_definition(inp, tab, usable, a, s):
    """None if (a, s) is the permuted pair of the first `usable` rows of (inp, tab) by the definition, else what is wrong."""
    if list(a) != sorted(inp[:usable]):
        return "A' is not the sorted input"
    if len(s) != usable or sorted(s) != sorted(tab[:usable]):
        return "S' is not a permutation of the table"
    rest = []
    for r in range(usable):
        if r == 0 or a[r] != a[r - 1]:
            if s[r] != a[r]:
                return "row %d starts a run of equal inputs and S' != A' there" % r
        else:
            rest.append(s[r])
    rest.reverse()
    for i in range(1, len(rest)):
        if rest[i - 1] > rest[i]:
            return "the repeated rows, read from the last to the first, do not hold the leftovers in ascending order"
    return None


# ------------------------------------------------------------------------------ the launch rule
def launch_plan(n, usable, nlookups):
    """{kernel name: launches} of one amdzk_permute_expression_pair_dev call: zk_sort_keys2 and zk_lookup_permute
    (plonk_kernels.hip), whatever the number of columns."""
    if nlookups == 0 or usable == 0:
        return {}
    tile = min(n, SORT_TILE)
    lds, glob, k = 1, 0, 2 * tile
    while k <= n:
        j = k // 2
        while j >= tile:
            glob += 1
            j //= 2
        lds += 1
        k *= 2
    plan = {"sort_bitonic_lds": lds, "lookup_mark": 1, "lookup_flag_scan": 2, "lookup_compact": 1, "lookup_assign": 1}
    if glob:
        plan["sort_bitonic_global"] = glob
    return plan
