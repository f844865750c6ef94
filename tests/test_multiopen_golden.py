"""CPU: the recorded oracle output of the 9000-query GWC case (tests/golden/multiopen_caps_gwc.bin, used by
test_gpu_multiopen.py) is what plonk_ref.gwc_prove computes. GWC's v is the first challenge of a fresh transcript and W_z
depends on v and on z's own queries only, so the oracle run on the queries of a few points gives exactly those points'
commitments of the full run; the full run is `python tests/multiopen_cases.py --write-golden`."""
import random

from multiopen_cases import PR, caps_golden, make_case


def test_recorded_gwc_commitments_are_the_oracles():
    case = make_case("caps")
    proof, nxt = caps_golden()
    sample = sorted(random.Random(5).sample(range(3000), 6)) + [2999]
    sub = [(p, z) for p, z in case.queries if z in sample]  # original order: points come out in ascending index order
    assert len(sub) == 3 * len(sample)
    points, _bytes, _next = case.oracle("gwc", queries=sub)
    assert [PR.g1_compress(p) for p in points] == [proof[32 * z:32 * z + 32] for z in sample]
    # the recorded next challenge is the transcript's state behind v and all 3000 recorded points
    T = PR.Blake2bRead(proof)
    T.squeeze_challenge()
    for _ in range(3000):
        T.read_point()
    assert T.squeeze_challenge() == nxt
