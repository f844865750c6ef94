"""GPU: the two newest features together — the later phases of a whole batch computed by witness programs run inside the
batch's phase callback (amdzk_witness_run from amdzk_batch_phase_fn), the challenges among the programs' inputs.

Three-phase rlc_circuit at k = 5, B = 3: the phase-1 cells r = a + ch * b and the phase-2 cells s = r * ch2 + ch * a[row + 1]
of all three proofs are ONE amdzk_witness_run each (one compiled program per phase, no zero fill). The device's columns
equal the circuit's own `fill`, and the proofs equal the phased harness's."""
import numpy as np
import pytest
import zkutil as zu

import batch_opts_util as U
import phased_circuits as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plonk(pkg):
    return __import__("anon_aadhaar_halo2_amd.halo2.plonk", fromlist=["x"])


def phase_programs(W, c):
    """Inputs of both: a[0 .. u], b[0 .. u), ch (and ch2). Columns: a, b, r, s = 0 .. 3."""
    u, progs = c.usable, {}
    for phase in (1, 2):
        p = W(c.k, 4)
        a = [p.input() for _ in range(u + 1)]
        b = [p.input() for _ in range(u)]
        ch = p.input()
        ch2 = p.input() if phase == 2 else None
        for row in range(u):
            r = p.add(a[row], p.mul(ch, b[row]))
            if phase == 1:
                p.assign(r, 2, row)
            else:
                p.assign(p.add(p.mul(r, ch2), p.mul(ch, a[row + 1])), 3, row)
        progs[phase] = p
    return progs


def test_later_phases_of_a_batch_from_witness_programs(ctx, pkg, plonk, oracle, monkeypatch):
    c = PC.rlc_circuit(plonk, 5, seed=6, three_phases=True)
    assert c.desc["advice_column_phase"] == [0, 0, 1, 2] and c.desc["challenge_phase"] == [0, 1]
    B = U.Batch(ctx, pkg, plonk, oracle, 5, [(c, None), (c, 111), (c, 112)])
    progs = phase_programs(pkg.witness.WitnessProgram, c)
    compiled = {phase: p.compile(ctx) for phase, p in progs.items()}
    u, runs = c.usable, []

    def synthesize(phase, wanted, chal, stream):
        assert list(wanted) == [1, 1, 1]
        B.calls.append((phase, wanted.copy(), chal.copy()))
        inputs = []
        for b, m in enumerate(B.m):
            words = zu.ints_to_fr(oracle, m.adv0[0][: u + 1] + m.adv0[1][:u])
            inputs.append(np.concatenate([words, chal[b, :phase]]))
        compiled[phase].run(inputs, B.d_adv, publics=False)  # the whole batch's cells of this phase: one run
        runs.append(phase)

    seeds = [41, 42, 43]
    got = B.batch(seeds, synthesize=synthesize)
    assert runs == [1, 2]
    chs = [B.challenges(b) for b in range(3)]
    for b, m in enumerate(B.m):  # what `fill` computes on the host, for the device's columns and for the harness
        for phase in (1, 2):
            m.fill(phase, dict(enumerate(chs[b])), m.adv)
        dev = B.d_adv[b].download((4, c.n, 4))
        assert np.array_equal(dev, np.stack([zu.ints_to_fr(oracle, col) for col in m.adv])), "proof %d: the device's columns" % b
    B.check_calls([0, 1, 2])
    for b in range(3):
        assert got[b] == B.expected(monkeypatch, b, seeds[b], chs[b]), "proof %d" % b
    assert len(set(got)) == 3
    for cw in compiled.values():
        cw.free()
    B.free()
