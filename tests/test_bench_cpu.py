"""bench.py's driver contract on the CPU (gloo): a plain ``python bench.py --gpus N`` launches the
N ranks itself and rank 0 reports the whole job; a job whose world differs from --gpus fails
loudly; the synthetic corpora (index/synth.py) have the shapes the realistic search benchmarks
rely on."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--opt", "device=cpu", "--steps", "2", "--warmup", "1", "--index-rows", "6000", "--batch",
        "4", "--seq", "12", "--opt", "heldout_searches=3"]


def _run(args, env_extra=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(OMP_NUM_THREADS="2", **(env_extra or {}))
    p = subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=400)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p, [json.loads(ln) for ln in lines]


def test_bench_self_launches_n_ranks():
    p, out = _run(["--gpus", "2", "--full"] + TINY)
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(out) == 1, p.stdout          # exactly one JSON line, from rank 0 ...
    assert p.stdout.strip().splitlines() == [json.dumps(out[0])], p.stdout   # ... and nothing else
    r = out[0]
    assert r["n_gpus"] == 2 and r["world"] == 2 and r["backend"] == "gloo"
    assert r["comm_check"]["collective"].startswith("all_gather ok")
    assert r["config"]["global_batch"] == 8 and r["config"]["parallelism"] == "dp2+index_shard2"
    assert r["value"] > 0 and r["steps"] == 2 and r["warmup"] == 1
    # --full: the realistic (held-out query) search rate rides in the same line
    assert r["heldout_searches"] == 3 and r["heldout_topk_qps"] > 0 and r["heldout_ms_per_search"] > 0


def test_bench_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """Without --full the run times its steps and nothing more (no held-out phase), --steps sets
    the number of timed steps, and --dump-outputs writes the last step's arrays as float .npy
    files that a second run with the same arguments reproduces exactly."""
    import numpy as np

    runs = []
    for name in ("a", "b"):
        p, out = _run(["--gpus", "1", "--dump-outputs", str(tmp_path / name)] + TINY)
        assert p.returncode == 0, p.stderr[-2000:]
        assert len(out) == 1, p.stdout
        runs.append(out[0])
    r = runs[0]
    assert r["steps"] == 2 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - 4 * 1000.0 / r["ms_per_step"]) / r["value"] < 0.01
    assert not [k for k in r if k.startswith("heldout_")]
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["embeddings.npy", "topk_ids.npy", "topk_scores.npy", "unit_embeddings.npy"]
    shapes = {"embeddings.npy": (4, 384), "unit_embeddings.npy": (4, 384),
              "topk_scores.npy": (4, 10), "topk_ids.npy": (4, 10)}
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == shapes[n], (n, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.array_equal(a, b), n
    # self queries are upserted before they are searched: every best score is the query's own
    # row's (or a near-duplicate's), 1 up to the bf16 rounding of the stored unit rows; the ids
    # name rows of the shard (6000 corpus rows + 3 steps of 4)
    s, ids = np.load(tmp_path / "a" / "topk_scores.npy"), np.load(tmp_path / "a" / "topk_ids.npy")
    assert np.abs(s[:, 0] - 1.0).max() < 2.0 ** -6 and (np.diff(s, axis=1) <= 0).all()
    assert (ids == np.floor(ids)).all() and ids.min() >= 0 and ids.max() < 6012


def test_bench_world_mismatch_fails():
    # a launcher-provided world of 1 with --gpus 2 must not report a 1-rank number as 2 GPUs
    p, out = _run(["--gpus", "2"] + TINY, env_extra={"WORLD_SIZE": "1", "RANK": "0",
                                                     "LOCAL_RANK": "0"}, drop=())
    assert p.returncode != 0 and not out
    assert "refusing" in p.stderr


def test_bench_simulated_world_is_labelled_a_projection():
    """--simulate-world N runs the per-rank work of the N-GPU step on ONE rank (a 1/N shard,
    N x batch gathered queries, the result exchange through a single-rank group): its JSON can
    never pass for an N-GPU measurement -- the metric says SIMULATED, n_gpus and world stay 1,
    and the N-GPU numbers sit in the simulated_* / projected_* fields only."""
    p, out = _run(["--opt", "simulate_world=4"] + TINY)
    assert p.returncode == 0, p.stderr[-2000:]
    r = out[0]
    assert r["metric"].startswith("SIMULATED 4-GPU") and "projection" in r["metric"]
    assert r["n_gpus"] == 1 and r["world"] == 1 and r["simulated"] is True
    assert r["simulated_world"] == 4 and r["config"]["simulated_world"] == 4
    assert r["config"]["index_rows_per_rank"] == 1500 and r["config"]["global_batch"] == 16
    assert "simulated" in r["config"]["parallelism"]
    assert r["value"] == r["projected_job_rate"] > 0
    # and it refuses to pose as a multi-rank run
    p2, out2 = _run(["--opt", "simulate_world=4", "--gpus", "2"] + TINY)
    assert p2.returncode != 0 and not out2


def test_bench_search_clustered_heldout_two_ranks():
    p, out = _run(["--gpus", "2", "--mode", "search", "--corpus", "clustered", "--opt",
                   "clusters=50", "--queries", "heldout"] + TINY)
    assert p.returncode == 0, p.stderr[-2000:]
    r = out[0]
    assert r["n_gpus"] == 2 and r["config"]["corpus"] == "clustered"
    assert r["config"]["queries"] == "heldout" and "held-out" in r["data"]


def test_bench_help_lists_at_most_15_options():
    """The headline's knobs stay few (VERDICT r4 housekeeping): the secondary ones live under
    --opt KEY=VALUE and an unknown key fails loudly.  The two switches of the driver contract,
    --full and --dump-outputs, configure no workload and are not counted among the 15."""
    p = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0
    opts = {ln.split()[0].rstrip(",") for ln in p.stdout.splitlines()
            if ln.startswith("  -") and not ln.startswith("  -h")}
    assert {"--full", "--dump-outputs"} <= opts, sorted(opts)
    assert len(opts - {"--full", "--dump-outputs"}) <= 15, sorted(opts)
    bad = subprocess.run([sys.executable, "bench.py", "--opt", "nope=1"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "expected KEY=VALUE" in bad.stderr


def test_synthetic_corpora_shapes():
    from codename_symbiont_amd.index.synth import CorpusGen

    g = CorpusGen("clustered", 384, "cpu", clusters=20, spread=0.6)
    x = g.unit(2000, seed=3)
    # every row sits near one of the shared centers: cos ~ 1/sqrt(1 + 0.36) = 0.857
    best = (x @ g.centers.t()).max(dim=1).values
    assert float(best.mean()) == pytest.approx(0.857, abs=0.03)
    assert torch.equal(g.rows(100, 9), g.rows(100, 9))          # reproducible per seed
    a = CorpusGen("anisotropic", 384, "cpu").unit(1000, seed=1)
    c = a @ a.t()
    off = c[~torch.eye(1000, dtype=torch.bool)]
    assert float(off.mean()) == pytest.approx(0.3, abs=0.05)
    r = CorpusGen("random", 384, "cpu").unit(1000, seed=1)
    assert abs(float((r @ r.t())[~torch.eye(1000, dtype=torch.bool)].mean())) < 0.01
