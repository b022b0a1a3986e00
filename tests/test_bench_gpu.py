"""bench.py contract on the GPU box: one JSON line with the fields the driver reads, in every store / launch mode
(tiny shapes; the numbers mean nothing here)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline"]


def run_bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--small", "--blocks", "2", "--steps", "3", "--warmup", "2",
           "--n-store", "30000", "--gcn-k", "16", "--k", "32", "--tokens-per-sample", "32", "--settle-s", "0.05", *extra]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29611")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("extra", [(), ("--force-exchange",), ("--force-exchange", "--shard-vals", "--layers", "2"),
                                   ("--graph", "--no-cpu-baseline"), ("--precision", "bf16x6", "--no-cpu-baseline")])
def test_bench_contract(extra):
    r = run_bench("--full", *extra)
    for k in REQUIRED:
        assert k in r, k
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 2 and r["higher_is_better"] is True
    assert r["unit"] == "tokens/s" and r["value"] > 0 and r["vs_baseline"] is None and r["scaling"] == "weak"
    assert "workload" in r["config"]
    # the timed region follows an untimed settle phase; per-step HIP-event times ride beside the wall-clock mean
    assert r["settle"]["steps"] >= 20 and len(r["settle"]["chunks_ms_per_step"]) >= 2
    assert r["ms_per_step_min"] <= r["ms_per_step_median"] <= r["ms_per_step_max"]
    assert r["ms_per_step_median"] <= r["ms_per_step"] * 1.5 and "sclk_mhz_timed_region" in r
    roof = r["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["bound"] in ("hbm", "mfma") and 0 <= roof["frac"] <= 1.0
    if "--no-cpu-baseline" not in extra:
        cb = r["cpu_baseline"]
        assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "tokens/s" and cb["sample"]


def test_bench_search_inside_the_step():
    """The default mode of the bench at a reduced store: the IVF-PQ search of every step's own queries runs on the device inside the
    timed step (`value`), checked against the float64 oracle first; the search-given figure rides beside it; one lane and three
    lanes (batches in flight on separate streams) add up the same scores."""
    common = ("--n-store", "3000000", "--blocks", "4", "--steps", "4", "--warmup", "3", "--gcn-k", "16", "--k", "64", "--settle-s", "0.05",
              "--full", "--no-cpu-baseline", "--no-extras", "--search-check", "8")
    out = {}
    for lanes in ("1", "3"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *common, "--lanes", lanes]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        r = out[lanes] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        assert r["value_includes_search"] is True and r["value"] > 0 and r["value_search_given"] > r["value"]
        ks = r["config"]["knn_search"]
        assert ks["where"].startswith("on the device") and ks["lanes"] == int(lanes) and ks["parity"]["ok"] is True
        assert ks["pairs_per_query"] > 0 and r["roofline"]["bound"] in ("hbm", "mfma")
        assert any(k_["kernel"].startswith("ivfpq_scan8") for k_ in r["kernels"])
    assert out["1"]["config"]["synthetic_ppl"] == out["3"]["config"]["synthetic_ppl"]
    # the same steps with the range-sharded store's exchange forced through RCCL (one rank): rows prefetched on the fetch stream, two
    # batches in flight on their lanes -- the same scores
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *common, "--lanes", "2", "--force-exchange"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29617"))
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert r["config"]["knn_search"]["lanes"] == 2 and r["config"]["store"].startswith("range-sharded") and r["config"]["collective_backend"] == "nccl"
    assert r["config"]["synthetic_ppl"] == out["1"]["config"]["synthetic_ppl"]


def test_bench_plain_run_is_lean(tmp_path):
    """A plain run (no --full) sets up, warms up, times its steps, dumps and prints the headline line: no parity gates, search-given
    leg, sub-benchmarks or CPU baseline.  It computes what the same run with --full computes: the same score sum and dumped outputs."""
    import numpy as np
    common = ("--n-store", "3000000", "--blocks", "4", "--steps", "3", "--warmup", "3", "--gcn-k", "16", "--k", "64", "--settle-s", "0.05",
              "--search-check", "8")
    out = {}
    for name, extra in (("plain", ()), ("full", ("--full", "--no-cpu-baseline", "--no-extras"))):
        d = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), *common, *extra, "--dump-outputs", str(d)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout
        out[name] = json.loads(lines[0]), {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    (r, files), (rf, files_f) = out["plain"], out["full"]
    for k in REQUIRED:
        assert k in r, k
    assert r["value"] > 0 and r["value_includes_search"] is True and r["steps"] == 3 and r["warmup"] == 3
    for k in ("parity", "cpu_baseline", "recipe_L3", "driver_path", "knn_search"):
        assert k not in r, k
    assert r["value_search_given"] is None and r["config"]["knn_search"]["parity"] is None
    assert rf["value_search_given"] > 0 and rf["parity"]["max_abs_dlogp_vs_oracle"] < 1e-4 and rf["config"]["knn_search"]["parity"]["ok"] is True
    assert r["config"]["synthetic_ppl"] == rf["config"]["synthetic_ppl"]
    assert sorted(files) == sorted(files_f)
    for k in files:
        assert np.array_equal(files[k], files_f[k]), k


def test_bench_modes_agree():
    """The sharded-store exchange and the HIP-graph replay reproduce the direct path's score sum."""
    a = run_bench("--no-cpu-baseline")
    b = run_bench("--no-cpu-baseline", "--force-exchange")
    c = run_bench("--no-cpu-baseline", "--graph")
    assert a["config"]["synthetic_ppl"] == b["config"]["synthetic_ppl"] == c["config"]["synthetic_ppl"]


@pytest.mark.parametrize("extra", [(), ("--layers", "2"), ("--shard-vals", "--exchange", "exact"),
                                   ("--exchange", "peer", "--layers", "2"), ("--exchange", "peer", "--shard-vals")])
def test_bench_two_ranks_on_one_gpu(extra):
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank), with both ranks on
    device 0 and the collectives staged through the host (gloo): the sharded code path of the bench -- halo shards with
    matching boundary rows, fetch stream, padded / exact exchange, the replicated-store comparison, the max-over-ranks
    timing and the score reduction -- runs with a real second rank.  L = 2 goes through the halo layout."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29613", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--small", "--blocks", "2", "--steps", "3",
           "--warmup", "2", "--n-store", "30000", "--gcn-k", "16", "--k", "32", "--tokens-per-sample", "32", "--full", "--no-cpu-baseline",
           "--settle-s", "0.05", *extra]
    env = dict(os.environ, GNNLM_BENCH_BACKEND="gloo", GNNLM_BENCH_DEVICE="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout                                   # rank 0 prints, once
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["value"] > 0 and r["scaling"] == "weak"
    c = r["config"]
    # the transport is named for what it is: gloo staged through the host moved no byte over RCCL / xGMI
    assert c["collective_backend"] == "gloo" and c["rccl_ranks"] == 0 and "xgmi_bytes_per_step_per_rank" not in c
    assert c["store"].startswith("range-sharded") and "host-staged" in c["store"] and c["exchange_bytes_per_step_per_rank_host_staged"] > 0
    if "--shard-vals" not in extra:                                    # (the comparison run needs the full label table)
        assert c["replicated_store"]["tokens_per_s"] > 0


def test_bench_two_ranks_search_inside_the_step():
    """The driver's scaling run in miniature: `bench.py --gpus 2` at real model shapes (reduced store), range-sharded graph store with
    the exchange, and every rank's OWN replica of the kNN index searched inside its timed step (weak scaling: no collective on the
    search).  Both ranks on device 0 over gloo."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--n-store", "3000000", "--blocks", "4", "--steps", "3", "--warmup", "3",
           "--gcn-k", "16", "--k", "64", "--settle-s", "0.05", "--full", "--no-cpu-baseline", "--no-extras", "--search-check", "8"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GNNLM_BENCH_BACKEND="gloo", GNNLM_BENCH_DEVICE="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    c = r["config"]
    assert r["n_gpus"] == 2 and r["value"] > 0 and r["value_includes_search"] is True and r["scaling"] == "weak"
    assert c["knn_search"]["where"].startswith("on the device") and c["knn_search"]["lanes"] == 2 and c["knn_search"]["parity"]["ok"] is True   # (two batches in flight on every rank, as at N = 1; the exchange stays on its own stream)
    assert c["store"].startswith("range-sharded") and c["collective_backend"] == "gloo" and c["rccl_ranks"] == 0


def test_bench_plain_launch_starts_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher around it (what the driver's scaling run types): the script starts the two
    ranks itself as child processes, relays rank 0's one JSON line and the exit code.  Both ranks on device 0 over gloo."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--small", "--blocks", "2", "--steps", "3", "--warmup", "2",
           "--n-store", "30000", "--gcn-k", "16", "--k", "32", "--tokens-per-sample", "32", "--full", "--no-cpu-baseline", "--settle-s", "0.05"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GNNLM_BENCH_BACKEND="gloo", GNNLM_BENCH_DEVICE="0")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["value"] > 0 and r["config"]["rccl_ranks"] == 0 and r["config"]["collective_backend"] == "gloo"
    assert r["config"]["exchange_bytes_per_step_per_rank_host_staged"] > 0 and r["config"]["replicated_store"]["tokens_per_s"] > 0
    # more ranks than GPUs without the one-GPU test transport: refused before anything is launched
    env.pop("GNNLM_BENCH_BACKEND")
    p = subprocess.run(cmd[:2] + ["--gpus", "64", "--small"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 2 and "GPU(s) are visible" in p.stderr


def test_bench_two_ranks_merge_before_the_exchange():
    """`--layers 3 --ids searched` on two ranks (one-GPU transport): equal context groups are merged on the device BEFORE the
    exchange, so a rank asks its peers for every distinct centre row once -- the bytes on the links fall with the merge factor
    (reported: config.merged_groups), the exact and the fixed-capacity exchange and the peer-mapped store agree on the score."""
    res = {}
    for ex in ("exact", "padded", "peer"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--small", "--blocks", "2", "--steps", "3", "--warmup", "3",
               "--n-store", "30000", "--gcn-k", "16", "--k", "32", "--tokens-per-sample", "32", "--no-cpu-baseline", "--settle-s", "0.05",
               "--layers", "3", "--ids", "searched", "--exchange", ex]
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        env.update(GNNLM_BENCH_BACKEND="gloo", GNNLM_BENCH_DEVICE="0")
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        res[ex] = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    c = res["exact"]["config"]
    mg = c["merged_groups"]
    n_all, n_req = mg["context_groups_per_step"], mg["distinct_requested_per_step_mean"]
    assert n_all == 2 * 32 * 16 and 0 < n_req < 0.8 * n_all                     # searched neighbours repeat (1.45x on this tiny corpus; 2.6x at the bench's size)
    unmerged = int(n_all / 2) * 2 * (8 + 5 * 16)                                # one request per group, halo layout (M = 16)
    assert c["exchange_bytes_per_step_per_rank_host_staged"] <= unmerged * (n_req / n_all) * 1.05
    # fixed-capacity buckets: sized from the distinct count measured in the warm-up (x 1.15 + 1024, agreed by a MAX all-reduce) and never
    # above the worst case -- at this toy size the constants decide, at the bench's size the count does
    from gnnlm_amd.dist import bucket_capacity
    assert res["padded"]["config"]["exchange_bytes_per_step_per_rank_host_staged"] <= bucket_capacity(n_all, 2) * 2 * (8 + 5 * 16)
    assert len({r["config"]["synthetic_ppl"] for r in res.values()}) == 1


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs: the last timed step's outputs as float32 / float64 files, 64 MB at most.  With one pooled batch every step scores
    the same tokens, so the dumped logp must give the run's own score sum (synthetic_ppl): search on the device with two batches in
    flight, several streams, the HIP-graph replay.  The same arguments with another --steps time that many steps and dump the same files."""
    import numpy as np

    def run(name, *extra):
        d = tmp_path / name
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--warmup", "2", "--settle-s", "0.05", "--no-cpu-baseline", "--no-extras",
               "--pool", "1", "--dump-outputs", str(d), *extra]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
        files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64_000_000
        n = r["config"]["blocks_per_step_per_gpu"] * r["config"]["tokens_per_block"]
        assert files["logp"].shape == (n,) and files["lm_logp"].shape == (n,)
        ppl = float(np.exp(-files["logp"].astype(np.float64).mean()))
        assert abs(ppl - r["config"]["synthetic_ppl"]) <= 1e-4 + 1e-6 * ppl, (ppl, r["config"]["synthetic_ppl"])
        return r, files
    search = ("--n-store", "3000000", "--blocks", "4", "--gcn-k", "16", "--k", "64", "--search-check", "8", "--lanes", "2")
    r3, a = run("steps3", *search, "--steps", "3")
    r5, b = run("steps5", *search, "--steps", "5")
    assert r3["steps"] == 3 and r5["steps"] == 5 and r3["config"]["knn_search"]["lanes"] == 2
    assert {"logp", "lm_logp", "p_knn", "recall", "gcn_feat", "knn_sims", "knn_ids", "knn_vals", "rows"} <= set(a) and sorted(a) == sorted(b)
    rows = a["rows"].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[-1] < 4 * 256 and a["knn_ids"].shape == (len(rows), 64) and a["gcn_feat"].shape[0] == len(rows)
    for k_ in a:
        assert np.array_equal(a[k_], b[k_]), k_
    small = ("--small", "--blocks", "2", "--n-store", "30000", "--gcn-k", "16", "--k", "32", "--tokens-per-sample", "32", "--steps", "3")
    run("graph", *small, "--graph")
    run("streams", *small, "--streams", "2")
