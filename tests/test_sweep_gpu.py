"""The kNN-LM tuning sweep (ks x temperatures x lmbdas from one forward, one search, one read of the search result), from the
kernel to the driver.  GPU only.

Bars: a grid point with 0 < lmbda < 1 is the single-setting kernel's result on the prefix columns BIT FOR BIT; against the
reference's golden vectors and the CPU oracle the bars are those of the single-setting tests (test_kernels_gpu.py).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import knn as oknn


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from gnnlm_amd import ops as _ops
    return _ops


def full_size_inputs(k):
    """The inputs of test_knn_interp_full_size (test_kernels_gpu.py): -1 ids in every fifth row, half of the targets hit."""
    rs = np.random.RandomState(8)
    n, N, V = 256, 200000, 267744
    vals = rs.randint(0, V, size=N).astype(np.int32)
    ids = rs.randint(0, N, size=(n, k)).astype(np.int64)
    ids[::5, -3:] = -1
    sims = np.sort(rs.uniform(0.2, 0.9, size=(n, k)).astype(np.float32), axis=1)[:, ::-1].copy()
    targets = np.where(rs.rand(n) < 0.5, vals[ids[:, 2]], rs.randint(0, V, size=n)).astype(np.int64)
    lm = np.log(rs.uniform(1e-4, 1, size=n)).astype(np.float32)
    return lm, sims, ids, targets, vals


KS, TS, LS = [1, 64, 65, None], [1.0, 0.1, 0.01], [0.0, 0.1, 0.25, 1.0]


@pytest.mark.parametrize("labels", ["knn_vals", "table_i32", "table_i16"])
@pytest.mark.parametrize("k", [1024, 200, 70])
def test_grid_equals_single_setting_kernel(ops, dev, k, labels):
    """Every grid point == ops.knn_interp on the contiguous prefix, torch.equal (logp where 0 < l < 1; p_knn and recall always);
    l = 0 rows == lm_logp exactly; l = 1 rows == torch.log(p_knn + 1e-10) to 1 ulp; nothing is NaN or infinite.

    Observed on the MI355X: the l = 1 rows are within 1 ulp of torch.log, not all equal to it (equal in 769 .. 1280 of the 3072
    entries of a case: the library's logf and torch's log do not round alike); the count is printed."""
    lm, sims, ids, targets, vals = full_size_inputs(k)
    if labels == "table_i16":
        vals = (vals % 30000).astype(np.int16)
        targets = np.where(np.arange(len(targets)) % 2 == 0, vals[ids[:, 2]], targets % 30000).astype(np.int64)
    lm_d, sims_d, ids_d, tg_d = (torch.from_numpy(a).to(dev) for a in (lm, sims, ids, targets))
    vals_d = torch.from_numpy(vals).to(dev)
    # labels delivered with the neighbours: vals[ids] with numpy's wrap of -1 to the last row (knn_model.py:198)
    kv_d = torch.from_numpy(vals[ids].astype(np.int32)).to(dev)
    by = dict(knn_vals=kv_d) if labels == "knn_vals" else dict(vals=vals_d)
    ks = sorted({min(v or k, k) for v in KS})
    out, pk, rec = ops.knn_interp_grid(lm_d, sims_d, ids_d, tg_d, ks, TS, LS, **by)
    assert out.shape == (len(ks) * len(TS) * len(LS), 256) and pk.shape == (len(ks) * len(TS), 256) and rec.shape == (len(ks), 256)
    assert torch.isfinite(out).all() and torch.isfinite(pk).all()
    points = ops.grid_points(ks, TS, LS)
    exact_l1 = total_l1 = 0
    for g, (kp, t, l) in enumerate(points):
        ik, it = ks.index(kp), TS.index(t)
        pre = dict(knn_vals=kv_d[:, :kp].contiguous()) if labels == "knn_vals" else dict(vals=vals_d)
        one = ops.knn_interp(lm_d, sims_d[:, :kp].contiguous(), ids_d[:, :kp].contiguous(), tg_d, t, l if 0 < l < 1 else 0.5,
                             vals_tag=False, **pre)
        assert torch.equal(pk[ik * len(TS) + it], one[1]), (kp, t)
        assert torch.equal(rec[ik], one[2]), kp
        if 0 < l < 1:
            assert torch.equal(out[g], one[0]), (kp, t, l)
        elif l == 0.0:
            assert torch.equal(out[g], lm_d), (kp, t)
        else:
            want = torch.log(one[1] + 1e-10)
            ulp = (out[g].view(torch.int32) - want.view(torch.int32)).abs()
            exact_l1 += int((ulp == 0).sum())
            total_l1 += ulp.numel()
            assert int(ulp.max()) <= 1, (kp, t, int(ulp.max()))
    print(f"k={k} {labels}: l = 1 rows equal torch.log(p_knn + 1e-10) exactly in {exact_l1} of {total_l1} entries, the rest within 1 ulp")
    # k' < k against the oracle on the prefix columns, at the bars of test_knn_interp_full_size
    for kp in ks:
        for t in (1.0, 0.01):
            p_ref, rec_ref = oknn.knn_target_prob(sims[:, :kp], ids[:, :kp], vals, targets, t)
            ik, it = ks.index(kp), TS.index(t)
            assert np.array_equal(rec[ik].cpu().numpy(), rec_ref.numpy())
            np.testing.assert_allclose(pk[ik * len(TS) + it].cpu().numpy(), p_ref.numpy(), rtol=5e-5, atol=1e-7)
            for l in (0.1, 0.25):
                ref = oknn.combine_knn_and_vocab_probs(p_ref, torch.from_numpy(lm), l)
                np.testing.assert_allclose(out[points.index((kp, t, l))].cpu().numpy(), ref.numpy(), rtol=2e-5, atol=5e-6)


@pytest.mark.parametrize("metric_type", ["do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2"])
def test_grid_golden_knn(ops, dev, golden, metric_type):
    """tests/golden/knn.npz: one grid call per tag with both temperatures and lmbda 0.25, at the bars of test_knn_interp_golden."""
    g = golden("knn")
    for cosine in (False, True):
        tags = {t: f"{metric_type}.{'cos' if cosine else 'raw'}.t{t}" for t in (1.0, 0.01)}
        tag = tags[1.0]
        # (the search result does not depend on the temperature: both tags hold the same dists / ids)
        assert np.array_equal(g[tags[1.0] + ".ids"], g[tags[0.01] + ".ids"]) and np.array_equal(g[tags[1.0] + ".dists"], g[tags[0.01] + ".dists"])
        q = oknn.normalize_queries(torch.from_numpy(g["queries"]), cosine)
        sims = oknn.sims_from_search(g[tag + ".dists"], g[tag + ".ids"], q, metric_type, g["keys"], cosine).float()
        n, k = sims.shape
        lm = torch.log(torch.linspace(0.01, 0.9, n))
        out, pk, rec = ops.knn_interp_grid(lm.to(dev), sims.contiguous().to(dev), torch.from_numpy(g[tag + ".ids"]).to(dev),
                                           torch.from_numpy(g["targets"]).to(dev), [k], [1.0, 0.01], [0.25], vals=torch.from_numpy(g["vals"]).reshape(-1).contiguous().to(dev))
        for it, t in enumerate((1.0, 0.01)):
            np.testing.assert_allclose(pk[it].cpu().numpy(), g[tags[t] + ".p"], rtol=2e-5, atol=1e-7)
            assert np.array_equal(rec[0].cpu().numpy(), g[tags[t] + ".recall"])
            ref = oknn.combine_knn_and_vocab_probs(torch.from_numpy(g[tags[t] + ".p"]), lm, 0.25)
            np.testing.assert_allclose(out[it].cpu().numpy(), ref.numpy(), rtol=2e-5, atol=2e-6)


def test_grid_golden_combine(ops, dev, golden):
    """tests/golden/combine.npz fed as test_combine_golden feeds it; the four lambdas are ONE grid call."""
    g = golden("combine")
    lm, pk = g["lm_logp"].reshape(-1), g["p_knn"].reshape(-1)
    keep = (pk > 0) & (pk < 1)
    sims = np.stack([np.log(pk[keep]), np.log1p(-pk[keep])], 1).astype(np.float32)
    ids = np.tile(np.array([[0, 1]], dtype=np.int64), (keep.sum(), 1))
    vals = np.array([5, 6], dtype=np.int32)
    tg = np.full(keep.sum(), 5, dtype=np.int64)
    lmbs = (0.1, 0.15, 0.2, 0.25)
    out, p, _ = ops.knn_interp_grid(torch.from_numpy(lm[keep]).to(dev), torch.from_numpy(sims).to(dev), torch.from_numpy(ids).to(dev),
                                    torch.from_numpy(tg).to(dev), [2], [1.0], lmbs, vals=torch.from_numpy(vals).to(dev))
    np.testing.assert_allclose(p[0].cpu().numpy(), pk[keep], rtol=1e-5)
    for il, lmb in enumerate(lmbs):
        np.testing.assert_allclose(out[il].cpu().numpy(), g[f"mix.{lmb}"].reshape(-1)[keep], rtol=3e-5, atol=3e-6)


@pytest.mark.parametrize("n", [1, 1023, 1025, 32768])
def test_rows_sum_f64(ops, dev, n):
    """Each of 75 rows == ops.masked_sum_f64 of that row exactly; the call accumulates."""
    x = torch.randn(75, n, generator=torch.Generator().manual_seed(n)).to(dev) * 7
    out = torch.zeros(75, dtype=torch.float64, device=dev)
    ops.rows_sum_f64(x, out)
    want = torch.cat([ops.masked_sum_f64(x[g].contiguous()) for g in range(75)])
    assert torch.equal(out, want)
    ops.rows_sum_f64(x, out)
    assert torch.equal(out, 2 * want)


def test_grid_refusals(ops, dev):
    """An error with a message, nothing launched (the outputs of a refused call do not exist: the call raises)."""
    from gnnlm_amd._lib import GnnlmError
    lm, sims, ids, targets, vals = full_size_inputs(70)
    a = [torch.from_numpy(v).to(dev) for v in (lm, sims, ids, targets)]
    vals_d = torch.from_numpy(vals).to(dev)
    ok = ops.knn_interp_grid(*a, [70], [1.0], [0.5], vals=vals_d)
    assert ok[0].shape == (1, 256)
    big = full_size_inputs(1500)
    with pytest.raises(GnnlmError, match="1024"):
        ops.knn_interp_grid(*[torch.from_numpy(v).to(dev) for v in big[:4]], [8], [1.0], [0.5], vals=vals_d)
    for ks, ts, ls, msg in (([1, 2, 3, 4, 5, 6, 7, 8, 9], [1.0], [0.5], "values of k"),
                            ([8], [1.0 + 0.1 * j for j in range(17)], [0.5], "temperatures"),
                            ([8], [1.0], [j / 16 for j in range(17)], "lmbdas"),
                            ([71], [1.0], [0.5], "k'"), ([0], [1.0], [0.5], "k'"),
                            ([8], [0.0], [0.5], "temperature"), ([8], [1.0], [1.5], "lmbda"), ([8], [1.0], [-0.1], "lmbda")):
        with pytest.raises(GnnlmError, match=msg):
            ops.knn_interp_grid(*a, ks, ts, ls, vals=vals_d)
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.knn_interp_grid(*[torch.from_numpy(v) for v in (lm, sims, ids, targets)], [8], [1.0], [0.5], vals=torch.from_numpy(vals))
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.rows_sum_f64(torch.zeros(3, 5), torch.zeros(3, dtype=torch.float64))
    with pytest.raises(GnnlmError, match="need vals"):
        ops.knn_interp_grid(*a, [8], [1.0], [0.5])
    torch.cuda.synchronize()


def _knn_args(data, k, temp, lam):
    return ["--knnlm", "--k", str(k), "--lmbda", str(lam), "--dstore-dir", str(data / "train_dstore"),
            "--index-file", str(data / "train_dstore" / "faiss_store.cosine"), "--temperature", str(temp), "--knn-sim-func", "ip"]


SWEEP = ["--sweep-lmbda", "0,0.1,0.25", "--sweep-temperature", "1.0,0.1", "--sweep-k", "4,8"]


@pytest.mark.parametrize("extra", [[], ["--batch-blocks", "0"], ["--batch-blocks", "4"], ["--batch-blocks", "0", "--streams", "3"],
                                   ["--gcn-context-window", "5"]],
                         ids=["default", "batch-blocks-0", "batch-blocks-4", "streams-3", "gcn-context-window-5"])
def test_eval_lm_sweep(dev, tmp_path, capsys, extra):
    """One sweep run against one plain run per grid point (make_data_dir's directory, the kNN arguments of test_eval_lm_end_to_end)."""
    from gnnlm_amd import eval_lm
    from test_mirrors_gpu import make_data_dir
    c = make_data_dir(tmp_path)
    data, T, n_test = c["data"], c["T"], c["n_test"]
    base1 = list(c["base"])
    base1[base1.index("--max-tokens") + 1] = str(T)
    if "--gcn-context-window" in extra:                    # (as test_eval_lm_gcn_context_window sets it up)
        base1[base1.index("--gcn-context-window") + 1] = "5"
        base1[base1.index("--max-tokens") + 1] = str(T + 5)
        extra = []
    lam, temp, k = 0.25, 1.0, 8
    capsys.readouterr()
    plain = eval_lm.cli_main(base1 + _knn_args(data, k, temp, lam) + extra)
    assert "sweep" not in plain
    plain_lines = capsys.readouterr().out.strip().split("\n")
    assert len(plain_lines) == 2
    res = eval_lm.cli_main(base1 + _knn_args(data, k, temp, lam) + extra + SWEEP)
    lines = capsys.readouterr().out.strip().split("\n")
    # (a) the run's own figures do not move
    assert res["score_sum"] == plain["score_sum"] and res["count"] == plain["count"] == n_test and res["ppl"] == plain["ppl"]
    # (d) the two reference lines first, then one line per point
    # ("Evaluated N tokens": N counts the context prefixes of --gcn-context-window too, as in the plain run)
    assert lines[0].startswith("Evaluated ") and lines[0].split(" in ")[0] == plain_lines[0].split(" in ")[0]
    assert lines[1] == plain_lines[1] and lines[1].startswith("Loss (base 2): ")
    assert len(lines) == 14 and all(l_.startswith("sweep k=") for l_ in lines[2:]) and sum(l_.endswith("<- best") for l_ in lines) == 1
    assert lines[2:] == eval_lm.sweep_lines(res["sweep"])
    # (b) every entry against a separate plain run at that setting
    assert [(r["k"], r["temperature"], r["lmbda"]) for r in res["sweep"]] == \
        [(k_, t_, l_) for k_ in (4, 8) for t_ in (1.0, 0.1) for l_ in (0.0, 0.1, 0.25)]
    lm_only = eval_lm.cli_main(base1 + extra)
    for r in res["sweep"]:
        one = lm_only if r["lmbda"] == 0.0 else eval_lm.cli_main(base1 + _knn_args(data, r["k"], r["temperature"], r["lmbda"]) + extra)
        bar = (1e-6 if r["k"] == k else 2e-4) * n_test
        print(r, one["score_sum"], abs(r["score_sum"] - one["score_sum"]))
        assert abs(r["score_sum"] - one["score_sum"]) < bar, (r, one["score_sum"])
        assert abs(r["ppl"] - 2 ** (-r["score_sum"] / n_test / np.log(2))) < 1e-9
        if (r["k"], r["temperature"], r["lmbda"]) == (k, temp, lam):
            assert r["score_sum"] == res["score_sum"]
    # --lmbda 0 with a sweep: the search still runs, the headline figure is the LM's
    # (against the run without --knnlm at the bar between batchings: that run groups its batches and lanes in its own way)
    res0 = eval_lm.cli_main(base1 + _knn_args(data, k, temp, 0.0) + extra + SWEEP)
    assert abs(res0["score_sum"] - lm_only["score_sum"]) < 1e-6 * n_test
    assert [r["score_sum"] for r in res0["sweep"]] == [r["score_sum"] for r in res["sweep"]]
    assert res0["sweep"][0]["score_sum"] == res0["score_sum"]


def test_engine_sweep(ops, dev):
    """GnnLmEngine.score(..., sweep=...): out["logp"] unchanged bit for bit, out["sweep_logp"] rows == ops.knn_interp per point
    (search-given path), and the search-inside path (knn_index=) the same from its own search result."""
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=1, k=32, seed=1)
    eng, batch = build_engine(prob, dev), to_batch(prob["block"], dev)
    sweep = ([5, 32], [1.0, 0.1], [0.0, 0.25, 1.0])
    base = eng.score(batch, 0.25, 1.0)
    out = eng.score(batch, 0.25, 1.0, sweep=sweep)
    assert torch.equal(out["logp"], base["logp"]) and torch.equal(out["lm_logp"], base["lm_logp"])
    assert out["sweep_logp"].shape == (12, batch.targets.shape[0])
    for g, (kp, t, l) in enumerate(ops.grid_points(*sweep)):
        if 0 < l < 1:
            one = ops.knn_interp(out["lm_logp"], batch.knn_sims[:, :kp].contiguous(), batch.knn_ids[:, :kp].contiguous(), batch.targets, t, l,
                                 vals=eng.store.vals, n_store=eng.store.n_store, vals_tag=False)[0]
            assert torch.equal(out["sweep_logp"][g], one)
        elif l == 0.0:
            assert torch.equal(out["sweep_logp"][g], out["lm_logp"])
    assert torch.equal(out["sweep_logp"][ops.grid_points(*sweep).index((32, 1.0, 0.25))], base["logp"])
    only = eng.score(batch, 0.0, 1.0, sweep=sweep)                       # lmbda 0: logp stays the LM's, the grid is still there
    assert torch.equal(only["logp"], base["lm_logp"]) and torch.equal(only["sweep_logp"], out["sweep_logp"])

    # the search inside the step: an index with the device-search contract (search_begin -> handle.result() -> sims, ids, labels)
    class Found:
        def __init__(self, r):
            self.r = r

        def result(self):
            return self.r

    class Index:
        calls = 0

        def search_begin(self, q, k, return_vals=True):
            Index.calls += 1
            kv = eng.store.vals[torch.where(batch.knn_ids < 0, batch.knn_ids + eng.store.n_store, batch.knn_ids)].int()
            return Found((batch.knn_sims[:, :k].contiguous(), batch.knn_ids[:, :k].contiguous(), kv[:, :k].contiguous()))

    inside = eng.score(batch, 0.25, 1.0, knn_index=Index(), k=32, sweep=sweep)
    assert Index.calls == 1                                              # ONE search feeds the setting and the grid
    assert torch.equal(inside["logp"], base["logp"]) and torch.equal(inside["sweep_logp"], out["sweep_logp"])
    inside0 = eng.score(batch, 0.0, 1.0, knn_index=Index(), k=32, sweep=sweep)
    assert Index.calls == 2 and torch.equal(inside0["logp"], base["lm_logp"]) and torch.equal(inside0["sweep_logp"], out["sweep_logp"])


def test_eval_lm_sweep_two_ranks(dev, tmp_path):
    """The sweep in a multi-process run (two ranks on device 0, collectives staged through the host, as
    test_eval_lm_multi_process_sharded_store runs them): the G sums travel in the run's one all_reduce, rank 0 alone prints the
    table, and every point equals the single-process sweep to the last bits float64 addition order allows."""
    import json
    import os
    import subprocess
    import sys
    from test_mirrors_gpu import make_data_dir
    c = make_data_dir(tmp_path, n_test=100, L=1)
    base = list(c["base"])
    base[base.index("--max-tokens") + 1] = str(c["T"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")

    def run(extra, ranks, port):
        out = str(tmp_path / f"res_{port}.json")
        cmd = [sys.executable] + (["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                                   "--master-port", str(port)] if ranks > 1 else []) + \
            ["-m", "gnnlm_amd.eval_lm"] + base + _knn_args(c["data"], 8, 1.0, 0.25) + SWEEP + extra + ["--result-json", out]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root, env=dict(env, GNNLM_EVAL_BACKEND="gloo", GNNLM_EVAL_DEVICE="0"))
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        return [l_ for l_ in p.stdout.splitlines() if l_.startswith(("Evaluated", "Loss", "sweep"))], json.load(open(out))
    one_lines, one = run([], 1, 0)
    assert len(one_lines) == 14 and len(one["sweep"]) == 12
    for i, extra in enumerate([["--store", "sharded"], ["--store", "replicated"]]):
        lines, res = run(extra, 2, 29690 + i)
        assert lines[1:] == one_lines[1:], (extra, lines, one_lines)       # the table, once, byte for byte
        assert res["world"] == 2 and res["count"] == 100
        for a, b in zip(res["sweep"], one["sweep"]):
            assert (a["k"], a["temperature"], a["lmbda"]) == (b["k"], b["temperature"], b["lmbda"])
            assert abs(a["score_sum"] - b["score_sum"]) <= 1e-12 * abs(b["score_sum"])


@pytest.mark.parametrize("metric_type", ["do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2"])
def test_knn_model_interpolate_grid(ops, dev, golden, tmp_path, metric_type):
    """KNNModel.interpolate_grid over the recorded searches of tests/golden/knn.npz, all four sim funcs, raw and cosine: p_knn / recall
    of the full k at test_knn_model_golden's bars, and every point == KNNModel.interpolate at that (k', t, l) -- which searches with
    k' itself -- bit for bit.  The split form (interpolate_begin, search_finish, two consumers) gives the same."""
    from gnnlm_amd.knn_model import KNNModel
    from test_mirrors_gpu import FixedIndex, write_dstore
    g = golden("knn")
    write_dstore(str(tmp_path / "d"), g["keys"], g["vals"].astype(np.int16), 50)
    q = torch.from_numpy(g["queries"]).to(dev)
    tg = torch.from_numpy(g["targets"]).to(dev)
    lm = torch.log(torch.linspace(0.01, 0.9, q.shape[0])).to(dev)
    ks, ts, ls = [3, 8], [1.0, 0.01], [0.0, 0.25, 1.0]
    for cosine in (False, True):
        tag = f"{metric_type}.{'cos' if cosine else 'raw'}"
        m = KNNModel("faiss_store.cosine" if cosine else "faiss_store.ip", str(tmp_path / "d"), k=8, metric_type=metric_type,
                     index=FixedIndex(g[tag + ".t1.0.dists"], g[tag + ".t1.0.ids"]), device=dev)
        out, pk, rec = m.interpolate_grid(q, tg, lm, ks, ts, ls)
        for it, t in enumerate(ts):
            np.testing.assert_allclose(pk[1 * len(ts) + it].cpu().numpy(), g[f"{tag}.t{t}.p"], rtol=3e-5, atol=1e-7)
            assert np.array_equal(rec[1].cpu().numpy(), g[f"{tag}.t{t}.recall"])
        for gi, (kp, t, l) in enumerate(ops.grid_points(ks, ts, ls)):
            if 0 < l < 1:
                one = m.interpolate(q, tg, lm, t, l, k=kp)
                assert torch.equal(out[gi], one[0]) and torch.equal(pk[ks.index(kp) * len(ts) + ts.index(t)], one[1]) and torch.equal(rec[ks.index(kp)], one[2])
            elif l == 0.0:
                assert torch.equal(out[gi], lm)
        found = m.search_finish(m.interpolate_begin(q))
        again = m.interpolate_grid_finish(found, tg, lm, ks, ts, ls)
        single = m.interpolate_finish(found, tg, lm, 0.01, 0.25)
        assert all(torch.equal(a, b) for a, b in zip(again, (out, pk, rec)))
        assert torch.equal(single[0], out[ops.grid_points(ks, ts, ls).index((8, 0.01, 0.25))])
