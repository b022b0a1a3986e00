"""Exact kNN-LM similarities (`--knn-sim-func ip | l2`, knn_model.py:161-175) recomputed from the stored keys by one HIP kernel,
from the kernel to the driver.  GPU only.

Bars.  The kernel against float64: per case `max |kernel - f64| <= 2 x max |oracle_f32 - f64| + ulp32(max |f64|)`, where the
oracle is `oracle.knn.sims_from_search`, the reference's own float32 arithmetic (pinned by tests/golden/knn.npz), over the same
inputs: the bar was set for two float32 sums of d terms in different orders (factor 2; on small cases the oracle's error can be a
single rounding: the one-ulp floor).  The kernel sums in float64 and rounds once, so its error is at most half an ulp32 of the result
and the bar holds in every case, the single-result ones included.  Independence is `torch.equal`.  End to end: perplexity within 0.02.
"""
import dataclasses
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import knn as oknn

FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from gnnlm_amd import ops as _ops
    return _ops


def sims_f64(q, keys, ids, metric, normalize, chunk=8):
    """Float64 restatement of knn_model.py:161-175 on the device (ids already wrapped into [0, n_rows))."""
    n, k = ids.shape
    out = torch.empty(n, k, dtype=torch.float64, device=q.device)
    qd = q.double()
    for r0 in range(0, n, chunk):
        v = keys[ids[r0:r0 + chunk]].double()
        qq = qd[r0:r0 + chunk, None, :]
        if metric == "l2":
            out[r0:r0 + chunk] = -((qq - v) ** 2).sum(-1)
        else:
            s = (v * qq).sum(-1)
            out[r0:r0 + chunk] = s / (v ** 2).sum(-1).sqrt() if normalize else s
    return out


def padded(t, pad):
    """The same values behind a row stride `pad` elements wider than the row."""
    buf = torch.zeros(t.shape[0], t.shape[1] + pad, dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


MODES = [("ip", False), ("ip", True), ("l2", False)]


@pytest.mark.parametrize("d", [16, 64, 100, 1024])
@pytest.mark.parametrize("key_dtype", ["fp16", "f32"])
@pytest.mark.parametrize("metric,normalize", MODES, ids=["ip", "ip-cosine", "l2"])
def test_kernel_against_float64(ops, dev, metric, normalize, key_dtype, d):
    """k in {1, 8, 1000, 1024} x n in {0, 1, 257} per case; strides wider than the rows on every operand, repeated ids, ids of -1
    (== row n_rows - 1, bit for bit), one id out of range (-FLT_MAX, the rest of the row untouched by it).

    The two errors are printed per case (run with -s); the d = 1024 ones are in DESIGN.md section 7.7."""
    n_rows = 5000
    gen = torch.Generator().manual_seed(1000 * d + 10 * len(metric) + normalize)
    keys_h = torch.randn(n_rows, d, generator=gen)
    keys_h = keys_h.half() if key_dtype == "fp16" else keys_h
    keys_d = padded(keys_h.to(dev), 8)
    for k in (1, 8, 1000, 1024):
        for n in (0, 1, 257):
            q_h = torch.randn(n, d, generator=gen)
            ids_h = torch.randint(0, n_rows, (n, k), generator=gen)
            if n:
                if k > 1:
                    ids_h[:, -1] = ids_h[:, 0]                      # a repeated id in every row
                ids_h[0, 0] = -1
                ids_h[n // 2, k // 2] = -1
            oor = (n - 1, k - 1) if n > 1 or k > 1 else None        # the 1 x 1 case keeps its one entry for the -1
            ids_bad = ids_h.clone()
            if n and oor:
                ids_bad[oor] = n_rows + 7 if k % 2 else -n_rows - 1
            q_d, ids_d = padded(q_h.to(dev), 5), padded(ids_bad.to(dev), 2)
            out = padded(torch.full((n, k), 7.0, device=dev), 3)
            got = ops.knn_recompute_sims(q_d, ids_d, keys_d, metric, normalize, out=out)
            assert got.data_ptr() == out.data_ptr() and got.shape == (n, k)
            if n == 0:
                continue
            assert torch.all(out._base[:, k:] == 0), "the padding of out was written"
            wrapped = torch.where(ids_h < 0, ids_h + n_rows, ids_h)
            again = ops.knn_recompute_sims(q_d, wrapped.to(dev), keys_d, metric, normalize)
            keep = torch.ones(n, k, dtype=torch.bool, device=dev)
            if oor:
                assert float(got[oor]) == -FLT_MAX
                keep[oor] = False
            assert torch.equal(got[keep], again[keep]), "an id of -1 must read row n_rows - 1"
            ref64 = sims_f64(q_h.to(dev), keys_h.to(dev), wrapped.to(dev), metric, normalize)
            orc = oknn.sims_from_search(np.zeros((n, k), np.float32), ids_h.numpy(), q_h, metric, keys_h.numpy(), normalize).to(dev)
            err = float((got.double() - ref64)[keep].abs().max())
            err_oracle = float((orc.double() - ref64)[keep].abs().max())
            floor = float(np.spacing(np.float32(ref64[keep].abs().max().item())))
            print(f"resim {metric}{'-cosine' if normalize else ''} {key_dtype} d={d} k={k} n={n}: |kernel - f64| = {err:.3e}  "
                  f"|oracle - f64| = {err_oracle:.3e}  ulp32 = {floor:.3e}")
            assert err <= 2 * err_oracle + floor, (metric, normalize, key_dtype, d, k, n, err, err_oracle, floor)


@pytest.mark.parametrize("d", [64, 100, 1024, 2500])
@pytest.mark.parametrize("key_dtype", ["fp16", "f32"])
@pytest.mark.parametrize("metric,normalize", MODES, ids=["ip", "ip-cosine", "l2"])
def test_result_depends_on_its_two_rows_only(ops, dev, metric, normalize, key_dtype, d):
    """torch.equal: columns [:, :k'] of a k call against a k' call; a slice of the queries against the full call; direct mode over
    keys[ids] against indexed mode; keys (and queries) with a padded row stride -- 16-byte aligned rows and not -- against contiguous."""
    n_rows, n, k = 3000, 70, 200
    gen = torch.Generator().manual_seed(d)
    keys = torch.randn(n_rows, d, generator=gen)
    keys = (keys.half() if key_dtype == "fp16" else keys).to(dev)
    q = torch.randn(n, d, generator=gen).to(dev)
    ids = torch.randint(0, n_rows, (n, k), generator=gen).to(dev)
    ids[3, 5] = -1
    full = ops.knn_recompute_sims(q, ids, keys, metric, normalize)
    assert torch.isfinite(full).all()
    for kp in (1, 3, 64, 65, 199):
        assert torch.equal(ops.knn_recompute_sims(q, ids[:, :kp].contiguous(), keys, metric, normalize), full[:, :kp]), kp
        assert torch.equal(ops.knn_recompute_sims(q, ids[:, :kp], keys, metric, normalize), full[:, :kp]), kp      # a view of ids
    for sl in (slice(0, 1), slice(13, 41), slice(69, 70)):
        assert torch.equal(ops.knn_recompute_sims(q[sl], ids[sl], keys, metric, normalize), full[sl]), sl
    rows = keys[torch.where(ids < 0, ids + n_rows, ids)]                      # [n, k, d]: what the host-gather path stages
    assert torch.equal(ops.knn_recompute_sims(q, None, rows, metric, normalize), full)
    assert torch.equal(ops.knn_recompute_sims(q, None, rows.view(n * k, d), metric, normalize), full)
    for pad in (8, 3, 1):
        assert torch.equal(ops.knn_recompute_sims(q, ids, padded(keys, pad), metric, normalize), full), pad
        assert torch.equal(ops.knn_recompute_sims(padded(q, pad), ids, keys, metric, normalize), full), pad
    # keys that start 2 / 4 bytes into an allocation: the element-wise loads, the same sums
    flat = torch.zeros(n_rows * d + 1, dtype=keys.dtype, device=dev)
    flat[1:] = keys.reshape(-1)
    assert torch.equal(ops.knn_recompute_sims(q, ids, flat[1:].view(n_rows, d), metric, normalize), full)


def test_offsets_beyond_4_gib(ops, dev):
    """An fp16 table of 2.4 M x 1024 (4.9 GB; the last tenth of its rows lies wholly beyond 4 GiB): ids from that tenth, against float64 on the rows copied to the host."""
    n_rows, d, n, k = 2_400_000, 1024, 64, 128
    keys = torch.empty(n_rows, d, dtype=torch.float16, device=dev)
    gen = torch.Generator(device=dev).manual_seed(3)
    for r0 in range(0, n_rows, 100_000):
        keys[r0:r0 + 100_000].normal_(generator=gen)
    assert keys.numel() * 2 > 4 << 30
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(n_rows - n_rows // 10, n_rows, (n, k), generator=g)
    ids[0, 0], ids[1, 1] = -1, n_rows - 1
    q = torch.randn(n, d, generator=g)
    wrapped = torch.where(ids < 0, ids + n_rows, ids)
    uniq, inv = torch.unique(wrapped, return_inverse=True)
    rows_h = keys[uniq.to(dev)].cpu()                                         # the sample: every row the ids name
    assert int((uniq.double() * d * 2).min()) > 4 << 30
    for metric, normalize in MODES:
        got = ops.knn_recompute_sims(q.to(dev), ids.to(dev), keys, metric, normalize).cpu()
        ref64 = sims_f64(q, rows_h, inv, metric, normalize)
        orc = oknn.sims_from_search(np.zeros((n, k), np.float32), inv.numpy(), q, metric, rows_h.numpy(), normalize)
        err, err_oracle = float((got.double() - ref64).abs().max()), float((orc.double() - ref64).abs().max())
        floor = float(np.spacing(np.float32(ref64.abs().max().item())))
        print(f"resim beyond 4 GiB {metric}{'-cosine' if normalize else ''}: |kernel - f64| = {err:.3e}  |oracle - f64| = {err_oracle:.3e}")
        assert err <= 2 * err_oracle + floor
        assert torch.equal(got[0, 0], ops.knn_recompute_sims(q[:1].to(dev), ids[1:2, 1:2].to(dev), keys, metric, normalize).cpu()[0, 0])
    del keys
    torch.cuda.empty_cache()


def test_refusals(ops, dev):
    from gnnlm_amd._lib import GnnlmError
    q, ids = torch.randn(4, 16, device=dev), torch.zeros(4, 8, dtype=torch.int64, device=dev)
    keys = torch.randn(50, 16, device=dev).half()
    assert ops.knn_recompute_sims(q, ids, keys, "ip").shape == (4, 8)
    with pytest.raises(GnnlmError, match="l2 never normalises"):
        ops.knn_recompute_sims(q, ids, keys, "l2", normalize_keys=True)
    with pytest.raises(GnnlmError, match="metric"):
        ops.knn_recompute_sims(q, ids, keys, 2)
    with pytest.raises(TypeError):
        ops.knn_recompute_sims(q, ids.int(), keys, "ip")
    with pytest.raises(TypeError):
        ops.knn_recompute_sims(q, ids, keys.bfloat16(), "ip")
    with pytest.raises(ValueError):
        ops.knn_recompute_sims(q, None, keys[:30], "ip")                     # direct mode: 30 rows are not n * k
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.knn_recompute_sims(q.cpu(), ids.cpu(), keys.cpu(), "ip")
    torch.cuda.synchronize()


class ReplayIndex:
    """Replays a recorded search (faiss contract: host arrays); carries the key table in HBM as an exact index does."""

    def __init__(self, dists, ids, keys):
        self.d, self.i, self.keys = dists, ids, keys

    def search(self, q, k):
        return self.d[:, :k], self.i[:, :k]


def write_dstore(path, keys, vals, vocab, fp16=True):
    os.makedirs(path, exist_ok=True)
    if keys is not None:
        keys.tofile(os.path.join(path, "keys.npy"))
    vals.tofile(os.path.join(path, "vals.npy"))
    json.dump({"dstore_size": len(vals), "hidden_size": 1024 if keys is None else keys.shape[1], "vocab_size": vocab, "dstore_fp16": fp16,
               "val_size": 1}, open(os.path.join(path, "info.json"), "w"))


def test_no_nkd_temporaries_at_the_drivers_batch(dev, tmp_path):
    """KNNModel.interpolate(metric_type="ip") on a replayed search at n = 32768, k = 1024, d = 1024 over a 1 M-row fp16 store: it
    completes and the peak of allocated memory rises by less than 64 n k bytes (2 GiB) -- nothing proportional to d."""
    from gnnlm_amd.knn_model import KNNModel
    n, k, d, n_rows, V = 32768, 1024, 1024, 1 << 20, 30000
    rs = np.random.RandomState(0)
    write_dstore(str(tmp_path / "d"), None, rs.randint(0, V, n_rows).astype(np.int16), V)
    keys = torch.empty(n_rows, d, dtype=torch.float16, device=dev).normal_(generator=torch.Generator(device=dev).manual_seed(1))
    ids = rs.randint(0, n_rows, (n, k)).astype(np.int64)
    ids[::7, -2:] = -1
    dists = np.zeros((n, k), dtype=np.float32)
    m = KNNModel("faiss_store.cosine", str(tmp_path / "d"), k=k, metric_type="ip", no_load_keys=True,
                 index=ReplayIndex(dists, ids, keys), device=dev)
    q = torch.randn(n, d, device=dev)
    tg = torch.randint(0, V, (n,), device=dev)
    lm = torch.log(torch.rand(n, device=dev) * 0.9 + 0.01)
    m.vals_device()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    logp, p, rec = m.interpolate(q, tg, lm, 1.0, 0.25)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f"interpolate(ip) at n={n} k={k} d={d}: peak rise {rise / 2 ** 20:.0f} MiB (bar {64 * n * k / 2 ** 20:.0f} MiB; 10 n k d = {10 * n * k * d / 2 ** 30:.0f} GiB)")
    assert rise < 64 * n * k
    assert torch.isfinite(logp).all() and logp.shape == (n,)
    # a few rows against float64
    qn = q[:4] / (q[:4] ** 2).sum(-1, keepdim=True).sqrt()
    m4 = KNNModel("faiss_store.cosine", str(tmp_path / "d"), k=k, metric_type="ip", no_load_keys=True,
                  index=ReplayIndex(dists[:4], ids[:4], keys), device=dev)
    sims = m4.search_sims(q[:4])[0]
    idw = torch.from_numpy(np.where(ids[:4] < 0, ids[:4] + n_rows, ids[:4])).to(dev)
    ref = sims_f64(qn, keys, idw, "ip", True)
    assert float((sims.double() - ref).abs().max()) < 1e-5
    del keys, m, m4
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def produced(tmp_path_factory):
    """test_pipeline_from_raw_keys's directory: raw key tables -> quantize_features -> run_index_build -> find_knn, every producer this
    repo's own, plus a checkpoint."""
    from gnnlm_amd import find_knn, quantize_features, run_index_build
    from gnnlm_amd.synthetic import make_problem
    tmp_path = tmp_path_factory.mktemp("resim")
    d, H, M, dsub, V, kg, T, L, k = 64, 4, 16, 4, 600, 6, 16, 2, 32
    n_train, n_test = 6000, 41
    prob = make_problem(n_store=n_train, d=d, n_heads=H, M=M, dsub=dsub, vocab=V, cutoff=[100, 300], T=n_test, kg=kg,
                        left=2, right=2, n_layers=L, k=8, seed=5)
    rs = np.random.RandomState(9)
    centres = rs.randn(30, d).astype(np.float32)
    train_keys = (centres[rs.randint(0, 30, n_train)] + 0.5 * rs.randn(n_train, d)).astype(np.float16)
    test_keys = (centres[rs.randint(0, 30, n_test)] + 0.5 * rs.randn(n_test, d)).astype(np.float16)
    targets = np.maximum(prob["block"]["targets"], 4)
    data = tmp_path / "data-bin"
    write_dstore(str(data / "train_dstore"), train_keys, prob["vals"].astype(np.int16), V)
    write_dstore(str(data / "test_dstore"), test_keys, targets.astype(np.int16), V)
    quantize_features.main(quantize_features.get_parser().parse_args(
        ["--data-dir", str(data), "--subset", "train", "--index", f"OPQ{M}_{d},,PQ{M}", "--code-size", str(M), "--chunk-size", "6000",
         "--pq-iters", "6", "--opq-iters", "3"]))
    run_index_build.main(run_index_build.get_parser().parse_args(
        ["--dstore-dir", str(data / "train_dstore"), "--index-type", f"OPQ{M}_{d},IVF32,PQ{M}", "--metric", "cosine", "--nprobe", "8"]))
    find_knn.main(find_knn.get_parser().parse_args(["--data-dir", str(data), "--subset", "test", "--k", str(kg), "--nprobe", "8"]))
    nbrs = np.array(np.memmap(str(data / "test_dstore" / f"neighbors.mmap.{kg}"), dtype=np.int64, mode="r", shape=(n_test, kg)))
    sd = {"decoder.hgt_decoder." + k_: v for k_, v in prob["sd"].items()}
    w = prob["asm"]
    for i, e in enumerate(w["emb"]):
        sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = e
        if i:
            sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = w["proj"][i]
    sd["decoder.adaptive_softmax.head.class_proj.weight"] = w["class_proj"]
    margs = Namespace(decoder_embed_dim=d, decoder_attention_heads=H, graph_layer=L, decoder_gcn_dim=d,
                      adaptive_softmax_cutoff="100,300", orig_prob_ratio=0.0, short_cut=False, quantizer_path="")
    torch.save({"args": margs, "model": sd}, str(tmp_path / "ckpt.pt"))
    base = [str(data), "--path", str(tmp_path / "ckpt.pt"), "--gen-subset", "test", "--graph", "--neighbor-context", "2", "--gcn-k", str(kg),
            "--use-precompute-feat", "--sample-break-mode", "none", "--max-tokens", str(T), "--tokens-per-sample", str(T),
            "--gcn-context-window", "0", "--knn-keytype", "gcn_feat", "--model-overrides",
            "{'orig_prob_ratio': 0.0, 'quantizer_path': '%s'}" % str(data / "quantizer"),
            "--knnlm", "--k", str(k), "--dstore-dir", str(data / "train_dstore"),
            "--index-file", str(data / "train_dstore" / "faiss_store.cosine"), "--probe", "8"]
    return dict(prob=prob, data=data, base=base, train_keys=train_keys, test_keys=test_keys, targets=targets, nbrs=nbrs, w=w,
                d=d, H=H, L=L, T=T, k=k, n_train=n_train, n_test=n_test)


@pytest.mark.parametrize("metric_type", ["ip", "l2"])
def test_model_two_phase(dev, produced, metric_type):
    """Over an IVFPQIndex with the labels attached, `ip` / `l2` take the pending path, and finishing the handle equals the synchronous
    call bit for bit; search_sims and the dense variant see the same similarities."""
    from gnnlm_amd.knn_model import KNNModel
    c = produced
    m = KNNModel(str(c["data"] / "train_dstore" / "faiss_store.cosine"), str(c["data"] / "train_dstore"), probe=8, k=c["k"],
                 metric_type=metric_type, use_memory=True, device=dev)
    assert getattr(m.index, "has_vals", False) and hasattr(m.index, "search_begin")
    assert "HBM" in m.keys_home()
    q = torch.from_numpy(c["test_keys"].astype(np.float32)).to(dev)
    tg = torch.from_numpy(c["targets"]).to(dev)
    lm = torch.log(torch.linspace(0.01, 0.9, q.shape[0])).to(dev)
    h = m.interpolate_begin(q)
    assert h[0] == "pending"
    two = m.interpolate_finish(h, tg, lm, 1.0, 0.25)
    one = m.interpolate(q, tg, lm, 1.0, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(two, one))
    sims, knns = m.search_sims(q)
    qn = q / (q ** 2).sum(-1, keepdim=True).sqrt()
    want = oknn.sims_from_search(np.zeros(tuple(knns.shape), np.float32), knns.cpu().numpy(), qn.cpu(), metric_type, c["train_keys"], True)
    np.testing.assert_allclose(sims.cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(m.search_finish(m.interpolate_begin(q))[2][0], sims)
    dense, masked, _ = m.get_knn_prob(q, return_knn=True)
    assert torch.equal(masked, sims.masked_fill(knns == -1, -1e10))
    # the default sim func is what it was: the index's own distances
    m0 = KNNModel(str(c["data"] / "train_dstore" / "faiss_store.cosine"), str(c["data"] / "train_dstore"), probe=8, k=c["k"],
                  no_load_keys=True, device=dev)
    d0, i0 = m0.search_sims(q)
    assert torch.equal(i0, knns) and not torch.equal(d0, sims)


@pytest.mark.parametrize("sim_func", ["ip", "l2"])
def test_eval_lm_end_to_end(dev, produced, capsys, caplog, sim_func):
    """eval_lm --knnlm --knn-sim-func ip | l2 against oracle.pipeline fed with oracle.knn.sims_from_search over the SAME produced
    files: perplexity within 0.02; with the sweep flags the point at the run's own setting equals score_sum exactly."""
    import logging
    from gnnlm_amd import eval_lm
    from gnnlm_amd.faiss_io import read_pq_quantizer
    from oracle import ivfpq as oivf, pipeline
    c = produced
    lam, temp = 0.25, 1.0
    cmd = c["base"] + ["--lmbda", str(lam), "--temperature", str(temp), "--knn-sim-func", sim_func]
    capsys.readouterr()
    with caplog.at_level(logging.INFO):
        res = eval_lm.cli_main(cmd)
    lines = capsys.readouterr().out.strip().split("\n")
    assert len(lines) == 2 and lines[0].startswith("Evaluated ") and lines[1].startswith("Loss (base 2): ")
    assert sum("similarities recomputed from the keys in HBM" in r.getMessage() for r in caplog.records) == 1
    lit = eval_lm.cli_main(cmd + ["--batch-blocks", "0"])                    # one-block batches on six streams, searches in flight
    assert lit["count"] == res["count"] and abs(lit["score_sum"] - res["score_sum"]) <= 1e-9 * abs(res["score_sum"])
    q = read_pq_quantizer(str(c["data"] / "quantizer"))
    z = np.load(str(c["data"] / "train_dstore" / "faiss_store.cosine.gnnlm.npz"))
    prob, T, n_test = c["prob"], c["T"], c["n_test"]
    model = {"sd": prob["sd"], "n_layers": c["L"], "n_heads": c["H"], "centroids": q["centroids"], "A": q["A"], "b": q["b"],
             "codes": np.load(str(c["data"] / "train_dstore" / "quantized-keys.npy")), "vals": prob["vals"], "n_store": c["n_train"],
             "left": 2, "right": 2, "asm": c["w"]}
    total = 0.0
    for s in range(0, n_test, T):
        e = min(n_test, s + T)
        one = {"neighbor_idxs": c["nbrs"][s:e], "tgt_feats": c["test_keys"][s:e], "targets": c["targets"][s:e], "knn_sims": None, "knn_ids": None}
        o = pipeline.eval_block(one, model, 0.0, 1.0)
        qn = oknn.normalize_queries(o["gcn_feat"].float(), True)
        dd, ii = oivf.search(qn.numpy(), z["R"], z["coarse"], z["pq"], z["list_off"], z["list_ids"], z["list_codes"], k=c["k"], nprobe=8)
        sims = oknn.sims_from_search(dd.astype(np.float32), ii, qn, sim_func, c["train_keys"], True)
        p, _ = oknn.knn_target_prob(sims, ii, prob["vals"], c["targets"][s:e], temp)
        total += oknn.combine_knn_and_vocab_probs(p, o["lm_logp"], lam).double().sum().item()
    ppl_ref = float(np.exp(-total / n_test))
    print(f"eval_lm --knn-sim-func {sim_func}: ppl {res['ppl']:.6f}, oracle {ppl_ref:.6f}")
    assert res["count"] == n_test and abs(res["ppl"] - ppl_ref) < 0.02
    # the default sim func gives another score: the recompute is in the run
    plain = eval_lm.cli_main(c["base"] + ["--lmbda", str(lam), "--temperature", str(temp)])
    assert plain["score_sum"] != res["score_sum"]
    capsys.readouterr()
    sw = eval_lm.cli_main(cmd + ["--sweep-lmbda", "0,0.1,0.25", "--sweep-temperature", "1.0,0.1", "--sweep-k", "4,32"])
    out = capsys.readouterr().out.strip().split("\n")
    assert sw["score_sum"] == res["score_sum"] and out[1] == lines[1]
    assert len(out) == 14 and all(l_.startswith("sweep k=") for l_ in out[2:])
    own = [r for r in sw["sweep"] if (r["k"], r["temperature"], r["lmbda"]) == (c["k"], temp, lam)]
    assert len(own) == 1 and own[0]["score_sum"] == sw["score_sum"]


class _Found:
    def __init__(self, r):
        self.r = r

    def result(self):
        return self.r


class _TorchIndex:
    """Device-search contract (search_begin -> handle.result() -> sims, ids, labels) over an exact torch search: test plumbing."""

    def __init__(self, keys, vals):
        self.kn = keys.float() / (keys.float() ** 2).sum(-1, keepdim=True).sqrt()
        self.vals = vals

    def search_begin(self, q, k, return_vals=True):
        s, i = torch.topk(q @ self.kn.T, k, dim=1)
        return _Found((s.contiguous(), i.contiguous(), self.vals[i].int().contiguous()))


@pytest.mark.parametrize("sim_func", ["ip", "l2"])
def test_engine(ops, dev, sim_func):
    """GnnLmEngine.score(..., knn_index=, knn_keys=, knn_sim_func=) == ops.knn_interp over ops.knn_recompute_sims of the returned ids,
    bit for bit; two batches begun on two streams get the results they have alone; the defaults are what they were."""
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=1, k=32, seed=1)
    eng, b1 = build_engine(prob, dev), to_batch(prob["block"], dev)
    keys = torch.randn(3000, 64, generator=torch.Generator().manual_seed(2)).half().to(dev)
    index = _TorchIndex(keys, eng.store.vals)
    gen = torch.Generator().manual_seed(3)
    b2 = dataclasses.replace(b1, tgt_feats=(b1.tgt_feats.float().cpu() * 0.5 + 0.3 * torch.randn(b1.tgt_feats.shape, generator=gen)).to(b1.tgt_feats.dtype).to(dev),
                             targets=torch.roll(b1.targets, 3))
    sweep = ([5, 32], [1.0, 0.1], [0.0, 0.25])
    alone = []
    for b in (b1, b2):
        out = eng.score(b, 0.25, 1.0, knn_index=index, k=32, knn_keys=keys, knn_sim_func=sim_func, sweep=sweep)
        x = out["gcn_feat"]
        qn = x / (x ** 2).sum(-1, keepdim=True).sqrt()
        sims = ops.knn_recompute_sims(qn.contiguous(), out["knn_ids"], keys, sim_func, normalize_keys=(sim_func == "ip"))
        assert torch.equal(out["knn_sims"], sims)
        want = ops.knn_interp(out["lm_logp"], sims, out["knn_ids"], b.targets, 1.0, 0.25, n_store=eng.store.n_store, knn_vals=out["knn_vals"])
        assert all(torch.equal(out[n_], w_) for n_, w_ in zip(("logp", "p_knn", "recall"), want))
        grid = ops.knn_interp_grid(out["lm_logp"], sims, out["knn_ids"], b.targets, *sweep, n_store=eng.store.n_store, knn_vals=out["knn_vals"])[0]
        assert torch.equal(out["sweep_logp"], grid)
        plain = eng.score(b, 0.25, 1.0, knn_index=index, k=32)
        assert torch.equal(plain["knn_ids"], out["knn_ids"]) and not torch.equal(plain["knn_sims"], out["knn_sims"])
        assert torch.equal(plain["logp"], eng.score(b, 0.25, 1.0, knn_index=index, k=32, knn_keys=keys)["logp"])     # keys alone change nothing
        alone.append(out)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    hs = []
    for s, b in ((s1, b1), (s2, b2)):
        with torch.cuda.stream(s):
            hs.append(eng.score_begin(b, 0.25, 1.0, knn_index=index, k=32, knn_keys=keys, knn_sim_func=sim_func))
    for s, h, want in zip((s1, s2), hs, alone):
        with torch.cuda.stream(s):
            out = eng.score_finish(h)
        s.synchronize()
        for name in ("logp", "p_knn", "recall", "knn_sims", "knn_ids"):
            assert torch.equal(out[name], want[name]), name
    with pytest.raises(ValueError):
        eng.score(b1, 0.25, 1.0, knn_index=index, k=32, knn_sim_func="ip")   # no key table
