"""The dense outputs through the Python layers: ``GnnLmModel.get_normalized_probs``, ``GnnLmEngine.predict`` and
``eval_lm --output-topk``, against the reference's fixtures and the float64 restatement of tests/dense_dist_ref.py.  GPU only."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import dense_dist_ref as R

pytestmark = pytest.mark.gpu
BAR = 2e-5
SMALLEST = dict(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8, left=2, right=2, n_layers=2, k=32,
                seed=0)       # the shape of smoke()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def scripted_model(asm, ratio):
    from gnnlm_amd.model import GnnLmModel

    class Scripted(GnnLmModel):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.adaptive_softmax, self.orig_prob_ratio, self.short_cut = asm, ratio, False

    return Scripted()


def golden_asm(g, dev):
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    emb = [torch.from_numpy(g[f"emb{i}"]) for i in range(3)]
    proj = [None] + [torch.from_numpy(g[f"proj{i}"]) for i in (1, 2)]
    return AdaptiveSoftmax([int(c) for c in g["cutoff"]], emb, proj, torch.from_numpy(g["class_proj"]), dev)


# ---------------------------------------------------------------------------------------------------- get_normalized_probs
def test_get_normalized_probs_golden(dev, golden):
    """[B, T, V] against the reference's own dense tensor (ratio 0), and the mixture of two of its row sets at ratio 0.3."""
    g = golden("adaptive_softmax")
    asm = golden_asm(g, dev)
    x = torch.from_numpy(g["x"]).to(dev)
    h = x.flip(1).contiguous()                                           # a second set of rows whose dense rows the fixture holds too
    dense = g["dense"].astype(np.float64)
    lp = scripted_model(asm, 0.0).get_normalized_probs((x, {"orig_x": h}), True, None)
    assert lp.shape == (2, 9, 24) and lp.dtype == torch.float32
    assert float(np.abs(lp.cpu().numpy() - dense).max()) < BAR
    p = scripted_model(asm, 0.0).get_normalized_probs((x, {}), False, {"target": None})
    np.testing.assert_allclose(p.cpu().numpy(), np.exp(dense), atol=BAR)
    np.testing.assert_allclose(p.sum(-1).cpu().numpy(), 1.0, atol=1e-5)
    mixed = scripted_model(asm, 0.3).get_normalized_probs((x, {"orig_x": h}), True, None).cpu().numpy()
    want = np.logaddexp(np.log(0.3) + dense[:, ::-1], np.log(0.7) + dense)                  # transformer.py:1056-1062,1075-1077
    assert float(np.abs(mixed - want).max()) < BAR
    assert float(np.abs(mixed - dense).max()) > 1e-3
    # without orig_x the ratio has nothing to mix with
    assert torch.equal(scripted_model(asm, 0.3).get_normalized_probs((x, {}), True, None), lp)


def test_get_normalized_probs_mixture_matches_the_reference_targets(dev, golden):
    """orig_ratio.npz: the reference's get_normalized_probs + gather at ratio 0.3 is the target column of ours."""
    g = golden("orig_ratio")
    asm = golden_asm(g, dev)
    x, h, t = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["h"]).to(dev), torch.from_numpy(g["target"]).to(dev)
    m = scripted_model(asm, 0.3)
    lp = m.get_normalized_probs((x, {"orig_x": h}), True, {"target": t})
    got = lp.gather(2, t.unsqueeze(-1)).squeeze(-1)
    assert float((got.cpu() - torch.from_numpy(g["mixed.0.3"])).abs().max()) < BAR
    # ... and of the target-only path this build scores with
    extra = {"orig_x": h}
    assert float((got - m.target_log_probs((x, extra), t)).abs().max()) < BAR


# ---------------------------------------------------------------------------------------------------- GnnLmEngine.predict
@pytest.fixture(scope="module")
def problem():
    from gnnlm_amd.synthetic import make_problem
    from oracle import pipeline
    prob = make_problem(**SMALLEST)
    ref = pipeline.run_problem(prob, 0.0, 1.0, dtype=torch.float64)       # the features of the float64 oracle
    w = {"cutoff": prob["asm"]["cutoff"], "emb": [e.numpy() for e in prob["asm"]["emb"]],
         "proj": [None if p is None else p.numpy() for p in prob["asm"]["proj"]], "class_proj": prob["asm"]["class_proj"].numpy()}
    blk = prob["block"]
    lm_gnn = R.adaptive_log_probs(ref["gcn_feat"], w)
    lm_base = R.adaptive_log_probs(blk["tgt_feats"].astype(np.float32), w)
    labels = R.neighbour_labels(blk["knn_ids"], prob["vals"])
    return dict(prob=prob, lm_gnn=lm_gnn, lm_base=lm_base, labels=labels)


def expected(problem, lmbda, temperature, ratio):
    blk, V = problem["prob"]["block"], problem["prob"]["vocab"]
    lm = problem["lm_gnn"] if ratio <= 0 else np.logaddexp(np.log(ratio) + problem["lm_base"], np.log(1 - ratio) + problem["lm_gnn"])
    if lmbda > 0:
        lm = R.mix(lm, R.knn_probs(blk["knn_sims"], blk["knn_ids"], problem["labels"], temperature, V), lmbda)
    return lm


def check_prediction(got, dense, targets, N, tol, label):
    """ids / logp / rank / target_logp against the float64 rows: equal where the rows' gaps exceed ``tol``, else within it"""
    ids, logp, rank, tlogp = (t.cpu().numpy() for t in got)
    n, V = dense.shape
    rid, rval = R.topn(dense, N)
    rrank = R.rank(dense, targets)
    assert ids.shape == (n, N) and ids.dtype == np.int64 and logp.dtype == np.float32 and rank.dtype == np.int32
    e = float(np.abs(logp - rval).max())
    et = float(np.abs(tlogp - dense[np.arange(n), targets]).max())
    print(f"{label}: |logp - f64| {e:.2e}, |target_logp - f64| {et:.2e}, ids equal {np.array_equal(ids, rid)}, rank equal {np.array_equal(rank, rrank)}")
    assert e < tol and et < tol
    assert float(np.abs(np.take_along_axis(dense, ids, 1) - rval).max()) < tol, "an id of the top-N is not among the N best"
    srt = -np.sort(-dense, axis=1)
    clear = (srt[:, :N] - srt[:, 1:N + 1]).min(1) > 2 * tol              # rows whose first N + 1 values are further apart than the bar
    assert clear.mean() > 0.8 and np.array_equal(ids[clear], rid[clear])
    tv = dense[np.arange(n), targets][:, None]
    near = (np.abs(dense - tv) <= 2 * tol).sum(1) - 1                    # other columns the bar cannot tell from the target
    assert (np.abs(rank - rrank) <= near).all() and np.array_equal(rank[near == 0], rrank[near == 0])
    for r in range(n):                                                   # the target's rank is its place in the list
        if rank[r] < N and near[r] == 0:
            assert ids[r, rank[r]] == targets[r]


@pytest.mark.parametrize("lmbda,temperature,ratio", [(0.0, 1.0, 0.0), (0.25, 1.0, 0.0), (0.1, 0.01, 0.0), (0.25, 1.0, 0.3), (0.0, 1.0, 0.3)])
def test_engine_predict(dev, problem, monkeypatch, lmbda, temperature, ratio):
    from gnnlm_amd import predict
    from gnnlm_amd.synthetic import build_engine, to_batch
    prob = problem["prob"]
    eng, batch = build_engine(prob, dev), to_batch(prob["block"], dev)
    N = 5
    got = eng.predict(batch, lmbda, temperature, orig_prob_ratio=ratio, topk=N)
    dense = expected(problem, lmbda, temperature, ratio)
    # the chain behind the rows is the 2-layer HGT in float32: smoke()'s bar for its log-probs
    check_prediction(got, dense, prob["block"]["targets"], N, 1e-4, f"lmbda={lmbda} t={temperature} ratio={ratio}")
    score = eng.score(batch, lmbda, temperature, orig_prob_ratio=ratio)
    assert float((got[3] - score["logp"]).abs().max()) < 4e-5            # target_logp is score()'s logp
    # row chunks (3 rows of 600 columns per chunk instead of one chunk): the same bits
    monkeypatch.setattr(predict, "DENSE_CHUNK_BYTES", 3 * 600 * 4)
    assert predict.chunk_rows(600) == 3
    again = eng.predict(batch, lmbda, temperature, orig_prob_ratio=ratio, topk=N)
    for a, b in zip(got, again):
        assert torch.equal(a, b)


def test_engine_predict_refusals(dev, problem):
    from gnnlm_amd.synthetic import build_engine, to_batch
    prob = problem["prob"]
    eng, batch = build_engine(prob, dev), to_batch(prob["block"], dev)
    for bad in (0, 2049, 601):
        with pytest.raises(ValueError):
            eng.predict(batch, topk=bad)
    with pytest.raises(ValueError):
        eng.predict(batch, 0.25, 1.0, sweep=([8], [1.0], [0.1]), topk=3)
    ids, logp, rank, tlogp = eng.predict(batch, topk=600)               # N = V: every column, in order
    assert bool((ids.sort(1).values == torch.arange(600, device=dev)).all())
    assert bool((logp[:, :-1] >= logp[:, 1:]).all())
    assert bool((ids.gather(1, rank.long().unsqueeze(1)).squeeze(1) == batch.targets).all())


# ---------------------------------------------------------------------------------------------------- eval_lm --output-topk
def write_dstore(path, keys, vals, vocab, fp16=True):
    os.makedirs(path, exist_ok=True)
    keys.tofile(os.path.join(path, "keys.npy"))
    vals.tofile(os.path.join(path, "vals.npy"))
    json.dump({"dstore_size": len(vals), "hidden_size": keys.shape[1], "vocab_size": vocab, "dstore_fp16": fp16,
               "val_size": 1}, open(os.path.join(path, "info.json"), "w"))


def make_data_dir(tmp_path, n_test=41, L=2):
    """A synthetic data directory in the reference's on-disk formats + a reference-style checkpoint (as tests/test_mirrors_gpu.py
    builds one)."""
    from gnnlm_amd.synthetic import make_problem
    d, H, M, dsub, V, kg, T = 64, 4, 16, 4, 600, 6, 16
    n_train = 2000                                  # n_test = 41: 2 full blocks + a 9-token block
    prob = make_problem(n_store=n_train, d=d, n_heads=H, M=M, dsub=dsub, vocab=V, cutoff=[100, 300], T=n_test, kg=kg,
                        left=2, right=2, n_layers=L, k=8, seed=3)
    data = tmp_path / "data-bin"
    rs = np.random.RandomState(0)
    train_keys = rs.randn(n_train, d).astype(np.float16)
    write_dstore(str(data / "train_dstore"), train_keys, prob["vals"].astype(np.int16), V)   # fp16 store, V < 2**15 -> int16
    np.save(str(data / "train_dstore" / "quantized-keys.npy"), prob["codes"])
    blk = prob["block"]
    blk["targets"] = np.maximum(blk["targets"], 4)        # ids 0-3 are fairseq's specials; pad (1) is stripped by the scorer
    write_dstore(str(data / "test_dstore"), blk["tgt_feats"], blk["targets"].astype(np.int16), V)
    blk["ids"].tofile(str(data / "test_dstore" / f"neighbors.mmap.{kg}"))
    sd = {"decoder.hgt_decoder." + k: v for k, v in prob["sd"].items()}
    w = prob["asm"]
    for i, e in enumerate(w["emb"]):
        sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = e
        if i:
            sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = w["proj"][i]
    sd["decoder.adaptive_softmax.head.class_proj.weight"] = w["class_proj"]
    sd["decoder.tgt_quantizer.centroids_torch"] = torch.from_numpy(prob["cen"])
    sd["decoder.tgt_quantizer.A"] = torch.from_numpy(prob["A"])
    sd["decoder.tgt_quantizer.b"] = torch.from_numpy(prob["b"])
    margs = Namespace(decoder_embed_dim=d, decoder_attention_heads=H, graph_layer=L, decoder_gcn_dim=d,
                      adaptive_softmax_cutoff="100,300", orig_prob_ratio=0.0, short_cut=False, quantizer_path="")
    torch.save({"args": margs, "model": sd}, str(tmp_path / "ckpt.pt"))
    base = [str(data), "--path", str(tmp_path / "ckpt.pt"), "--gen-subset", "test", "--graph", "--neighbor-context", "2",
            "--gcn-k", str(kg), "--use-precompute-feat", "--sample-break-mode", "none", "--max-tokens", str(2 * T),
            "--tokens-per-sample", str(T), "--gcn-context-window", "0", "--knn-keytype", "gcn_feat",
            "--model-overrides", "{'orig_prob_ratio': 0.0}"]
    model = {"sd": prob["sd"], "n_layers": L, "n_heads": H, "centroids": prob["cen"], "A": prob["A"], "b": prob["b"],
             "codes": prob["codes"], "vals": prob["vals"], "n_store": n_train, "left": 2, "right": 2, "asm": w}
    return dict(prob=prob, blk=blk, data=data, base=base, model=model, train_keys=train_keys, T=T, n_test=n_test,
                n_train=n_train, w=w, L=L, H=H)


def restated_rows(c, lam, temp, k):
    """The float64 rows eval_lm's distribution has, block by block: oracle features -> dense head -> exact search -> kNN mix"""
    from oracle import knn as oknn, pipeline
    prob, blk, model, T, n_test = c["prob"], c["blk"], c["model"], c["T"], c["n_test"]
    w = {"cutoff": c["w"]["cutoff"], "emb": [e.numpy() for e in c["w"]["emb"]], "proj": [None if p is None else p.numpy() for p in c["w"]["proj"]],
         "class_proj": c["w"]["class_proj"].numpy()}
    lm_rows, mix_rows = [], []
    for s in range(0, n_test, T):
        e = min(n_test, s + T)
        one = {"neighbor_idxs": blk["ids"][s:e], "tgt_feats": blk["tgt_feats"][s:e], "targets": blk["targets"][s:e], "knn_sims": None, "knn_ids": None}
        o = pipeline.eval_block(one, model, 0.0, 1.0, dtype=torch.float64)
        lm = R.adaptive_log_probs(o["gcn_feat"].numpy(), w)
        q = oknn.normalize_queries(o["gcn_feat"].float(), True).numpy()
        dd, ii = oknn.brute_force_search(q, c["train_keys"], k, "ip", cosine=True)
        p = R.knn_probs(dd, ii, R.neighbour_labels(ii, prob["vals"]), temp, prob["vocab"])
        lm_rows.append(lm)
        mix_rows.append(R.mix(lm, p, lam))
    return np.concatenate(lm_rows), np.concatenate(mix_rows)


def gaps(dense, targets, N):
    srt = -np.sort(-dense, axis=1)
    tv = dense[np.arange(len(targets)), targets][:, None]
    others = np.abs(dense - tv)
    others[np.arange(len(targets)), targets] = np.inf
    return float((srt[:, :N] - srt[:, 1:N + 1]).min()), float(others.min())


@pytest.mark.parametrize("knn", [True, False])
def test_eval_lm_output_topk(dev, tmp_path, capsys, caplog, knn):
    """--output-topk 5 [--knnlm]: the saved ids / target_rank are the restatement's, the perplexity line and the result JSON
    are those of the run without the flag."""
    import logging
    from gnnlm_amd import eval_lm
    c = make_data_dir(tmp_path)
    lam, temp, k, N, T = 0.25, 1.0, 8, 5, c["T"]
    base = list(c["base"])
    base[base.index("--max-tokens") + 1] = str(T)          # one block per batch as in the recipe
    if knn:
        base += ["--knnlm", "--k", str(k), "--lmbda", str(lam), "--dstore-dir", str(c["data"] / "train_dstore"),
                 "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", str(temp), "--knn-sim-func", "ip"]
    capsys.readouterr()
    plain = eval_lm.cli_main(base + ["--result-json", str(tmp_path / "plain.json")])
    plain_out = capsys.readouterr().out
    out_path = str(tmp_path / "top.npz")
    with caplog.at_level(logging.INFO, logger="gnnlm_amd.eval_lm"):
        res = eval_lm.cli_main(base + ["--result-json", str(tmp_path / "top.json"), "--output-topk", str(N), "--topk-out", out_path])
    top_out = capsys.readouterr().out
    ppl = lambda text: [ln for ln in text.splitlines() if ln.startswith("Loss (base 2)")]
    assert len(ppl(plain_out)) == 1 and ppl(plain_out) == ppl(top_out)
    timed = ("seconds", "wall_seconds")
    ja, jb = json.load(open(tmp_path / "plain.json")), json.load(open(tmp_path / "top.json"))
    assert {k_: v for k_, v in ja.items() if k_ not in timed} == {k_: v for k_, v in jb.items() if k_ not in timed}
    assert res["score_sum"] == plain["score_sum"] and res["count"] == c["n_test"]
    z = np.load(out_path)
    assert sorted(z.files) == ["ids", "logp", "target_rank"]
    ids, logp, rank = z["ids"], z["logp"], z["target_rank"]
    assert ids.shape == (c["n_test"], N) and ids.dtype == np.int32 and logp.dtype == np.float32 and rank.shape == (c["n_test"],) \
        and rank.dtype == np.int32
    lm_rows, mix_rows = restated_rows(c, lam, temp, k)
    dense = mix_rows if knn else lm_rows
    targets = c["blk"]["targets"].astype(np.int64)
    rid, rval = R.topn(dense, N)
    g_top, g_tgt = gaps(dense, targets, N)
    print(f"knn={knn}: smallest gap among the first {N + 1} values {g_top:.2e}, between a target and another column {g_tgt:.2e}; "
          f"|logp - f64| {float(np.abs(logp - rval).max()):.2e}")
    assert g_top > 1e-4 and g_tgt > 1e-4, "the fixture has a near tie: its order is not the restatement's to decide"
    assert np.array_equal(ids, rid)
    assert np.array_equal(rank, R.rank(dense, targets))
    assert float(np.abs(logp - rval).max()) < 1e-4                        # (the 2-layer HGT in float32 in front: smoke()'s bar)
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith("top-1 acc")]
    assert len(lines) == 1
    acc1, accn, mrr = float((rank == 0).mean()), float((rank < N).mean()), float((1.0 / (rank + 1.0)).mean())
    assert lines[0] == "top-1 acc {:.4f} | top-{} acc {:.4f} | MRR {:.4f}".format(acc1, N, accn, mrr)


def test_eval_lm_output_topk_refusals(dev, tmp_path):
    from gnnlm_amd import eval_lm
    c = make_data_dir(tmp_path)
    for extra, word in ((["--sweep-orig-prob-ratio", "0,0.3"], "--sweep"), (["--graph-capture"], "--graph-capture"), (["--output-topk", "4000"], "2048")):
        with pytest.raises(ValueError, match=word):
            eval_lm.cli_main(c["base"] + ["--output-topk", "5"] + extra)


COMBOS = {
    "fp16+knn": (["--fp16"], True),
    "eos": (["--sample-break-mode", "eos"], False),
    "complete+ctx+knn": (["--sample-break-mode", "complete", "--gcn-context-window", "8"], True),
    "ratio+knn": (["--model-overrides", "{'orig_prob_ratio': 0.3}"], True),
    "ratio+eos+fp16": (["--model-overrides", "{'orig_prob_ratio': 0.3}", "--sample-break-mode", "eos", "--fp16"], False),
    "reinit-nfeat+knn": (["--reinit-nfeat"], True),              # the directory of tests/test_reinit_nfeat_gpu.py (no PQ codes, no quantizer)
    "dense-head+knn": ([], True),                                # the directory of tests/test_dense_head_gpu.py (plain softmax with xl_bias, V = 205)
    "dense-head+ratio+eos": (["--model-overrides", "{'orig_prob_ratio': 0.3}", "--sample-break-mode", "eos"], False),
}


@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_eval_lm_output_topk_with_other_flags(dev, tmp_path, monkeypatch, combo):
    """--output-topk beside --fp16, the break modes, a context window, orig_prob_ratio, --reinit-nfeat, the plain head and --knnlm: the score sum is the run's
    without the flag, and every hypothesis ties its dense rows to its own scores -- a target of rank r < N is entry r of the list
    with the log-probability the hypothesis scores it with, a target of rank >= N scores no
    higher than the list's last entry; the saved table is the hypotheses' rows in corpus order."""
    from test_ragged_gpu import SENT_SIZES, make_ragged_dir
    from gnnlm_amd import eval_lm
    from gnnlm_amd.sequence_scorer import SequenceScorer
    flags, knn = COMBOS[combo]
    N = 5
    # f32: two kernels, the log-prob bar once each.  --fp16: the target-column path and the dense path each round the float32 tail
    # projection to float16 on their own GEMM route; where the two float32 values straddle a float16 rounding boundary one operand
    # element moves by 2^-11 of itself and a band logit by up to 2^-11 |xi_e| |emb_e| (a few 1e-4 at these weights): 5e-4
    tol = 5e-4 if "--fp16" in flags else 4e-5
    if combo.startswith("reinit"):
        from test_reinit_nfeat_gpu import make_dir
        c = make_dir(tmp_path, 2)
    elif combo.startswith("dense-head"):
        from test_dense_head_gpu import make_dense_dir
        c = make_dense_dir(tmp_path, SENT_SIZES)
    else:
        c = make_ragged_dir(tmp_path, SENT_SIZES, L=2)
    # one block per batch as in the recipe (several per launch): with B > 1 per batch the scorer keeps the reference's [T, B]-against-
    # [B, T] target pairing under --knnlm, and a hypothesis' tokens are then not the targets it scores
    args = c["base"] + ["--tokens-per-sample", "64", "--max-tokens", "64"] + flags
    if knn:
        args += ["--knnlm", "--k", "8", "--lmbda", "0.25", "--dstore-dir", str(c["data"] / "train_dstore"),
                 "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]
    seen = []
    inner = SequenceScorer.generate_finish

    def finish(scorer, h):
        hypos = inner(scorer, h)
        seen.append((int(h["sample"]["id"][0]), [{k_: (v.clone() if torch.is_tensor(v) else v) for k_, v in hy[0].items()} for hy in hypos]))
        return hypos
    monkeypatch.setattr(SequenceScorer, "generate_finish", finish)
    plain = eval_lm.cli_main(args)
    assert all("topk_ids" not in hy for _, hs in seen for hy in hs)
    seen.clear()
    out_path = str(tmp_path / "top.npz")
    top = eval_lm.cli_main(args + ["--output-topk", str(N), "--topk-out", out_path])
    assert top["score_sum"] == plain["score_sum"] and top["count"] == plain["count"] == c["n_test"]
    rows_ids, rows_rank, inside = [], [], 0
    for _, hs in sorted(seen, key=lambda e: e[0]):
        for hy in hs:
            ids, sc, rk, tok, pos = hy["topk_ids"], hy["topk_scores"], hy["target_rank"].long(), hy["tokens"], hy["positional_scores"]
            assert ids.shape == (tok.numel(), N) and sc.shape == ids.shape and rk.shape == tok.shape and bool((rk >= 0).all())
            assert bool((sc[:, :-1] >= sc[:, 1:]).all())
            m = rk < N
            inside += int(m.sum())
            if m.any():
                at = rk[m].unsqueeze(1)
                assert bool((ids[m].gather(1, at).squeeze(1) == tok[m]).all())
                assert float((sc[m].gather(1, at).squeeze(1) - pos[m]).abs().max()) < tol
            if (~m).any():
                assert bool((pos[~m] <= sc[~m][:, -1] + tol).all())
            rows_ids.append(ids.cpu().numpy())
            rows_rank.append(rk.cpu().numpy())
    assert inside > 0
    z = np.load(out_path)
    assert np.array_equal(z["ids"], np.concatenate(rows_ids).astype(np.int32))
    assert np.array_equal(z["target_rank"], np.concatenate(rows_rank).astype(np.int32))
    assert z["ids"].shape == (c["n_test"], N)
