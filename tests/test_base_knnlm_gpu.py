"""kNN-LM on the base transformer LM (``eval_lm --knnlm`` without ``--graph``): the driver against the float64 restatement
(tests/base_knnlm_ref.py, pinned to the reference by tests/test_base_knnlm_ref_cpu.py) on the fixture tests/golden/base_knnlm.npz --
three configurations, cosine and inner product, both key types, k = 40 and 8, two temperatures -- and the flags around it: --lmbda 0,
--sweep-*, --output-topk, --save-knnlm-dstore, the recipe end to end at toy size, the refusals.  GPU only.

Bar on the mixed log-prob: 2e-5 + 2 * 2e-5 / t.  2e-5 is the project's bar on LM log-probs and on search scores; a log-softmax moves
by at most twice the sup-norm change of its logits (sims / t), and logaddexp is 1-Lipschitz in each argument.  Perplexity within 0.02,
knn_recall equal, the neighbours' similarities within 2e-5 of float64.

Measured on an MI355X: mixed log-probs at most 6.8e-6 from float64 (t = 0.1; 1.4e-6 at t = 1), similarities 2.4e-6
(inner product) and 1.7e-7 (cosine), perplexity equal to four decimals in every case, the toy recipe equal to the hand-made
``KNNModel.interpolate`` bit for bit.
"""
import json
import os

import numpy as np
import pytest
import torch

import base_knnlm_ref as kr
import test_transformer_lm_gpu as base
import transformer_lm_ref as tr

pytestmark = pytest.mark.gpu

LMBDA = 0.25


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def write_store(path, keys, vals, V):
    os.makedirs(path, exist_ok=True)
    np.asarray(keys, np.float32).tofile(os.path.join(path, "keys.npy"))
    np.asarray(vals, np.int32).reshape(-1, 1).tofile(os.path.join(path, "vals.npy"))
    json.dump({"dstore_size": int(len(vals)), "hidden_size": int(keys.shape[1]), "vocab_size": int(V), "dstore_fp16": False, "val_size": 1},
              open(os.path.join(path, "info.json"), "w"))


@pytest.fixture(scope="module")
def fx(golden, tmp_path_factory):
    """DATA/test.bin/.idx, a checkpoint with the fixture's weights (plain output layer tied to the embedding) and its datastore."""
    g = golden("base_knnlm")
    root = tmp_path_factory.mktemp("base_knnlm")
    m = tr.make_model(pos_rows=128, **kr.MODEL)
    assert np.array_equal(m["E"], g["E"])
    base.write_split(root, "test", g["tokens"], kr.SIZES)
    args = base.args_of(m, kr.MODEL)
    torch.save({"args": args, "model": base.state_dict_of(m, "qkv")}, root / "base.pt")
    write_store(str(root / "store"), g["keys"], g["vals"], kr.MODEL["V"])
    return {"g": g, "root": root, "ckpt": root / "base.pt", "store": str(root / "store"), "m": m, "ref": {}, "plain": {}}


def flags(cfg):
    mode, tps, w, max_tokens = kr.CONFIGS[cfg]
    return ["--sample-break-mode", mode, "--tokens-per-sample", str(tps), "--max-tokens", str(max_tokens)] + (["--context-window", str(w)] if w else [])


def reference(fx, cfg, keytype, cosine, k, t, lmbda=LMBDA):
    key = (cfg, keytype, cosine, k, t, lmbda)
    if key not in fx["ref"]:
        g = fx["g"]
        samples = [(int(s), int(e)) for s, e in g[f"{cfg}.samples"]]
        fx["ref"][key] = kr.score(fx["m"], g["tokens"], samples, g[f"{cfg}.ctx"].tolist(), g["keys"], g["vals"], keytype, cosine, k, t, lmbda)
    return fx["ref"][key]


class CountingIndex:
    """An ExactIndex that records its searches (one entry per call: queries, similarities, ids)."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def search_device(self, q, k):
        val, idx = self.inner.search_device(q, k)
        self.calls.append((q.detach().cpu().numpy(), val.cpu().numpy(), idx.cpu().numpy()))
        return val, idx


class ForbiddenIndex:
    def search_device(self, q, k):
        raise AssertionError("the index was searched")

    search = search_device


def knn_model(fx, dev, cosine, k, index=None, sim_func="do_not_recomp_ip"):
    from gnnlm_amd.knn_model import ExactIndex, KNNModel
    if index is None:
        index = CountingIndex(ExactIndex(torch.from_numpy(fx["g"]["keys"]), "ip", cosine, dev))
    return KNNModel(os.path.join(fx["store"], "faiss_store.cosine" if cosine else "faiss_store.ip"), fx["store"], k=k, no_load_keys=True,
                    metric_type=sim_func, index=index, device=dev)


def drive(fx, extra, knn=None):
    from gnnlm_amd.eval_lm import get_parser, main
    args = get_parser().parse_args([str(fx["root"]), "--path", str(fx["ckpt"]), "--gen-subset", "test"] + extra)
    args.keep_pos_scores = True
    if knn is not None:
        args.knn_model = knn
    return main(args)


def plain(fx, cfg):
    if cfg not in fx["plain"]:
        fx["plain"][cfg] = drive(fx, flags(cfg))
    return fx["plain"][cfg]


def knn_flags(k, t, lmbda=LMBDA, keytype=None):
    return ["--knnlm", "--k", str(k), "--lmbda", str(lmbda), "--temperature", str(t)] + (["--knn-keytype", keytype] if keytype else [])


# ---------------------------------------------------------------------------------------------------- the driver against float64
@pytest.mark.parametrize("cosine", [False, True], ids=["ip", "cosine"])
@pytest.mark.parametrize("cfg", sorted(kr.CONFIGS))
def test_driver_against_restatement(dev, fx, cfg, cosine):
    n = len(fx["g"]["tokens"])
    for keytype in (None, "last_ffn_input"):
        for k in (40, 8):
            for t in (1.0, 0.1):
                ref = reference(fx, cfg, keytype, cosine, k, t)
                knn = knn_model(fx, dev, cosine, k)
                res = drive(fx, flags(cfg) + knn_flags(k, t, keytype=keytype), knn)
                assert res["count"] == n == len(ref["mixed"])
                # the index saw the scored rows, each once, never a context row
                calls = knn.index.calls
                assert sum(c[0].shape[0] for c in calls) == n
                assert res["tokens"] == n + int(sum(fx["g"][f"{cfg}.ctx"]))
                got_sims, got_ids = np.concatenate([c[1] for c in calls]), np.concatenate([c[2] for c in calls])
                assert np.array_equal(np.sort(got_ids, 1), np.sort(ref["ids"], 1))                     # the float64 neighbour set (margin 1e-3)
                d_sims = np.abs(got_sims - np.take_along_axis(ref["sims"], got_ids, 1)).max()
                d = np.abs(res["pos_scores"] - ref["mixed"]).max()
                ppl = float(2 ** (-ref["mixed"].sum() / n / np.log(2)))
                print(f"{cfg} {'cosine' if cosine else 'ip'} {keytype or 'inner'} k={k} t={t}: max |d sims| = {d_sims:.3e}, max |d logp| = {d:.3e} "
                      f"(bar {2e-5 + 4e-5 / t:.1e}), ppl {res['ppl']:.4f} vs {ppl:.4f}")
                assert d_sims <= 2e-5
                assert d <= 2e-5 + 2 * 2e-5 / t
                assert abs(res["ppl"] - ppl) <= 0.02
                # the fixture itself: what the reference's scorer returned
                tag = f"{cfg}.{'cosine' if cosine else 'ip'}.{keytype or 'inner'}.k{k}.t{t}"
                assert np.abs(res["pos_scores"] - fx["g"][tag + ".pos"]).max() <= 2e-5 + 2 * 2e-5 / t + 1e-5


def test_knn_recall_reaches_the_word_outputs(dev, fx, monkeypatch):
    """--output-knn-recall: the hypotheses handed to the word outputs carry knn_recall per token, equal to the restatement's."""
    from gnnlm_amd import eval_lm
    seen = []
    real = eval_lm.word_outputs

    def spy(args, hypos, *rest):
        seen.extend(h[0]["knn_recall"].cpu().numpy() for h in hypos)
        return real(args, hypos, *rest)

    monkeypatch.setattr(eval_lm, "word_outputs", spy)
    for cfg in sorted(kr.CONFIGS):
        for cosine, keytype, k in ((True, None, 8), (False, "last_ffn_input", 40), (False, None, 8)):
            seen.clear()
            ref = reference(fx, cfg, keytype, cosine, k, 1.0)
            drive(fx, flags(cfg) + knn_flags(k, 1.0, keytype=keytype) + ["--output-knn-recall", "--output-word-probs"], knn_model(fx, dev, cosine, k))
            assert np.array_equal(np.concatenate(seen), ref["recall"]), (cfg, cosine, keytype, k)
            assert np.array_equal(ref["recall"], fx["g"][f"{cfg}.{'cosine' if cosine else 'ip'}.{keytype or 'inner'}.k{k}.t1.0.recall"])


@pytest.mark.parametrize("cosine", [False, True], ids=["ip", "cosine"])
def test_recomputed_similarities(dev, fx, cosine):
    """--knn-sim-func ip: the similarities are recomputed from the stored keys (normalised for a cosine index) against the packed
    queries -- the same numbers as the search's own, so the same restatement and the same bar."""
    cfg, k, t = "none+ctx", 8, 1.0
    ref = reference(fx, cfg, None, cosine, k, t)
    from gnnlm_amd.knn_model import ExactIndex, KNNModel
    index = CountingIndex(ExactIndex(torch.from_numpy(fx["g"]["keys"]), "ip", cosine, dev))
    knn = KNNModel(os.path.join(fx["store"], "faiss_store.cosine" if cosine else "faiss_store.ip"), fx["store"], k=k, metric_type="ip", index=index, device=dev)
    res = drive(fx, flags(cfg) + knn_flags(k, t) + ["--knn-sim-func", "ip"], knn)
    d = np.abs(res["pos_scores"] - ref["mixed"]).max()
    print(f"--knn-sim-func ip, {'cosine' if cosine else 'ip'} index: max |d logp| = {d:.3e}")
    assert d <= 2e-5 + 2 * 2e-5 / t


# ---------------------------------------------------------------------------------------------------- --lmbda 0, the plain path
@pytest.mark.parametrize("cfg", sorted(kr.CONFIGS))
def test_lmbda_0_is_the_plain_run_without_a_search(dev, fx, cfg):
    want = plain(fx, cfg)
    got = drive(fx, flags(cfg) + knn_flags(8, 1.0, lmbda=0.0), knn_model(fx, dev, True, 8, index=ForbiddenIndex()))
    assert np.array_equal(got["pos_scores"].view(np.uint32), want["pos_scores"].view(np.uint32))
    assert got["score_sum"] == want["score_sum"] and got["count"] == want["count"]
    ref = reference(fx, cfg, None, False, 40, 1.0, 0.0)
    assert np.abs(want["pos_scores"] - ref["lm"]).max() <= 2e-5


# ---------------------------------------------------------------------------------------------------- sweeps
def test_sweep_points_equal_their_single_runs(dev, fx):
    cfg, ks, ts, ls = "none+ctx", [40, 8], [1.0, 0.1], [0.25, 0.6]
    knn = knn_model(fx, dev, True, 40)
    res = drive(fx, flags(cfg) + knn_flags(40, 1.0) + ["--sweep-k", "40,8", "--sweep-temperature", "1,0.1", "--sweep-lmbda", "0.25,0.6"], knn)
    n_batches = len(knn.index.calls)
    assert n_batches >= 2 and sum(c[0].shape[0] for c in knn.index.calls) == res["count"]              # one search per batch for the whole grid
    rows = res["sweep"]
    assert [(r["k"], r["temperature"], r["lmbda"]) for r in rows] == [(k, t, l) for k in ks for t in ts for l in ls]
    assert set(rows[0]) == {"k", "temperature", "lmbda", "score_sum", "loss", "ppl"}
    for r in rows:
        single = drive(fx, flags(cfg) + knn_flags(r["k"], r["temperature"], lmbda=r["lmbda"]), knn_model(fx, dev, True, r["k"]))
        assert abs(r["score_sum"] / res["count"] - single["score_sum"] / single["count"]) <= 1e-6, r
        ref = reference(fx, cfg, None, True, r["k"], r["temperature"], r["lmbda"])
        assert abs(r["score_sum"] - ref["mixed"].sum()) / res["count"] <= 2e-5 + 4e-5 / r["temperature"]
    # the run's own setting is scored as without the sweep
    own = drive(fx, flags(cfg) + knn_flags(40, 1.0), knn_model(fx, dev, True, 40))
    assert np.array_equal(res["pos_scores"], own["pos_scores"])


# ---------------------------------------------------------------------------------------------------- --output-topk
@pytest.mark.parametrize("with_knn", [True, False], ids=["knn", "lm"])
def test_output_topk(dev, fx, tmp_path, with_knn):
    cfg, k, t, N = "none+ctx", 8, 1.0, 5
    extra = flags(cfg) + (knn_flags(k, t) if with_knn else [])
    mk = lambda: knn_model(fx, dev, True, k) if with_knn else None
    without = drive(fx, extra, mk())
    out = tmp_path / "top.npz"
    res = drive(fx, extra + ["--output-topk", str(N), "--topk-out", str(out)], mk())
    assert np.array_equal(res["pos_scores"], without["pos_scores"])
    for key in ("score_sum", "count", "ppl", "tokens"):
        assert res[key] == without[key], key
    z = np.load(out)
    ref = reference(fx, cfg, None, True, k, t)
    dense = kr.dense_mix(ref["dense_lm"], ref["sims"], fx["g"]["vals"], k, t, LMBDA) if with_knn else ref["dense_lm"]
    n = len(ref["targets"])
    assert z["ids"].shape == (n, N) and z["logp"].shape == (n, N) and z["target_rank"].shape == (n,)
    top2 = -np.sort(-dense, axis=1)[:, :2]
    clear = (top2[:, 0] - top2[:, 1]) > 1e-4
    assert clear.sum() >= n // 2
    assert np.array_equal(z["ids"][clear, 0], dense.argmax(1)[clear])
    tl = dense[np.arange(n), ref["targets"]]
    rank = (dense > tl[:, None]).sum(1)
    near = (np.abs(dense - tl[:, None]) <= 1e-4).sum(1) > 1                                        # another entry within 1e-4 of the target's
    assert np.array_equal(z["target_rank"][~near], rank[~near])
    assert np.abs(z["logp"][:, 0] - dense.max(1)).max() <= 2e-5 + 4e-5 / t


# ---------------------------------------------------------------------------------------------------- --save-knnlm-dstore --knnlm
def test_saving_the_datastore_with_knnlm_writes_the_same_bytes(dev, fx, tmp_path):
    cfg = "none+ctx"
    a, b = tmp_path / "a", tmp_path / "b"
    save = lambda p: ["--save-knnlm-dstore", "--dstore-mmap", str(p), "--knn-keytype", "last_ffn_input"]
    drive(fx, flags(cfg) + save(a))
    res = drive(fx, flags(cfg) + save(b) + knn_flags(8, 1.0), knn_model(fx, dev, True, 8))
    for f in ("keys.npy", "vals.npy", "info.json"):
        sub = "test_dstore-last_ffn_input"
        assert open(a / sub / f, "rb").read() == open(b / sub / f, "rb").read(), f
    ref = reference(fx, cfg, "last_ffn_input", True, 8, 1.0)
    assert np.abs(res["pos_scores"] - ref["mixed"]).max() <= 2e-5 + 4e-5


# ---------------------------------------------------------------------------------------------------- the recipe, end to end
def test_recipe_end_to_end_at_toy_size(dev, tmp_path):
    """save the datastore with the driver -> run_index_build (IVF-PQ: one list, PQ16 -- the smallest the builder accepts, which needs
    d = 64 and a few hundred keys) -> --knnlm --knn-sim-func do_not_recomp_ip; the scores equal KNNModel.interpolate called directly
    on extract_features' scored rows with the same index.  (The search itself is pinned by tests/test_knn_search_gpu.py.)"""
    from gnnlm_amd import run_index_build
    from gnnlm_amd.eval_base_lm import context_lengths, shifted_source
    from gnnlm_amd.eval_lm import get_parser, main
    from gnnlm_amd.ivfpq import IVFPQIndex
    from gnnlm_amd.knn_model import KNNModel
    from gnnlm_amd.transformer_lm import TransformerLM
    c = dict(seed=91, V=48, d=64, H=2, L=1, ffn=64, act="relu", final_norm=True, emb_norm=False, positions="sinusoidal")
    m = tr.make_model(pos_rows=128, **c)
    rs = np.random.RandomState(17)
    n = 320
    tokens = rs.randint(4, c["V"], size=n).astype(np.int64)
    base.write_split(tmp_path, "train", tokens, [n])
    ckpt = tmp_path / "base.pt"
    torch.save({"args": base.args_of(m, c), "model": base.state_dict_of(m, "qkv")}, ckpt)
    common = [str(tmp_path), "--path", str(ckpt), "--gen-subset", "train", "--sample-break-mode", "none", "--tokens-per-sample", "16",
              "--context-window", "8", "--max-tokens", "40", "--max-sentences", "1"]

    def run(extra):
        args = get_parser().parse_args(common + extra)
        args.keep_pos_scores = True
        return main(args)

    run(["--save-knnlm-dstore", "--dstore-mmap", str(tmp_path)])
    dd = tmp_path / "train_dstore"
    run_index_build.main(run_index_build.get_parser().parse_args(["--dstore-dir", str(dd), "--index-type", "IVF1,PQ16", "--metric", "ip", "--nprobe", "1"]))
    k, t = 16, 1.0
    knn_args = ["--knnlm", "--dstore-dir", str(dd), "--index-file", str(dd / "faiss_store.ip"), "--knn-sim-func", "do_not_recomp_ip", "--k", str(k),
                "--lmbda", str(LMBDA), "--temperature", str(t), "--probe", "1"]
    res = run(knn_args)
    # the same, by hand: one sample per batch (--max-sentences 1), the scored rows of inner_states[-1], KNNModel.interpolate
    model, _ = TransformerLM.from_checkpoint(str(ckpt), dev)
    knn = KNNModel(str(dd / "faiss_store.ip"), str(dd), k=k, probe=1, no_load_keys=True, metric_type="do_not_recomp_ip", device=dev)
    assert isinstance(knn.index, IVFPQIndex)
    src = shifted_source(tokens)
    lengths = [8] * (n // 8)
    ctx = context_lengths(lengths, 8, 8)
    want, s = [], 0
    for ln, cx in zip(lengths, ctx.tolist()):
        x, extra = model.extract_features(torch.from_numpy(src[s - cx:s + ln]).to(dev), [0, cx + ln])
        target = torch.from_numpy(tokens[s:s + ln]).to(dev)
        lm = model.target_logp(x[cx:], target)
        want.append(knn.interpolate(extra["inner_states"][-1][cx:].contiguous(), target, lm, t, LMBDA)[0].cpu().numpy())
        s += ln
    want = np.concatenate(want)
    assert res["count"] == n
    d = np.abs(res["pos_scores"] - want).max()
    print(f"recipe at toy size: max |driver - KNNModel.interpolate by hand| = {d:.3e}")
    assert d <= 1e-6
    assert np.abs(res["pos_scores"] - run([])["pos_scores"]).max() > 1e-3                             # the kNN term is really there


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev, fx, tmp_path):
    f = flags("none")
    # the key width must be the store's
    wide = str(tmp_path / "wide")
    write_store(wide, np.zeros((8, 64), np.float32), np.arange(8), kr.MODEL["V"])
    with pytest.raises(ValueError, match=r"(?s)32.*64|64.*32"):
        drive(fx, f + ["--knnlm", "--lmbda", "0.25", "--dstore-dir", wide, "--index-file", os.path.join(wide, "faiss_store.ip"), "--knn-sim-func", "ip"])
    with pytest.raises(ValueError, match="sweep-orig-prob-ratio"):
        drive(fx, f + knn_flags(8, 1.0) + ["--sweep-orig-prob-ratio", "0,0.5"], knn_model(fx, dev, True, 8))
    with pytest.raises(ValueError, match="--knnlm"):
        drive(fx, f + ["--sweep-lmbda", "0.1,0.2"])                                                    # a sweep needs the kNN term
    with pytest.raises(ValueError, match="--knnlm"):
        drive(fx, f + ["--output-knn-recall"])
    # the three refusals tests/test_transformer_lm_gpu.py::test_driver_refusals pins, still raised as before
    with pytest.raises(ValueError, match="--knnlm needs --dstore-dir and --index-file"):
        drive(fx, f + ["--knnlm"])
    with pytest.raises(NotImplementedError, match="use-precompute-feat"):
        drive(fx, f + ["--graph"])
    with pytest.raises(ValueError, match="graph-capture"):
        drive(fx, f + ["--graph-capture"])
