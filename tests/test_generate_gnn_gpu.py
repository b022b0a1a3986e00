"""Generation from the GNN-LM end to end (generate_gnn.GnnGenerator: base-LM step -> exact kNN search -> incremental HGT step -> head)
against the float64 chain of tests/gnn_decode_ref.py, which recomputes the graph decoder over the whole prefix for every token.

Conditions on the seeded inputs, computed from the float64 chain alone and asserted here: at every step the best and the second-best
log-prob differ by >= 1e-3, and every fed token's kg-th and (kg + 1)-th neighbour scores differ by >= 1e-3.  Under them the demands
are: the same tokens, the same neighbour-id sets for every token, log-probs within 2e-5 (README "Parity").  GPU only."""
import io

import numpy as np
import pytest
import torch

import decode_ref as dr
import gnn_decode_ref as gr
import test_transformer_lm_gpu as base
import transformer_lm_ref as tr
from test_generate_gpu import gen_lm

pytestmark = pytest.mark.gpu

LOGP_BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def make_generator(head, dev, lm=None):
    from gnnlm_amd.generate_gnn import GnnGenerator, IndexSearch
    from gnnlm_amd.hgt import HGT, CodeStore
    from gnnlm_amd.knn_model import ExactIndex
    from gnnlm_amd.model import GnnLmModel
    st = gr.gnn_store(head)
    d = dr.GEN_MODEL["d"]
    lm = gen_lm(gr.GNN_SEED, head, dev) if lm is None else lm
    hgt = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=gr.GNN_LAYERS, n_heads=st["H"])
    hgt.load_state_dict({k: torch.as_tensor(v) for k, v in st["sd"].items()}, strict=True)
    gnn = GnnLmModel(hgt, lm.head)                                      # the tied head: the GNN-LM's output layer is the base LM's
    store = CodeStore(codes=t(st["codes"], dev), centroids=t(st["cen"], dev), n_store=gr.GNN_KEYS, A=t(st["A"], dev), b=t(st["b"], dev))
    knn = IndexSearch(ExactIndex(t(st["keys"], dev), "ip", False, dev))
    return GnnGenerator(lm, gnn, knn, gr.GNN_KG, gr.GNN_LEFT, gr.GNN_RIGHT, store=store)


@pytest.mark.parametrize("head", dr.GEN_HEADS)
def test_greedy_generation_equals_the_float64_chain(dev, head):
    g = make_generator(head, dev)
    prompts = gr.gnn_prompts()
    assert [len(p) for p in prompts] == [1, 5, 40]
    tokens, logp, lengths = g.generate(prompts, gr.GNN_NEW)
    tokens, logp, lengths = tokens.cpu().numpy(), logp.cpu().numpy(), lengths.cpu().numpy()
    p_ids = g.last_run["prompt_ids"].cpu().numpy()
    s_ids = [x.cpu().numpy() for x in g.last_run["step_ids"]]
    off = np.concatenate([[0], np.cumsum([len(p) for p in prompts])])
    for i, p in enumerate(prompts):
        c = gr.gnn_chain(i, head)
        print(f"{head} prompt {i}: reference minimum log-prob gap {c['gaps'].min():.3e}, minimum neighbour-score gap {c['nb_gaps'].min():.3e}")
        assert c["gaps"].min() >= gr.GAP and c["nb_gaps"].min() >= gr.GAP              # the conditions, on the reference alone
        n = int(lengths[i])
        assert n == len(c["tokens"]) and tokens[i, :n].tolist() == c["tokens"], (i, tokens[i].tolist(), c["tokens"])
        assert (tokens[i, n:] == dr.PAD).all() and (logp[i, n:] == 0).all()
        got_ids = [p_ids[off[i] + j] for j in range(len(p))] + [s_ids[s][i] for s in range(n - 1)]
        assert len(got_ids) == c["ids"].shape[0]
        for j, (a, b) in enumerate(zip(got_ids, c["ids"])):
            assert set(a.tolist()) == set(b.tolist()), (i, j)
        e = float(np.abs(logp[i, :n] - c["logp"]).max())
        print(f"{head} prompt {i}: {n} tokens, max |d logp| = {e:.3e}")
        assert e <= LOGP_BAR
    # the graph decoder's cache stands where the base LM's does
    assert g.gnn_cache.len.tolist() == [len(p) + int(lengths[i]) - 1 for i, p in enumerate(prompts)]
    assert int(g.gnn_cache.n_bad.item()) == 0


def test_graph_decoder_changes_the_text_and_short_cut_removes_it(dev):
    """The GNN rows are what is scored: the picks' log-probs are not the base LM's own (the tiny models repeat one token either way,
    so the text says little), and with short_cut (rows pass through) tokens and log-probs are the base LM's again, bit for bit."""
    from gnnlm_amd.generate import Generator
    g = make_generator("dense", dev)
    prompts = gr.gnn_prompts()
    with_gnn = [x.cpu().numpy() for x in g.generate(prompts, 12)]
    plain = [x.cpu().numpy() for x in Generator(g.lm).generate(prompts, 12)]
    assert np.abs(with_gnn[1] - plain[1]).max() > 1e-2
    g.gnn.short_cut = True
    cut = [x.cpu().numpy() for x in g.generate(prompts, 12)]
    g.gnn.short_cut = False
    for x, y in zip(cut, plain):
        assert np.array_equal(x, y)
    g.gnn.orig_prob_ratio = 0.25
    with pytest.raises(NotImplementedError, match="orig_prob_ratio"):
        g.generate(prompts, 4)
    g.gnn.orig_prob_ratio = 0.0


def test_seeded_sampling_repeats_bit_for_bit(dev):
    g = make_generator("dense", dev)
    prompts = gr.gnn_prompts()
    for kw in (dict(sampling_topk=5), dict(sampling_topp=0.8)):
        runs = [g.generate(prompts, 12, sampling=True, temperature=0.8, unk_penalty=0.5, seed=s, **kw) for s in (7, 7, 8)]
        a, b, c = [[x.cpu().numpy() for x in r] for r in runs]
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert not np.array_equal(a[0], c[0])


# ---------------------------------------------------------------------------------------------------- the command line
@pytest.fixture(scope="module")
def cli(tmp_path_factory, dev):
    """DATA/test.bin/.idx, a GNN-LM checkpoint (the base LM under decoder.*, beside decoder.hgt_decoder.* and decoder.tgt_quantizer.*)
    and D/quantized-keys.npy; the index is handed over as an object."""
    from gnnlm_amd.generate_gnn import IndexSearch
    from gnnlm_amd.knn_model import ExactIndex
    root = tmp_path_factory.mktemp("generate_gnn")
    m, _ = dr.gen_model(gr.GNN_SEED, "dense")
    st = gr.gnn_store()
    c = dict(dr.GEN_MODEL, act="relu", emb_norm=False)
    rs = np.random.RandomState(8)
    sizes = [12, 20, 9, 23]
    tokens = rs.randint(4, dr.GEN_MODEL["V"], size=sum(sizes)).astype(np.int64)
    tokens[np.cumsum(sizes) - 1] = tr.EOS
    base.write_split(root, "test", tokens, sizes)
    sd = base.state_dict_of(m, "qkv")
    sd.update({"decoder.hgt_decoder." + k: torch.as_tensor(v) for k, v in st["sd"].items()})
    sd.update({"decoder.tgt_quantizer.centroids_torch": torch.from_numpy(st["cen"]), "decoder.tgt_quantizer.A": torch.from_numpy(st["A"]),
               "decoder.tgt_quantizer.b": torch.from_numpy(st["b"])})
    torch.save({"args": base.args_of(m, c, graph_layer=gr.GNN_LAYERS), "model": sd}, root / "gnn.pt")
    (root / "dstore").mkdir()
    np.save(root / "dstore" / "quantized-keys.npy", st["codes"])
    knn = IndexSearch(ExactIndex(t(st["keys"], dev), "ip", False, dev))
    return {"root": root, "ckpt": root / "gnn.pt", "tokens": tokens, "knn": knn, "dstore": root / "dstore"}


def drive(cli, extra, module="generate_gnn"):
    mod = __import__(f"gnnlm_amd.{module}", fromlist=["get_parser"])
    args = mod.get_parser().parse_args([str(cli["root"]), "--path", str(cli["ckpt"])] + extra)
    args.knn_model = cli["knn"]
    buf = io.StringIO()
    return mod.main(args, file=buf), buf.getvalue().splitlines()


GNN_FLAGS = ["--gcn-k", str(gr.GNN_KG), "--neighbor-context", "1"]


def test_command_line_round_trip(dev, cli, tmp_path):
    out = tmp_path / "gen.npz"
    res, lines = drive(cli, GNN_FLAGS + ["--dstore-dir", str(cli["dstore"]), "--n-prompts", "3", "--prompt-len", "8", "--max-len-b", "10",
                                         "--out", str(out)])
    assert [l.split("\t")[0] for l in lines] == ["S-0", "H-0", "S-1", "H-1", "S-2", "H-2"]
    for i in range(3):
        assert lines[2 * i].split("\t")[1].split() == [str(int(v)) for v in cli["tokens"][8 * i:8 * i + 8]]
        _, score, text = lines[2 * i + 1].split("\t")
        n = int(res["lengths"][i])
        assert text.split() == [str(int(v)) for v in res["tokens"][i, :n]]
        assert abs(float(score) - float(res["logp"][i, :n].astype(np.float64).sum())) <= 1e-9
    z = np.load(out)
    assert np.array_equal(z["tokens"], res["tokens"]) and np.array_equal(z["logp"], res["logp"]) and np.array_equal(z["lengths"], res["lengths"])
    assert z["prompts"].shape == (3, 9) and (z["prompts"][:, 0] == tr.EOS).all()
    # the loaded checkpoint is the model of the direct test: the same generator on the same prompts gives the same text
    g = make_generator("dense", dev)
    direct = g.generate(res["prompts"], 10)[0].cpu().numpy()
    assert np.array_equal(direct, res["tokens"])
    # sampling and --fp16 through the same driver
    res_s, lines = drive(cli, GNN_FLAGS + ["--dstore-dir", str(cli["dstore"]), "--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "6",
                                           "--sampling", "--sampling-topk", "10", "--temperature", "0.8", "--seed", "3", "--fp16"])
    assert len(lines) == 4 and res_s["tokens"].shape == (2, 6) and np.isfinite(res_s["logp"]).all()


@pytest.mark.parametrize("flags,exc,word", [
    (["--beam", "2"], ValueError, "--beam"),
    (["--knnlm"], ValueError, "--knnlm"),
    (["--sweep-lmbda", "0.1,0.2"], ValueError, "--sweep-lmbda"),
    (["--sweep-temperature", "1,2"], ValueError, "--sweep-temperature"),
    (["--sweep-k", "8,16"], ValueError, "--sweep-k"),
    (["--reinit-nfeat"], ValueError, "--reinit-nfeat"),
    (["--store", "sharded"], ValueError, "--store sharded"),
    (["--store", "peer"], ValueError, "--store peer"),
    (["--min-len", "2"], ValueError, "--min-len"),
    (["--no-repeat-ngram-size", "3"], ValueError, "--no-repeat-ngram-size"),
    (["--intra-context", "16"], ValueError, "--intra-context"),
    (["--gcn-context-window", "8"], ValueError, "--gcn-context-window"),
    (["--sampling"], ValueError, "--sampling-topk"),
])
def test_command_line_refusals(dev, cli, flags, exc, word):
    with pytest.raises(exc, match=word):
        drive(cli, GNN_FLAGS + ["--dstore-dir", str(cli["dstore"]), "--max-len-b", "4"] + flags)


def test_more_than_one_process_is_refused_and_generate_still_refuses_graph(dev, cli, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one process"):
        drive(cli, GNN_FLAGS + ["--dstore-dir", str(cli["dstore"]), "--max-len-b", "4"])
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="--graph"):
        drive(cli, ["--max-len-b", "4", "--graph"], module="generate")
    with pytest.raises(ValueError, match="--graph"):
        drive(cli, ["--max-len-b", "4", "--graph"], module="beam_search")
