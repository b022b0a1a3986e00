"""Beam search from the base LM end to end: BeamGenerator against beam_search_ref driven by the float64 restatement of the model
(tests/beam_ref.py, tests/decode_ref.py) -- tokens and order exact, raw scores within steps x 2e-5 (the log-prob bar of README
"Parity", accumulated over the hypothesis) -- on seeds whose float64 run keeps every candidate and final-score pair 1e-3 apart
(tests/test_beam_ref_cpu.py checks that), so a flipped candidate is a defect.  Every hypothesis is scored again by prefill + the
plain step; beam 1 is the greedy Generator; a captured select + step pair replays the eager loop bit for bit; the kNN mix and the
command line run through the driver.  GPU only."""
import io
import os

import numpy as np
import pytest
import torch

import beam_ref as br
import decode_ref as dr
import test_transformer_lm_gpu as base
import transformer_lm_ref as tr

pytestmark = pytest.mark.gpu

LOGP_BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def gen_lm(seed, head, dev):
    from gnnlm_amd.transformer_lm import TransformerLM
    m, hw = dr.gen_model(seed, head)
    c = dict(dr.GEN_MODEL, act="relu", emb_norm=False)
    if hw is None:
        return TransformerLM.from_state_dict(base.state_dict_of(m, "qkv"), base.args_of(m, c), dev)
    cut = ",".join(str(v) for v in dr.GEN_CUT)
    args = base.args_of(m, c, adaptive_softmax_cutoff=cut, adaptive_input=True, adaptive_input_cutoff=cut, adaptive_input_factor=2,
                        tie_adaptive_weights=True)
    return TransformerLM.from_state_dict(base.state_dict_of(m, "qkv", list(zip(hw["emb"], hw["proj"])), hw["class_proj"]), args, dev)


def rescore(g, prompt, hyps, unk_penalty, dev):
    """The cumulative log-probabilities of the hypotheses of one prompt under prefill + the plain step (no table): [n_hyps][len]."""
    lm, n = g.lm, len(hyps)
    width = max(len(h["tokens"]) for h in hyps)
    toks = np.full((n, width), 4, np.int64)
    for i, h in enumerate(hyps):
        toks[i, :len(h["tokens"])] = h["tokens"]
    cache = lm.new_cache(n, len(prompt) + width)
    off = np.arange(n + 1) * len(prompt)
    x, extra = lm.prefill(t(np.tile(np.asarray(prompt, np.int64), n), dev), off, cache)
    x = x[t(off[1:] - 1, dev)]
    cum = np.zeros((n, width))
    for s in range(width):
        lp = g.next_log_probs(x, {}, 1.0, unk_penalty)
        cum[:, s] = (cum[:, s - 1] if s else 0.0) + lp[torch.arange(n, device=dev), t(toks[:, s], dev)].double().cpu().numpy()
        if s + 1 < width:
            x, _ = lm.step(t(toks[:, s].copy(), dev), cache)
    return cum


# ---------------------------------------------------------------------------------------------------- 1. against float64, and itself
@pytest.mark.parametrize("head,beam", sorted(br.E2E_SEEDS))
def test_beam_search_against_the_float64_run(dev, head, beam):
    from gnnlm_amd.beam_search import BeamGenerator
    m, hw, prompts, want, info = br.e2e_case(head, beam)
    assert min(info["step_margin"], info["final_margin"]) >= br.E2E_MARGIN
    g = BeamGenerator(gen_lm(br.E2E_SEEDS[head, beam], head, dev))
    got = g.generate(prompts, br.E2E["max_new"], beam=beam, lenpen=br.E2E["lenpen"], min_len=br.E2E["min_len"], unk_penalty=br.E2E["unk_penalty"])
    for i, p in enumerate(prompts):
        assert [h["tokens"].tolist() for h in got[i]] == [h["tokens"].tolist() for h in want[i]], (i, got[i], want[i])
        again = rescore(g, p, got[i], br.E2E["unk_penalty"], dev)
        for f, (a, b) in enumerate(zip(got[i], want[i])):
            n = len(a["tokens"])
            e_raw, e_score = abs(a["raw"] - b["raw"]), abs(a["score"] - b["score"])
            e_pos = float(np.abs(a["positional_scores"] - b["positional_scores"]).max())
            cum = np.cumsum(a["positional_scores"].astype(np.float64))
            e_self = float(np.abs(again[f, :n] - cum).max())
            print(f"{head} beam {beam} prompt {i} hypothesis {f}: {n} tokens, |d raw| = {e_raw:.2e}, |d score| = {e_score:.2e}, "
                  f"max |d positional| = {e_pos:.2e}, scored again max |d cumulative| = {e_self:.2e} (bar {n * LOGP_BAR:.1e})")
            assert e_raw <= n * LOGP_BAR and e_score <= n * LOGP_BAR and e_pos <= 2 * n * LOGP_BAR
            assert e_self <= n * LOGP_BAR
            assert abs(a["score"] - a["raw"] / n ** br.E2E["lenpen"]) <= 1e-6 * abs(a["raw"])


def test_beam_one_is_the_greedy_generator(dev):
    from gnnlm_amd.beam_search import BeamGenerator
    from gnnlm_amd.generate import Generator
    lm = gen_lm(301, "adaptive", dev)
    prompts, n = dr.gen_prompts(301), 12
    tokens, logp, lengths = [x.cpu().numpy() for x in Generator(lm).generate(prompts, n)]
    got = BeamGenerator(lm).generate(prompts, n, beam=1)
    for i in range(len(prompts)):
        assert len(got[i]) == 1
        h, k = got[i][0]["tokens"].tolist(), int(lengths[i])
        greedy = tokens[i, :k].tolist()
        assert h == greedy if greedy[-1] == dr.EOS else h == greedy + [dr.EOS], (i, h, greedy)
        # the differences of a float32 cumulative history: two roundings at magnitudes below 64 (ulp 3.8e-6) each
        assert got[i][0]["positional_scores"][0] == logp[i, 0] and np.abs(got[i][0]["positional_scores"][:k] - logp[i, :k]).max() <= 1e-5


# ---------------------------------------------------------------------------------------------------- 2. a captured select + step
def test_captured_select_and_step_replay_the_eager_loop(dev):
    from gnnlm_amd import ops
    from gnnlm_amd.beam_search import BeamGenerator
    seed, beam, max_new, N = br.E2E_SEEDS["dense", 5], 5, 12, 8
    lm = gen_lm(seed, "dense", dev)
    g = BeamGenerator(lm)
    prompts = dr.gen_prompts(seed)[1:]
    bound = max(len(p) for p in prompts) + max_new

    def cand(run, x, step):
        """the candidates of a step, eagerly, under the settings of the float64 run (whose sentences all last to the length limit)"""
        return g.candidates(run, x, {}, step, min_len=br.E2E["min_len"], unk_penalty=br.E2E["unk_penalty"])

    def pair(run, xbuf):
        ops.beam_select(run["cand"][0], run["cand"][1], run["state"], src=run["table"], eos=dr.EOS, pad=dr.PAD)
        x, _ = lm.step(run["state"].next, run["cache"], want_inner=False, want_ffn_input=False, max_len=bound, src=run["table"])
        xbuf.copy_(x)

    def start():
        run = g.start(prompts, max_new, beam)
        val, idx = cand(run, run["x"], 0)
        ops.beam_select(val, idx, run["state"], src=run["table"], eos=dr.EOS, pad=dr.PAD)                # the first step: beam_in = 1
        x, _ = lm.step(run["state"].next, run["cache"], want_inner=False, want_ffn_input=False, max_len=bound, src=run["table"])
        xbuf = x.clone()
        cand(run, xbuf, 1)
        pair(run, xbuf)                                          # the warm-up of the pair itself (step 1)
        return run, xbuf

    def snap(run, xbuf):
        s = run["state"]
        return [v.clone() for v in (s.next, s.parent, s.score, s.t, xbuf, run["table"], run["cache"].len)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run, xbuf = start()
        eager = []
        for s in range(N):
            cand(run, xbuf, 2 + s)
            pair(run, xbuf)
            eager.append(snap(run, xbuf))
        run2, xbuf2 = start()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pair(run2, xbuf2)
        replayed = []
        for s in range(N):
            cand(run2, xbuf2, 2 + s)
            graph.replay()
            replayed.append(snap(run2, xbuf2))
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for s, (a, b) in enumerate(zip(eager, replayed)):
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), s
    assert int(run2["cache"].n_bad.item()) == 0 and run2["state"].t.tolist() == [2 + N] * len(prompts)
    assert eager[-1][6].tolist() == [len(p) + 2 + N for p in prompts for _ in range(beam)]
    # every slot is alive at every recorded step, and the best hypothesis so far is a prefix of the float64 run's best
    _, _, _, want, _ = br.e2e_case("dense", 5)
    st = {k: getattr(run2["state"], k).cpu().numpy() for k in ("hist_tok", "hist_par", "hist_score")}
    assert (st["hist_tok"][:, :2 + N] != dr.PAD).all() and int(run2["state"].finished.sum()) == 0
    finals = {tuple(h["tokens"][:2 + N].tolist()) for hs in want for h in hs}
    alive = {tuple(br.walk(st, b, 1 + N, j)[0]) for b in range(len(prompts)) for j in range(beam)}
    assert finals <= alive


# ---------------------------------------------------------------------------------------------------- 3. the kNN mix
N_KEYS = 200


def knn_fixture(seed, dev, root):
    """A KNNModel over 200 keys (an ExactIndex, inner product): scaled inner_states[-1] rows of the model itself with seeded labels."""
    from gnnlm_amd.knn_model import ExactIndex, KNNModel
    import test_base_knnlm_gpu as bk
    m, _ = dr.gen_model(seed, "dense")
    rs = np.random.RandomState(seed + 3)
    stream = rs.randint(4, dr.GEN_MODEL["V"], size=N_KEYS).astype(np.int64)
    keys = (0.05 * tr.forward(m, stream, np.arange(0, N_KEYS + 1, 50))["last_inner"]).astype(np.float32)
    vals = rs.randint(4, dr.GEN_MODEL["V"], size=N_KEYS).astype(np.int64)
    store = os.path.join(str(root), "store")
    bk.write_store(store, keys, vals, dr.GEN_MODEL["V"])
    return KNNModel(os.path.join(store, "faiss_store.ip"), store, k=N_KEYS, no_load_keys=True, metric_type="do_not_recomp_ip",
                    index=ExactIndex(torch.from_numpy(keys), "ip", False, dev), device=dev)


# ---------------------------------------------------------------------------------------------------- 4. the command line
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    root = tmp_path_factory.mktemp("beam")
    m, _ = dr.gen_model(301, "dense")
    c = dict(dr.GEN_MODEL, act="relu", emb_norm=False)
    rs = np.random.RandomState(8)
    sizes = [12, 20, 9, 23]
    tokens = rs.randint(4, dr.GEN_MODEL["V"], size=sum(sizes)).astype(np.int64)
    tokens[np.cumsum(sizes) - 1] = tr.EOS
    base.write_split(root, "test", tokens, sizes)
    torch.save({"args": base.args_of(m, c), "model": base.state_dict_of(m, "qkv")}, root / "base.pt")
    return {"root": root, "ckpt": root / "base.pt", "tokens": tokens}


def drive(cli, extra, knn=None):
    from gnnlm_amd.beam_search import get_parser, main
    args = get_parser().parse_args([str(cli["root"]), "--path", str(cli["ckpt"])] + extra)
    if knn is not None:
        args.knn_model = knn
    buf = io.StringIO()
    return main(args, file=buf), buf.getvalue().splitlines()


def test_command_line(dev, cli, tmp_path):
    out = tmp_path / "beam.npz"
    res, lines = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "6", "--beam", "3", "--nbest", "2", "--out", str(out)])
    assert [l.split("\t")[0] for l in lines] == ["S-0", "H-0", "P-0", "H-0", "P-0", "S-1", "H-1", "P-1", "H-1", "P-1"]
    for i in range(2):
        assert lines[5 * i].split("\t")[1].split() == [str(int(v)) for v in cli["tokens"][8 * i:8 * i + 8]]
        hs = res["hypotheses"][i]
        assert len(hs) == 2 and hs[0]["score"] >= hs[1]["score"]
        for f, h in enumerate(hs):
            _, score, text = lines[5 * i + 1 + 2 * f].split("\t")
            assert text.split() == [str(int(v)) for v in h["tokens"]] and abs(float(score) - h["score"]) <= 1e-9
            pos = [float(v) for v in lines[5 * i + 2 + 2 * f].split("\t")[1].split()]
            assert len(pos) == len(h["tokens"]) and np.abs(np.asarray(pos) - h["positional_scores"]).max() <= 5.1e-5
    z = np.load(out)
    assert z["tokens"].shape == (2, 2, 7) and z["prompts"].shape == (2, 9) and (z["prompts"][:, 0] == tr.EOS).all()
    for i in range(2):
        for f, h in enumerate(res["hypotheses"][i]):
            n = int(z["lengths"][i, f])
            assert z["tokens"][i, f, :n].tolist() == h["tokens"].tolist() and float(z["scores"][i, f]) == np.float32(h["score"])
    # the default is the reference's --beam 5; with the default --nbest 1 one hypothesis per prompt, the float64 run's best
    res5, lines = drive(cli, ["--n-prompts", "1", "--prompt-len", "8", "--max-len-b", "6"])
    assert [l.split("\t")[0] for l in lines] == ["S-0", "H-0", "P-0"]
    m, _ = dr.gen_model(301, "dense")
    prompt = [tr.EOS] + [int(v) for v in cli["tokens"][:8]]
    want, info = br.beam_search_ref(br.IncLprobs(m), [prompt], 5, 6)
    assert min(info["step_margin"], info["final_margin"]) >= br.E2E_MARGIN
    assert res5["hypotheses"][0][0]["tokens"].tolist() == want[0][0]["tokens"].tolist()
    # --score-prompt: the prompt's cumulative log-probability and length as the reference's prefix run counts them
    res_p, _ = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "4", "--beam", "2", "--score-prompt", "--lenpen", "0.7"])
    for i in range(2):
        prompt = [tr.EOS] + [int(v) for v in cli["tokens"][8 * i:8 * i + 8]]
        rows = dr.incremental_rows(m, prompt)["out"]
        ref = sum(dr.dense_logp(m, rows[u])[prompt[u + 1]] for u in range(8))
        e = abs(float(res_p["score0"][i]) - ref)
        print(f"--score-prompt {i}: log p(prompt) = {ref:.6f}, |dev - ref64| = {e:.2e}")
        assert e <= 8 * LOGP_BAR and int(res_p["len0"][i]) == 8
        h = res_p["hypotheses"][i][0]
        assert abs(h["score"] - h["raw"] / (8 + len(h["tokens"])) ** 0.7) <= 1e-5 and h["raw"] < res_p["score0"][i]
        assert abs(float(h["positional_scores"].astype(np.float64).sum()) - (h["raw"] - float(res_p["score0"][i]))) <= 1e-4
    # --fp16, the other flags, and kNN through the same driver
    res_h, lines = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "5", "--beam", "4", "--fp16", "--temperature", "0.8",
                               "--unkpen", "0.5", "--min-len", "3", "--unnormalized"])
    assert len(lines) == 6 and all(len(h[0]["tokens"]) >= 3 and h[0]["score"] == h[0]["raw"] for h in res_h["hypotheses"])
    knn = knn_fixture(301, dev, tmp_path)
    res_k, lines = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "5", "--beam", "3", "--nbest", "3", "--knnlm", "--k", str(N_KEYS),
                               "--lmbda", "0.25", "--knn-temperature", "1"], knn=knn)
    assert all(len(hs) == 3 and all(np.isfinite(h["score"]) and np.isfinite(h["positional_scores"]).all() for h in hs) for hs in res_k["hypotheses"])
    assert res_k["hypotheses"][0][0]["tokens"].tolist() != [] and len(lines) == 2 * (1 + 2 * 3)


@pytest.mark.parametrize("flags,exc,word", [
    (["--sampling"], ValueError, "--sampling"),
    (["--sampling-topk", "5"], ValueError, "--sampling"),
    (["--sampling-topp", "0.9"], ValueError, "--sampling-topp"),
    (["--no-repeat-ngram-size", "3"], ValueError, "--no-repeat-ngram-size"),
    (["--graph"], ValueError, "--graph"),
    (["--sweep-lmbda", "0.1,0.2"], ValueError, "--sweep-lmbda"),
    (["--sweep-temperature", "1,2"], ValueError, "--sweep-temperature"),
    (["--sweep-k", "8,16"], ValueError, "--sweep-k"),
    (["--beam", "25"], ValueError, "--beam"),                  # 2 * beam > V - 1 = 49
    (["--beam", "33"], ValueError, "--beam"),
    (["--beam", "2", "--nbest", "3"], ValueError, "--nbest"),
    (["--score-prompt", "--knnlm", "--dstore-dir", "D", "--index-file", "F"], ValueError, "--score-prompt"),
    (["--knnlm"], ValueError, "--knnlm"),
])
def test_command_line_refusals(dev, cli, flags, exc, word):
    with pytest.raises(exc, match=word):
        drive(cli, ["--max-len-b", "4"] + flags)


def test_more_than_one_process_is_refused_and_generate_still_refuses_beam(dev, cli, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one process"):
        drive(cli, ["--max-len-b", "4"])
    monkeypatch.delenv("WORLD_SIZE")
    from gnnlm_amd.generate import get_parser, main
    args = get_parser().parse_args([str(cli["root"]), "--path", str(cli["ckpt"]), "--beam", "2"])
    with pytest.raises(ValueError, match="--beam.*beam_search"):
        main(args, file=io.StringIO())
