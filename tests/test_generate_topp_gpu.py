"""Nucleus (top-p) sampling through ``Generator.generate`` and the command line, on the toy models of tests/decode_ref.py (V = 50, both
heads): seeded runs, every pick inside the float64 nucleus of the row it was drawn from, ``sampling_topp`` -> 0 is the greedy chain, the
kNN mix, the driver, and a captured pick + step pair.  GPU only."""
import numpy as np
import pytest
import torch

import decode_ref as dr
import test_generate_gpu as tg
import topp_ref as tp
from test_generate_gpu import cli, dev, t  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NEW = 16
SLACK = 1e-4                            # covers the 2e-5 log-prob parity bar between the device rows and the float64 chain


def mass_in_front(lp64, token):
    """The mass of the entries in front of ``token`` in the order of the row (larger value first, then smaller id)."""
    o = tp.order(lp64)
    pos = int(np.nonzero(o == token)[0][0])
    return float(tp.masses(lp64)[o[:pos]].sum())


@pytest.mark.parametrize("head", dr.GEN_HEADS)
def test_seeded_runs_and_every_pick_inside_the_float64_nucleus(dev, head):
    from gnnlm_amd.generate import Generator
    seed, p = 301, 0.8
    lm = tg.gen_lm(seed, head, dev)
    m, hw = dr.gen_model(seed, head)
    g = Generator(lm)
    prompts = dr.gen_prompts(seed)
    a, b, c = [[x.cpu().numpy() for x in g.generate(prompts, NEW, sampling=True, sampling_topp=p, seed=s)] for s in (21, 21, 22)]
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert not np.array_equal(a[0], c[0])
    assert g.mean_nucleus is not None and 1.0 <= g.mean_nucleus <= dr.GEN_MODEL["V"]
    tokens, logp, lengths = a
    worst, sizes = 0.0, []
    for i, prompt in enumerate(prompts):
        n = int(lengths[i])
        rows = dr.incremental_rows(m, prompt + tokens[i, :n - 1].tolist())["out"][len(prompt) - 1:]
        assert (tokens[i, n:] == dr.PAD).all() and (logp[i, n:] == 0).all()
        for s in range(n):
            lp64 = dr.dense_logp(m, rows[s]) if hw is None else dr.adaptive_dense_logp(rows[s], **hw)
            lp64[dr.PAD] = -np.inf
            front = mass_in_front(lp64, int(tokens[i, s]))
            assert front < p * (1 + SLACK), (i, s, front)
            worst = max(worst, abs(float(logp[i, s]) - lp64[tokens[i, s]]))
            sizes.append(tp.nucleus(lp64, p)[1])
    print(f"{head}: max |returned logp - float64 logp of the pick| = {worst:.3e}; float64 nucleus sizes {min(sizes)} .. {max(sizes)}, "
          f"device mean {g.mean_nucleus:.2f}")
    assert worst <= tg.LOGP_BAR
    assert max(sizes) > 1                                       # the nucleus is not the arg-max alone: this is not greedy in disguise


@pytest.mark.parametrize("head", dr.GEN_HEADS)
@pytest.mark.parametrize("seed", dr.GEN_SEEDS)
def test_a_vanishing_p_is_the_greedy_chain(dev, seed, head):
    from gnnlm_amd.generate import Generator
    lm = tg.gen_lm(seed, head, dev)
    prompts = dr.gen_prompts(seed)
    tokens, logp, lengths = [x.cpu().numpy() for x in Generator(lm).generate(prompts, dr.GEN_NEW, sampling=True, sampling_topp=1e-6, seed=5)]
    for i in range(len(prompts)):
        want, want_lp, _, _ = dr.gen_chain(seed, i, head)
        n = int(lengths[i])
        assert n == len(want) and tokens[i, :n].tolist() == want
        assert float(np.abs(logp[i, :n] - want_lp).max()) <= tg.LOGP_BAR


def test_knn_mix_is_finite_and_in_the_nucleus(dev, tmp_path):
    from gnnlm_amd.generate import Generator
    seed, p = 301, 0.7
    lm = tg.gen_lm(seed, "dense", dev)
    knn, _, _ = tg.knn_fixture(seed, dev, tmp_path)
    g = Generator(lm, knn, lmbda=tg.LMBDA, knn_temperature=tg.KNN_T)
    prompts = dr.gen_prompts(seed)
    tokens, logp, lengths = g.generate(prompts, 12, sampling=True, sampling_topp=p, seed=4)
    assert bool(torch.isfinite(logp).all()) and bool((lengths >= 1).all())
    tokens, logp, lengths = tokens.cpu().numpy(), logp.cpu().numpy(), lengths.cpu().numpy()
    # replay the text: every pick lies in the nucleus of the mixed distribution it was drawn from and carries its log-prob
    off = np.concatenate([[0], np.cumsum([len(q) for q in prompts])])
    cache = lm.new_cache(len(prompts), max(len(q) for q in prompts) + 12)
    x, extra = lm.prefill(t(np.concatenate(prompts).astype(np.int64), dev), off, cache)
    last = t(off[1:] - 1, dev)
    x, extra = x[last], {"inner_states": [extra["inner_states"][-1][last]]}
    for s in range(12):
        lp = g.next_log_probs(x, extra).cpu().numpy()
        for i in range(len(prompts)):
            if s < lengths[i]:
                assert mass_in_front(lp[i].astype(np.float64), int(tokens[i, s])) < p * (1 + SLACK)
                assert abs(float(lp[i, tokens[i, s]]) - float(logp[i, s])) <= tg.LOGP_BAR
        x, extra = lm.step(t(tokens[:, s].copy(), dev), cache)


def test_command_line(dev, cli, tmp_path):
    out = tmp_path / "topp.npz"
    flags = ["--n-prompts", "3", "--prompt-len", "8", "--max-len-b", "10", "--sampling", "--sampling-topp", "0.9", "--seed", "3", "--out", str(out)]
    res, lines = tg.drive(cli, flags)
    assert [l.split("\t")[0] for l in lines] == ["S-0", "H-0", "S-1", "H-1", "S-2", "H-2"]
    z = np.load(out)
    assert np.array_equal(z["tokens"], res["tokens"]) and np.array_equal(z["logp"], res["logp"]) and z["tokens"].shape == (3, 10)
    again, _ = tg.drive(cli, flags)
    assert np.array_equal(again["tokens"], res["tokens"])
    whole, _ = tg.drive(cli, flags[:-4] + ["--sampling-topp", "1.5"])             # P >= 1: the whole vocabulary
    assert np.isfinite(whole["logp"]).all()
    for bad, word in ((["--sampling-topp", "0.9"], "--sampling"), (["--sampling", "--sampling-topp", "nan"], "--sampling-topp"),
                      (["--sampling", "--sampling-topk", "5", "--sampling-topp", "0.9"], "--sampling-topp")):
        with pytest.raises(ValueError, match=word):
            tg.drive(cli, ["--max-len-b", "4"] + bad)


def test_captured_pick_and_step_replay_the_eager_loop(dev):
    from gnnlm_amd import ops
    lm = tg.gen_lm(302, "dense", dev)
    prompts = dr.gen_prompts(302)
    B, N, p = len(prompts), 8, 0.8
    off = np.concatenate([[0], np.cumsum([len(q) for q in prompts])])
    toks = t(np.concatenate(prompts).astype(np.int64), dev)
    bound = max(len(q) for q in prompts) + N + 2
    u_all = torch.rand(N + 1, B, generator=torch.Generator(device=dev).manual_seed(9), device=dev)

    def one(cache, tok, state):
        """step + head + nucleus pick, everything into preallocated tensors; the step's uniform numbers are row state["i"] of u_all"""
        x, _ = lm.step(tok, cache, want_inner=False, want_ffn_input=False, max_len=bound)
        lp = lm.head.log_probs(x)
        lp[:, dr.PAD] = float("-inf")
        torch.index_select(u_all, 0, state["i"], out=state["u"])
        state["i"] += 1
        ops.sample_topp(lp, p, state["u"][0], pad=dr.PAD, eos=dr.EOS, done=cache.done, out=state["next"], out_logp=state["lp"],
                        n_keep=state["n_keep"])
        tok.copy_(state["next"])

    def start():
        cache = lm.new_cache(B, bound)
        lm.prefill(toks, off, cache)
        state = {"next": torch.empty(B, dtype=torch.int64, device=dev), "lp": torch.zeros(B, device=dev), "u": torch.empty(1, B, device=dev),
                 "i": torch.zeros(1, dtype=torch.int64, device=dev), "n_keep": torch.zeros(B, dtype=torch.int32, device=dev)}
        tok = t(np.asarray([q[-1] for q in prompts], np.int64), dev)
        one(cache, tok, state)                                   # the warm-up step
        return cache, tok, state

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cache, tok, state = start()
        eager = []
        for _ in range(N):
            one(cache, tok, state)
            eager.append((tok.clone(), state["lp"].clone(), state["n_keep"].clone()))
        eager_len = cache.len.clone()
        cache2, tok2, state2 = start()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one(cache2, tok2, state2)
        replayed = []
        for _ in range(N):
            graph.replay()
            replayed.append((tok2.clone(), state2["lp"].clone(), state2["n_keep"].clone()))
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for (a, alp, an), (b, blp, bn) in zip(eager, replayed):
        assert torch.equal(a, b) and torch.equal(alp.view(torch.int32), blp.view(torch.int32)) and torch.equal(an, bn)
    assert torch.equal(cache2.len, eager_len) and int(cache2.n_bad.item()) == 0
    assert min(int(n.min()) for _, _, n in eager) >= 1
