"""Incremental decoding of the base LM end to end: prefill + step against the float64 restatement (teacher-forced), greedy generation
against the reference chains of tests/decode_ref.py token for token, seeded top-k sampling, a captured step, the refusals, the kNN
mix and the command line.  GPU only.

Bars: features FEATURE_BAR (5e-5, transformer_lm_ref.py); precision 3 the rule of test_transformer_lm_gpu.py (FP16_SHARE of the
rounding's own effect, against the restatement with float16-rounded operands); log-probs 2e-5 (README "Parity")."""
import io
import os

import numpy as np
import pytest
import torch

import decode_ref as dr
import test_transformer_lm_gpu as base
import transformer_lm_ref as tr

pytestmark = pytest.mark.gpu

PROMPTS, STEPS, EMPTY_STEPS = [1, 31, 33, 70], 40, 41
LOGP_BAR = 2e-5
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def forced_case(case):
    """-> (model, tokens [sum(PROMPTS) + 4 * STEPS] packed per sequence, offsets of the full sequences, float64 refs by half_gemm)."""
    if case not in _REF:
        c = tr.GPU_CASES[case]
        m = tr.make_model(pos_rows=tr.PAD + 1 + max(PROMPTS) + STEPS, **c)
        lens = [n + STEPS for n in PROMPTS]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        tokens = np.random.RandomState(c["seed"] + 9).randint(0, c["V"], size=int(off[-1])).astype(np.int64)
        _REF[case] = (m, tokens, off, {})
    m, tokens, off, refs = _REF[case]
    return m, tokens, off, refs


def forced_ref(case, half):
    m, tokens, off, refs = forced_case(case)
    if half not in refs:
        refs[half] = tr.forward(m, tokens, off, torch.float64, half)
    return refs[half]


KEYS = ("out", "last_inner", "last_ffn_input")


def unpack(x, extra):
    return {"out": x.cpu().numpy(), "last_inner": extra["inner_states"][-1].cpu().numpy(), "last_ffn_input": extra["last_ffn_input"].cpu().numpy()}


# ---------------------------------------------------------------------------------------------------- 1. teacher-forced parity
@pytest.mark.parametrize("precision", [None, "fp16"], ids=["f32", "fp16"])
@pytest.mark.parametrize("case", [1, 2])
def test_prefill_and_steps_against_restatement(dev, case, precision):
    m, tokens, off, _ = forced_case(case)
    lm = base.build(m, dev, precision)
    B = len(PROMPTS)
    p_rows = np.concatenate([np.arange(off[b], off[b] + PROMPTS[b]) for b in range(B)])
    p_off = np.concatenate([[0], np.cumsum(PROMPTS)])
    cache = lm.new_cache(B, max(PROMPTS) + STEPS)
    x, extra = lm.prefill(t(tokens[p_rows], dev), p_off, cache)
    got = {k: [v] for k, v in unpack(x, extra).items()}
    rows = [p_rows]
    x2, extra2 = lm.extract_features(t(tokens[p_rows], dev), p_off)
    for k, v in unpack(x2, extra2).items():
        assert np.array_equal(v.view(np.uint32), got[k][0].view(np.uint32)), k          # prefill is extract_features, bit for bit
    assert cache.len.tolist() == PROMPTS and cache.steps == max(PROMPTS)
    for s in range(STEPS):
        r = off[:-1] + np.asarray(PROMPTS) + s
        x, extra = lm.step(t(tokens[r], dev), cache)
        for k, v in unpack(x, extra).items():
            got[k].append(v)
        rows.append(r)
    assert cache.len.tolist() == [n + STEPS for n in PROMPTS] and int(cache.n_bad.item()) == 0
    lm.check_tokens()
    # 41 steps from an empty cache
    cache0 = lm.new_cache(B, EMPTY_STEPS)
    got0, rows0 = {k: [] for k in KEYS}, []
    for s in range(EMPTY_STEPS):
        r = off[:-1] + s
        x, extra = lm.step(t(tokens[r], dev), cache0)
        for k, v in unpack(x, extra).items():
            got0[k].append(v)
        rows0.append(r)
    assert cache0.len.tolist() == [EMPTY_STEPS] * B
    rows, rows0 = np.concatenate(rows), np.concatenate(rows0)
    ref64 = forced_ref(case, False)
    for name, g, rr in (("prefill + steps", got, rows), ("empty cache", got0, rows0)):
        for k in KEYS:
            dev_rows = np.concatenate(g[k])
            if precision is None:
                e = tr.rel_err(dev_rows, ref64[k][rr])
                print(f"case {case} {name} {k}: max|dev - ref64| / max|ref64| = {e:.3e}")
                assert e <= tr.FEATURE_BAR
            else:
                ref16 = forced_ref(case, True)
                share = tr.rms(dev_rows - ref16[k][rr]) / tr.rms(ref64[k][rr] - ref16[k][rr])
                print(f"case {case} {name} precision 3 {k}: rms(dev - rounded ref64) / rms(effect of the rounding) = {share:.3f}")
                assert share <= tr.FP16_SHARE


def test_sinusoidal_table_is_sized_once_for_the_cache(dev):
    """A loaded checkpoint's sinusoidal table (130 rows here) is grown by new_cache to the positions the cache can hold; no step
    replaces it -- a step that did would build and upload a table per token -- and the positions beyond the first table are right."""
    lm = gen_lm(301, "dense", dev)
    m, _ = dr.gen_model(301, "dense")
    assert not lm.learned_pos and lm.pos.shape[0] == 130
    n, steps, cap = 140, 12, 200
    cache = lm.new_cache(2, cap)
    table = lm.pos
    assert table.shape[0] == tr.PAD + 1 + cap
    tokens = np.random.RandomState(5).randint(4, dr.GEN_MODEL["V"], size=2 * (n + steps)).astype(np.int64)
    off = np.asarray([0, n + steps, 2 * (n + steps)])
    ref = tr.forward(dict(m, P=tr.sinusoidal_table(tr.PAD + 1 + cap, dr.GEN_MODEL["d"])), tokens, off)["out"]
    p_rows = np.concatenate([np.arange(off[b], off[b] + n) for b in range(2)])
    x, _ = lm.prefill(t(tokens[p_rows], dev), [0, n, 2 * n], cache)
    got, rows = [x.cpu().numpy()], [p_rows]
    for s in range(steps):
        r = off[:-1] + n + s
        x, _ = lm.step(t(tokens[r], dev), cache)
        assert lm.pos is table                                   # the same tensor: nothing was rebuilt
        got.append(x.cpu().numpy())
        rows.append(r)
    assert cache.len.tolist() == [n + steps] * 2
    e = tr.rel_err(np.concatenate(got), ref[np.concatenate(rows)])
    print(f"positions up to {n + steps} on a table grown from 130 rows: max|dev - ref64| / max|ref64| = {e:.3e}")
    assert e <= tr.FEATURE_BAR


# ---------------------------------------------------------------------------------------------------- 2. greedy generation
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


@pytest.mark.parametrize("head", dr.GEN_HEADS)
@pytest.mark.parametrize("seed", dr.GEN_SEEDS)
def test_greedy_generation_equals_the_reference_chain(dev, seed, head):
    from gnnlm_amd.generate import Generator
    lm = gen_lm(seed, head, dev)
    prompts = dr.gen_prompts(seed)
    tokens, logp, lengths = Generator(lm).generate(prompts, dr.GEN_NEW)
    tokens, logp, lengths = tokens.cpu().numpy(), logp.cpu().numpy(), lengths.cpu().numpy()
    for i in range(len(prompts)):
        want, want_lp, gaps, _ = dr.gen_chain(seed, i, head)
        n = int(lengths[i])
        assert n == len(want) and tokens[i, :n].tolist() == want, (i, tokens[i].tolist(), want)
        assert (tokens[i, n:] == dr.PAD).all() and (logp[i, n:] == 0).all()
        e = float(np.abs(logp[i, :n] - want_lp).max())
        print(f"seed {seed} {head} prompt {i}: {n} tokens, max |d logp| = {e:.3e} (minimum gap {gaps.min():.3e})")
        assert e <= LOGP_BAR


# ---------------------------------------------------------------------------------------------------- 3. sampling
def test_sampling_is_reproducible_and_stays_in_the_top_k(dev):
    from gnnlm_amd.generate import Generator
    lm = gen_lm(301, "dense", dev)
    g = Generator(lm)
    prompts, K, T = dr.gen_prompts(301), 5, 0.7
    runs = [g.generate(prompts, 24, sampling=True, sampling_topk=K, temperature=T, unk_penalty=0.5, seed=s) for s in (11, 11, 12)]
    a, b, c = [[x.cpu().numpy() for x in r] for r in runs]
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], c[0])                       # another seed, another text
    assert not np.array_equal(a[0], Generator(lm).generate(prompts, 24)[0].cpu().numpy())       # and not the greedy one
    # every pick lies in the top-k of the distribution it was drawn from, and carries that distribution's log-prob: replay the text
    tokens, logp, lengths = a
    off = np.concatenate([[0], np.cumsum([len(p) for p in prompts])])
    cache = lm.new_cache(len(prompts), max(len(p) for p in prompts) + 24)
    x, extra = lm.prefill(t(np.concatenate(prompts).astype(np.int64), dev), off, cache)
    x = x[t(off[1:] - 1, dev)]
    for s in range(24):
        lp = g.next_log_probs(x, {"inner_states": [None]}, T, 0.5)
        top = torch.topk(lp, K, dim=1)
        for i in range(len(prompts)):
            if s < lengths[i]:
                j = (top.indices[i] == int(tokens[i, s])).nonzero()
                assert j.numel() == 1, (i, s)
                assert float(top.values[i, j.item()]) == float(logp[i, s])
        x, extra = lm.step(t(tokens[:, s].copy(), dev), cache)
    with pytest.raises(ValueError, match="--sampling-topk"):
        g.generate(prompts, 4, sampling=True)
    with pytest.raises(ValueError, match="--sampling-topk"):
        g.generate(prompts, 4, sampling=True, sampling_topk=2049)


def test_temperature_divides_the_decoder_output(dev):
    """sequence_generator.py:572-573 divides decoder_out[0]: the features under the adaptive softmax, the LOGITS -- rows and bias -- under
    the plain output layer.  The unk penalty and the pad rule come after."""
    from gnnlm_amd.dense_softmax import DenseSoftmax
    from gnnlm_amd.generate import Generator
    T, pen = 0.5, 0.75
    rs = np.random.RandomState(4)
    x = rs.randn(5, dr.GEN_MODEL["d"]).astype(np.float32).astype(np.float64)
    for head in dr.GEN_HEADS:
        lm = gen_lm(301, head, dev)
        m, hw = dr.gen_model(301, head)
        if hw is None:
            bias = rs.randn(dr.GEN_MODEL["V"])
            lm.head = DenseSoftmax(lm.head.weight, t(bias.astype(np.float32), dev))
            z = (x @ np.asarray(m["E"], np.float64).T + bias.astype(np.float32)) / T
            want = z - z.max(-1, keepdims=True) - np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True))
        else:
            want = np.stack([dr.adaptive_dense_logp(r / T, **hw) for r in x])
        want[:, dr.UNK] -= pen
        want[:, dr.PAD] = -np.inf
        got = Generator(lm).next_log_probs(t(x.astype(np.float32), dev), {}, T, pen).cpu().numpy()
        ok = np.isfinite(want)
        assert np.array_equal(ok, np.isfinite(got))
        e = float(np.abs(got[ok] - want[ok]).max())
        print(f"{head}: log_softmax(decoder_out / {T}) max |dev - ref64| = {e:.3e}")
        assert e <= LOGP_BAR


# ---------------------------------------------------------------------------------------------------- 4. a captured step
def test_captured_step_replays_the_eager_loop(dev):
    from gnnlm_amd import ops
    lm = gen_lm(302, "dense", dev)
    prompts = dr.gen_prompts(302)
    B, N = len(prompts), 8
    off = np.concatenate([[0], np.cumsum([len(p) for p in prompts])])
    toks = t(np.concatenate(prompts).astype(np.int64), dev)
    bound = max(len(p) for p in prompts) + N + 2

    def one(cache, tok, state):
        """step + head + pick, everything into preallocated tensors"""
        x, _ = lm.step(tok, cache, want_inner=False, want_ffn_input=False, max_len=bound)
        lp = lm.head.log_probs(x)
        lp[:, dr.PAD] = float("-inf")
        ops.topk_merge(lp, state["val"], state["id"], init=True)
        ops.sample_topk(state["val"], state["id"], pad=dr.PAD, eos=dr.EOS, done=cache.done, out=state["next"], out_logp=state["lp"])
        tok.copy_(state["next"])

    def start():
        cache = lm.new_cache(B, bound)
        lm.prefill(toks, off, cache)
        state = {"val": torch.empty(B, 1, device=dev), "id": torch.empty(B, 1, dtype=torch.int64, device=dev),
                 "next": torch.empty(B, dtype=torch.int64, device=dev), "lp": torch.zeros(B, device=dev)}
        tok = t(np.asarray([p[-1] for p in prompts], np.int64), dev)
        one(cache, tok, state)                                   # the warm-up step: workspaces of this stream, code objects
        return cache, tok, state

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cache, tok, state = start()
        eager = []
        for _ in range(N):
            one(cache, tok, state)
            eager.append((tok.clone(), state["lp"].clone()))
        eager_len = cache.len.clone()
        cache2, tok2, state2 = start()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one(cache2, tok2, state2)
        replayed = []                                            # (the capture itself ran nothing)
        for _ in range(N):
            graph.replay()
            replayed.append((tok2.clone(), state2["lp"].clone()))
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    for (a, alp), (b, blp) in zip(eager, replayed):
        assert torch.equal(a, b) and torch.equal(alp.view(torch.int32), blp.view(torch.int32))
    assert torch.equal(cache2.len, eager_len) and int(cache2.n_bad.item()) == 0
    # and it is the reference chain: the warm-up step fed the prompt's last token again, so compare with that text
    m, _ = dr.gen_model(302, "dense")
    for i, p in enumerate(prompts):
        want, _, gaps, _ = dr.greedy_chain(m, p + [p[-1]], N + 1)
        assert gaps.min() >= 1e-3
        got = [int(a[i]) for a, _ in eager]
        assert got[:len(want) - 1] == want[1:len(got) + 1], (i, got, want)


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_before_any_launch(dev):
    from gnnlm_amd._lib import GnnlmError
    c = tr.GPU_CASES[2]                                          # learned positions
    m = tr.make_model(pos_rows=tr.PAD + 1 + 10, **c)
    lm = base.build(m, dev)
    toks = t(np.arange(4, 14).astype(np.int64), dev)
    cache = lm.new_cache(1, 16)
    lm.prefill(toks, [0, 10], cache)
    nxt = t(np.asarray([5], np.int64), dev)
    with pytest.raises(GnnlmError, match="position table"):
        lm.step(nxt, cache)                                      # position 10 needs row pad + 1 + 10 of a table of pad + 1 + 10 rows
    assert cache.len.tolist() == [10] and cache.steps == 10 and int(cache.n_bad.item()) == 0
    with pytest.raises(GnnlmError, match="position table"):
        lm.prefill(t(np.arange(4, 15).astype(np.int64), dev), [0, 11], lm.new_cache(1, 16))
    # the cache is full
    m2 = tr.make_model(pos_rows=64, **c)
    lm2 = base.build(m2, dev)
    cache = lm2.new_cache(1, 10)
    lm2.prefill(toks, [0, 10], cache)
    with pytest.raises(GnnlmError, match="full"):
        lm2.step(nxt, cache)
    with pytest.raises(GnnlmError, match="max_len"):
        lm2.step(nxt, cache, max_len=11)                         # the C entry's own refusal
    assert cache.len.tolist() == [10]
    with pytest.raises(GnnlmError, match="longer than the cache"):
        lm2.prefill(toks, [0, 10], lm2.new_cache(1, 9))
    with pytest.raises(GnnlmError, match="n_blocks"):
        lm2.prefill(toks, [0, 4, 10], lm2.new_cache(1, 16))
    with pytest.raises(TypeError):
        lm2.step(nxt.int(), lm2.new_cache(1, 4))
    lm2.check_tokens()


# ---------------------------------------------------------------------------------------------------- 6. the kNN mix
N_KEYS, KNN_T, LMBDA = 200, 1.0, 0.25


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
    knn = KNNModel(os.path.join(store, "faiss_store.ip"), store, k=N_KEYS, no_load_keys=True, metric_type="do_not_recomp_ip",
                   index=ExactIndex(torch.from_numpy(keys), "ip", False, dev), device=dev)
    return knn, keys, vals


def test_knn_mix(dev, tmp_path):
    from gnnlm_amd.generate import Generator
    seed = 301
    lm = gen_lm(seed, "dense", dev)
    m, _ = dr.gen_model(seed, "dense")
    knn, keys, vals = knn_fixture(seed, dev, tmp_path)
    prompts = dr.gen_prompts(seed)
    plain = [x.cpu().numpy() for x in Generator(lm).generate(prompts, 12)]
    zero = [x.cpu().numpy() for x in Generator(lm, knn, lmbda=0.0, knn_temperature=KNN_T).generate(prompts, 12)]
    for a, b in zip(plain, zero):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))                # lmbda = 0 searches nothing and changes nothing
    # lmbda = 0.25: the distribution the first pick is made from, against the float64 mix of the reference distributions
    g = Generator(lm, knn, lmbda=LMBDA, knn_temperature=KNN_T)
    off = np.concatenate([[0], np.cumsum([len(p) for p in prompts])])
    cache = lm.new_cache(len(prompts), 40)
    x, extra = lm.prefill(t(np.concatenate(prompts).astype(np.int64), dev), off, cache)
    last = t(off[1:] - 1, dev)
    got = g.next_log_probs(x[last], {"inner_states": [extra["inner_states"][-1][last]]}).cpu().numpy()
    V = dr.GEN_MODEL["V"]
    for i, p in enumerate(prompts):
        row = dr.incremental_rows(m, p)
        lm_lp = dr.dense_logp(m, row["out"][-1])
        sims = keys.astype(np.float64) @ row["last_inner"][-1] / KNN_T
        w = np.exp(sims - sims.max())
        p_knn = np.bincount(vals, weights=w / w.sum(), minlength=V)
        with np.errstate(divide="ignore"):
            want = np.logaddexp(np.log(1 - LMBDA) + lm_lp, np.log(LMBDA) + np.log(p_knn))
        want[dr.PAD] = -np.inf
        ok = np.isfinite(want)
        assert np.array_equal(ok, np.isfinite(got[i]))
        e = float(np.abs(got[i][ok] - want[ok]).max())
        print(f"prompt {i}: kNN-mixed log-probs max |dev - ref64| = {e:.3e}; the mix moves them by {np.abs(want[ok] - lm_lp[ok]).max():.3e}")
        assert e <= LOGP_BAR
        assert np.abs(want[ok] - lm_lp[ok]).max() > 1e-2
    tokens, logp, lengths = g.generate(prompts, 12)
    assert tokens.shape == (len(prompts), 12) and bool((lengths >= 1).all()) and bool(torch.isfinite(logp).all())


# ---------------------------------------------------------------------------------------------------- 7. the command line
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    root = tmp_path_factory.mktemp("generate")
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
    from gnnlm_amd.generate import get_parser, main
    args = get_parser().parse_args([str(cli["root"]), "--path", str(cli["ckpt"])] + extra)
    if knn is not None:
        args.knn_model = knn
    buf = io.StringIO()
    return main(args, file=buf), buf.getvalue().splitlines()


def test_command_line(dev, cli, tmp_path):
    out = tmp_path / "gen.npz"
    res, lines = drive(cli, ["--n-prompts", "3", "--prompt-len", "8", "--max-len-b", "10", "--out", str(out)])
    assert [l.split("\t")[0] for l in lines] == ["S-0", "H-0", "S-1", "H-1", "S-2", "H-2"]
    for i in range(3):
        assert lines[2 * i].split("\t")[1].split() == [str(int(v)) for v in cli["tokens"][8 * i:8 * i + 8]]       # no dict.txt: ids
        _, score, text = lines[2 * i + 1].split("\t")
        n = int(res["lengths"][i])
        assert text.split() == [str(int(v)) for v in res["tokens"][i, :n]]
        assert abs(float(score) - float(res["logp"][i, :n].astype(np.float64).sum())) <= 1e-9
    z = np.load(out)
    assert np.array_equal(z["tokens"], res["tokens"]) and np.array_equal(z["logp"], res["logp"]) and np.array_equal(z["lengths"], res["lengths"])
    assert z["prompts"].shape == (3, 9) and (z["prompts"][:, 0] == tr.EOS).all()
    # the continuation is the reference's: eos, the prompt, then greedy under the float64 restatement
    m, _ = dr.gen_model(301, "dense")
    want = dr.greedy_chain(m, [tr.EOS] + [int(v) for v in cli["tokens"][:8]], 10)
    assert want[2].min() >= 1e-3 and res["tokens"][0, :len(want[0])].tolist() == want[0]
    # words when DATA/dict.txt exists
    with open(cli["root"] / "dict.txt", "w") as f:
        f.write("".join(f"w{i} 1\n" for i in range(4, dr.GEN_MODEL["V"])))
    try:
        _, lines = drive(cli, ["--prompt-ids", "5,17,9", "--max-len-b", "4"])
    finally:
        os.remove(cli["root"] / "dict.txt")
    assert lines[0] == "S-0\tw5 w17 w9" and len(lines) == 2
    assert all(w.startswith("w") or w in ("<s>", "</s>", "<unk>") for w in lines[1].split("\t")[2].split())
    # sampling, --fp16, and kNN through the same driver
    res_s, lines = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "6", "--sampling", "--sampling-topk", "10",
                               "--temperature", "0.8", "--seed", "3", "--fp16"])
    assert len(lines) == 4 and res_s["tokens"].shape == (2, 6)
    knn, _, _ = knn_fixture(301, dev, tmp_path)
    res_k, lines = drive(cli, ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "6", "--knnlm", "--k", str(N_KEYS), "--lmbda", "0.25",
                               "--knn-temperature", "1"], knn=knn)
    assert len(lines) == 4 and np.isfinite(res_k["logp"]).all()


@pytest.mark.parametrize("flags,exc,word", [
    (["--beam", "2"], ValueError, "--beam"),
    (["--sampling", "--sampling-topk", "5", "--sampling-topp", "0.9"], ValueError, "--sampling-topp"),
    (["--sampling"], ValueError, "--sampling-topk"),
    (["--sampling", "--sampling-topk", "2049"], ValueError, "--sampling-topk"),
    (["--no-repeat-ngram-size", "3"], ValueError, "--no-repeat-ngram-size"),
    (["--min-len", "2"], ValueError, "--min-len"),
    (["--graph"], ValueError, "--graph"),
    (["--sweep-lmbda", "0.1,0.2"], ValueError, "--sweep-lmbda"),
    (["--sweep-temperature", "1,2"], ValueError, "--sweep-temperature"),
    (["--sweep-k", "8,16"], ValueError, "--sweep-k"),
    (["--knnlm"], ValueError, "--knnlm"),
    (["--knnlm", "--lmbda", "0", "--dstore-dir", "D", "--index-file", "F"], ValueError, "--lmbda"),
])
def test_command_line_refusals(dev, cli, flags, exc, word):
    with pytest.raises(exc, match=word):
        drive(cli, ["--max-len-b", "4"] + flags)


def test_more_than_one_process_and_other_head_widths_are_refused(dev, cli, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one process"):
        drive(cli, ["--max-len-b", "4"])
    monkeypatch.delenv("WORLD_SIZE")
    from gnnlm_amd.transformer_lm import TransformerLM
    m, _ = dr.gen_model(301, "dense")
    c = dict(dr.GEN_MODEL, act="relu", emb_norm=False, H=8)      # d_k = 8
    with pytest.raises(ValueError, match="16, 32, 64, 128"):
        TransformerLM.from_state_dict(base.state_dict_of(m, "qkv"), base.args_of(m, c), dev)
    assert "--knn-temperature" in __import__("gnnlm_amd.generate", fromlist=["get_parser"]).get_parser().format_help()
