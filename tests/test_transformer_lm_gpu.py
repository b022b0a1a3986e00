"""The base transformer LM on the device: the embed kernel bit for bit, the orchestrator against the float64 restatement
(tests/transformer_lm_ref.py), causality, the checkpoint loader, the refusals of the C entry point, and the driver end to end
(perplexity, --context-window, the datastore writer).  GPU only.

Bars: features max|dev - ref64| / max|ref64| <= 5e-5 (README "Parity"; tests/test_transformer_lm_ref_cpu.py shows float32 itself
within a quarter of it on these cases); per-token log-probs 2e-5 and perplexity 0.02 (the project's existing bars); precision 3
as derived in test_transformer_lm_ref_cpu.py::test_float16_operand_rounding_is_reproducible_in_float32, and against the reference's
own model.half() run with the rule of tests/test_fp16_gpu.py (never further from float64 than the reference's half run, RMS).

Measured on an MI355X: features 2.5e-7 / 2.9e-7 / 4.2e-7 on cases 1 / 2 / 3; precision 3 at 0.16 / 0.16 / 0.09 of the
rounding's effect (bar 0.5), rms 6.4e-4 against float64 where the reference's half run has 1.4e-3; driver log-probs 1.4e-6, perplexity
equal to four decimals in the three configurations.
"""
import ctypes
import struct
from argparse import Namespace

import numpy as np
import pytest
import torch

import transformer_lm_ref as tr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def build(m, dev, precision=None):
    """A TransformerLM from a restatement model dict (q | k | v concatenated, unscaled: the fold happens in the mirror)."""
    from gnnlm_amd.token_embed import TokenEmbedding
    from gnnlm_amd.transformer_lm import TransformerLM
    layers = []
    for w in m["layers"]:
        lw = {k: torch.from_numpy(w[k]) for k in ("ln1_g", "ln1_b", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")}
        lw["wqkv"] = torch.from_numpy(np.concatenate([w["wq"], w["wk"], w["wv"]], 0))
        lw["bqkv"] = torch.from_numpy(np.concatenate([w["bq"], w["bk"], w["bv"]], 0))
        layers.append(lw)
    pair = lambda p: None if p is None else (torch.from_numpy(p[0]), torch.from_numpy(p[1]))
    E = TokenEmbedding(t(np.asarray(m["E"], np.float32), dev), "plain")
    return TransformerLM(E, layers, m["H"], act=m["act"], scale=m["scale"], pos=None if m["P"] is None else torch.from_numpy(m["P"]),
                         learned_pos=True, ln_emb=pair(m["ln_emb"]), ln_out=pair(m["ln_out"]), device=dev, precision=precision)


def run(model, tokens, off, dev):
    x, extra = model.extract_features(t(tokens, dev), off)
    torch.cuda.synchronize()
    return {"out": x.cpu().numpy(), "last_inner": extra["inner_states"][-1].cpu().numpy(), "last_ffn_input": extra["last_ffn_input"].cpu().numpy()}


# ---------------------------------------------------------------------------------------------------- 1. the embed kernel
@pytest.mark.parametrize("d", [8, 36])
@pytest.mark.parametrize("positions", ["sinusoidal", "learned", "none"])
def test_embed_bit_for_bit(dev, d, positions):
    from gnnlm_amd import ops
    from gnnlm_amd._lib import GnnlmError
    V, lens, pad = 11, [1, 5, 33], tr.PAD
    off = np.concatenate([[0], np.cumsum(lens)])
    rs = np.random.RandomState(7 + d)
    E = rs.randn(V, d).astype(np.float32)
    rows = pad + 1 + max(lens)                                   # a block exactly as long as the table holds
    P = {"sinusoidal": tr.sinusoidal_table(rows, d), "learned": rs.randn(rows, d).astype(np.float32), "none": None}[positions]
    tokens = rs.randint(0, V, size=int(off[-1])).astype(np.int64)
    tokens[[0, 1, 2, 3, 7, 38]] = [0, V - 1, -1, V, V - 1, -1]  # both ends of the vocabulary, and three ids outside it
    scale = float(np.sqrt(d))
    want, n_bad = tr.embed_f32(E, tokens, off, P, pad, scale)
    assert n_bad == 3
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.lm_embed(t(tokens, dev), t(E, dev), off, P=None if P is None else t(P, dev), pad_idx=pad, scale=scale, n_bad=bad)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert int(bad.item()) == 3
    assert (got.cpu().numpy()[[2, 3, 38]] == 0).all()
    if P is not None:
        # the fused multiply-add of the two steps would differ somewhere: the test has teeth
        valid = (tokens >= 0) & (tokens < V)
        pos = np.concatenate([pad + 1 + np.arange(n) for n in lens])
        fma = (np.float64(np.float32(scale)) * E[np.clip(tokens, 0, V - 1)].astype(np.float64) + P[pos]).astype(np.float32)
        assert not np.array_equal(fma[valid], want[valid])
        # one row short: refused before anything is launched
        out = torch.full((int(off[-1]), d), SENTINEL, device=dev)
        with pytest.raises(GnnlmError, match="position table"):
            ops.lm_embed(t(tokens, dev), t(E, dev), off, P=t(P[:-1], dev), pad_idx=pad, scale=scale, out=out, n_bad=bad)
        torch.cuda.synchronize()
        assert (out == SENTINEL).all() and int(bad.item()) == 3


def test_relu_in_place(dev):
    from gnnlm_amd import ops
    for n in (1, 7, 1024, 4099):
        x = torch.randn(n, device=dev)
        x[0] = float("nan")
        want = torch.relu(x)
        got = ops.relu_(x.clone())
        assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0))


# ---------------------------------------------------------------------------------------------------- 2. the orchestrator
@pytest.mark.parametrize("case", sorted(tr.GPU_CASES))
def test_orchestrator_against_restatement(dev, case):
    m, tokens, off = tr.gpu_case(case)
    ref = tr.gpu_case_ref(case)
    got = run(build(m, dev), tokens, off, dev)
    for key in ("out", "last_inner", "last_ffn_input"):
        e = tr.rel_err(got[key], ref[key])
        print(f"case {case} {key}: max|dev - ref64| / max|ref64| = {e:.3e}")
        assert e <= tr.FEATURE_BAR


def test_orchestrator_precision_3(dev, golden):
    m, tokens, off = tr.gpu_case(1)
    ref16, ref64 = tr.gpu_case_ref(1, half_gemm=True), tr.gpu_case_ref(1)
    f32 = run(build(m, dev), tokens, off, dev)
    f16 = run(build(m, dev, precision="fp16"), tokens, off, dev)
    assert not np.array_equal(f16["out"], f32["out"])                         # the mode is really taken
    for key in ("out", "last_inner", "last_ffn_input"):
        share = tr.rms(f16[key] - ref16[key]) / tr.rms(ref64[key] - ref16[key])
        print(f"case 1 precision 3 {key}: rms(dev - rounded ref64) / rms(effect of the rounding) = {share:.3f}")
        assert share <= tr.FP16_SHARE
    # against the reference's own model.half() run, as tests/test_fp16_gpu.py: never further from float64 than it is (RMS, no margin)
    g = golden("transformer_lm")
    name = "relu_sin_adaptive"
    gm = tr.golden_model(g, name, 4, "relu", 8.0)
    gm["P"] = tr.sinusoidal_table(64, 64)
    toks = g[f"{name}.tokens"]
    bsz, T = toks.shape
    goff = np.arange(bsz + 1) * T
    r64 = tr.forward(gm, toks.reshape(-1), goff)
    gm32 = dict(gm, E=np.asarray(gm["E"], np.float32))
    d32, d16 = run(build(gm32, dev), toks.reshape(-1), goff, dev), run(build(gm32, dev, precision="fp16"), toks.reshape(-1), goff, dev)
    for key, gk in (("out", "x_half"), ("last_inner", "last_inner_half")):
        ref_half = g[f"{name}.{gk}"].reshape(bsz * T, -1).astype(np.float64)
        e_ours, e_ref, e_f32 = tr.rms(d16[key] - r64[key]), tr.rms(ref_half - r64[key]), tr.rel_err(d32[key], r64[key])
        print(f"{name} {key}: rms(ours fp16 - f64) = {e_ours:.3e}, rms(reference half - f64) = {e_ref:.3e}, ours f32 rel {e_f32:.3e}")
        assert e_f32 <= tr.FEATURE_BAR
        assert e_ours <= e_ref


def test_causality(dev):
    """Tokens after position p of one block changed: every row at or before p, and every other block, is bit-identical."""
    m, tokens, off = tr.gpu_case(1)
    model = build(m, dev)
    a = run(model, tokens, off, dev)
    blk, p = 4, 40                                                # the 70-token block, inside its second query tile
    changed = tokens.copy()
    s, e = int(off[blk]), int(off[blk + 1])
    changed[s + p + 1:e] = (changed[s + p + 1:e] + 7) % tr.GPU_CASES[1]["V"]
    b = run(model, changed, off, dev)
    same = np.ones(int(off[-1]), bool)
    same[s + p + 1:e] = False
    for key in a:
        assert np.array_equal(a[key][same].view(np.uint32), b[key][same].view(np.uint32)), key
        assert not np.array_equal(a[key][~same], b[key][~same])


# ---------------------------------------------------------------------------------------------------- 3. the loader
def state_dict_of(m, layout, bands=None, class_proj=None):
    """A reference-style state dict of a restatement model: ``layout`` "in_proj" (fused) or "qkv" (split projections)."""
    sd = {}
    T = torch.from_numpy
    if bands is None:
        sd["decoder.embed_tokens.weight"] = T(np.asarray(m["E"], np.float32))
        sd["decoder.embed_out"] = T(np.asarray(m["E"], np.float32))
    else:
        for i, (e, p) in enumerate(bands):
            sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"], sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = T(e), T(p)
        sd["decoder.adaptive_softmax.head.class_proj.weight"] = T(class_proj)
    for i, w in enumerate(m["layers"]):
        p = f"decoder.layers.{i}."
        if layout == "in_proj":
            sd[p + "self_attn.in_proj_weight"] = T(np.concatenate([w["wq"], w["wk"], w["wv"]], 0))
            sd[p + "self_attn.in_proj_bias"] = T(np.concatenate([w["bq"], w["bk"], w["bv"]], 0))
        else:
            for n in "qkv":
                sd[p + f"self_attn.{n}_proj.weight"], sd[p + f"self_attn.{n}_proj.bias"] = T(w["w" + n]), T(w["b" + n])
        sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"] = T(w["wo"]), T(w["bo"])
        sd[p + "self_attn_layer_norm.weight"], sd[p + "self_attn_layer_norm.bias"] = T(w["ln1_g"]), T(w["ln1_b"])
        sd[p + "final_layer_norm.weight"], sd[p + "final_layer_norm.bias"] = T(w["ln2_g"]), T(w["ln2_b"])
        for n in ("fc1", "fc2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = T(w["w" + n[-1]]), T(w["b" + n[-1]])
    if m["ln_out"] is not None:
        sd["decoder.layer_norm.weight"], sd["decoder.layer_norm.bias"] = T(m["ln_out"][0]), T(m["ln_out"][1])
    if m["ln_emb"] is not None:
        sd["decoder.layernorm_embedding.weight"], sd["decoder.layernorm_embedding.bias"] = T(m["ln_emb"][0]), T(m["ln_emb"][1])
    return sd


def args_of(m, c, **over):
    a = dict(decoder_embed_dim=c["d"], decoder_attention_heads=c["H"], decoder_layers=c["L"], decoder_ffn_embed_dim=c["ffn"],
             activation_fn=c["act"], decoder_learned_pos=False, no_token_positional_embeddings=False, max_target_positions=128,
             no_decoder_final_norm=not c["final_norm"], layernorm_embedding=c["emb_norm"], adaptive_softmax_cutoff=None,
             share_decoder_input_output_embed=False, decoder_input_dim=c["d"], decoder_output_dim=c["d"])
    a.update(over)
    return Namespace(**a)


def test_loader_layouts_and_refusals(dev):
    from gnnlm_amd.transformer_lm import TransformerLM
    m, tokens, off = tr.gpu_case(1)
    c = tr.GPU_CASES[1]
    outs = []
    for layout in ("in_proj", "qkv"):
        model = TransformerLM.from_state_dict(state_dict_of(m, layout), args_of(m, c), dev)
        outs.append(run(model, tokens, off, dev))
    for key in outs[0]:
        assert np.array_equal(outs[0][key].view(np.uint32), outs[1][key].view(np.uint32)), key
    assert tr.rel_err(outs[0]["out"], tr.gpu_case_ref(1)["out"]) <= tr.FEATURE_BAR        # (the loader builds the sinusoidal table itself)
    sd = state_dict_of(m, "qkv")
    for over, word in ((dict(decoder_input_dim=32), "decoder_input_dim"), (dict(decoder_output_dim=32), "decoder_output_dim"),
                       (dict(character_embeddings=True), "character_embeddings"), (dict(activation_fn="tanh"), "activation_fn")):
        with pytest.raises(ValueError, match=word):
            TransformerLM.from_state_dict(sd, args_of(m, c, **over), dev)
    # a token id outside the vocabulary is counted on the device and raised with the results
    model = TransformerLM.from_state_dict(sd, args_of(m, c), dev)
    bad = tokens.copy()
    bad[5] = c["V"]
    with pytest.raises(ValueError, match="outside the vocabulary"):
        model.extract_features(t(bad, dev), off)


# ---------------------------------------------------------------------------------------------------- 4. refusals of the C entry point
def test_c_entry_refusals_leave_outputs_untouched(dev):
    from gnnlm_amd import _lib
    from gnnlm_amd.ragged import as_ragged
    m, tokens, off = tr.gpu_case(1)
    model = build(m, dev)
    rg = as_ragged(off, dev)
    n, d = rg.n_tok, model.d
    tok = t(tokens, dev)
    outs = [torch.full((n, d), SENTINEL, device=dev) for _ in range(3)]
    L = _lib.lib()

    def call(mutate=None, ws_short=0):
        desc = model._desc(model._positions(int(rg.lengths.max())))
        io = _lib.gnnlm_tlm_io_t()
        io.tokens, io.blocks, io.max_len = tok.data_ptr(), rg.desc(), int(rg.lengths.max())
        io.out, io.last_inner, io.last_ffn_input = (o.data_ptr() for o in outs)
        need = L.gnnlm_transformer_lm_workspace_bytes(ctypes.byref(desc), ctypes.byref(io))
        if mutate:
            mutate(desc, io)
        ws = torch.empty(need, device=dev, dtype=torch.uint8)
        return L.gnnlm_transformer_lm_forward(ctypes.byref(desc), ctypes.byref(io), ctypes.c_void_p(ws.data_ptr()), need - ws_short, _lib.stream())

    def set_(**kw):
        def f(desc, io):
            for k, v in kw.items():
                setattr(desc if hasattr(desc, k) else io, k, v)
        return f

    bad = [("d_k = 8", set_(H=8), 0), ("d % 4", set_(d=62), 0), ("ffn % 4", set_(ffn=94), 0), ("H * d_k != d", set_(H=3), 0),
           ("act", set_(act=2), 0), ("precision", set_(precision=4), 0), ("NULL tokens", set_(tokens=None), 0),
           ("NULL layers", set_(layers=None), 0), ("half a LayerNorm", set_(ln_out_g=outs[0].data_ptr()), 0),
           ("a block longer than the table", set_(max_len=10 ** 6), 0), ("short workspace", None, 1)]
    for what, mutate, short in bad:
        assert call(mutate, short) == -22, what
        assert L.gnnlm_last_error()
    torch.cuda.synchronize()
    for o in outs:
        assert (o == SENTINEL).all()
    assert call() == 0                                            # the unmodified call is accepted
    torch.cuda.synchronize()
    assert tr.rel_err(outs[0].cpu().numpy(), tr.gpu_case_ref(1)["out"]) <= tr.FEATURE_BAR


# ---------------------------------------------------------------------------------------------------- 5. the driver, end to end
SIZES = [5, 9, 3, 20, 7, 12, 2, 17, 4, 11]                       # sentence lengths; the 20 and the 17 are longer than a block of 16
V, CUT, D = 48, [16, 32], 32


def write_split(data, split, tokens, sizes):
    with open(data / f"{split}.idx", "wb") as f:
        f.write(b"MMIDIDX\x00\x00" + struct.pack("<Q", 1) + struct.pack("<B", 4) + struct.pack("<Q", len(sizes)))
        f.write(np.asarray(sizes, np.int32).tobytes())
        f.write((np.concatenate([[0], np.cumsum(sizes)[:-1]]) * 4).astype(np.int64).tobytes())
    np.asarray(tokens, np.int32).tofile(data / f"{split}.bin")


@pytest.fixture(scope="module")
def fixture_dir(tmp_path_factory):
    """DATA/test.bin/.idx and a checkpoint: adaptive input (V = 48, cutoffs 16,32, d = 32, H = 2, 2 layers) + its tied adaptive softmax."""
    root = tmp_path_factory.mktemp("base_lm")
    rs = np.random.RandomState(5)
    tokens = rs.randint(4, V, size=sum(SIZES)).astype(np.int64)
    tokens[np.cumsum(SIZES) - 1] = tr.EOS                         # sentences end in eos, as binarised text does
    write_split(root, "test", tokens, SIZES)
    c = dict(seed=77, V=V, d=D, H=2, L=2, ffn=64, act="relu", final_norm=True, emb_norm=False, positions="sinusoidal")
    m = tr.make_model(pos_rows=128, **c)
    bands, lo = [], 0
    for i, hi in enumerate(CUT + [V]):
        dim = D // 2 ** i
        bands.append(((rs.randn(hi - lo, dim) * dim ** -0.5).astype(np.float32), (rs.randn(D, dim) * D ** -0.5).astype(np.float32)))
        lo = hi
    class_proj = (rs.randn(2, D) * D ** -0.5).astype(np.float32)
    m["E"] = tr.adaptive_table(bands)
    args = args_of(m, c, adaptive_softmax_cutoff="16,32", adaptive_input=True, adaptive_input_cutoff="16,32", adaptive_input_factor=2,
                   tie_adaptive_weights=True)
    ckpt = root / "base.pt"
    torch.save({"args": args, "model": state_dict_of(m, "qkv", bands, class_proj)}, ckpt)
    head = dict(cutoff=CUT + [V], emb=[b[0] for b in bands], proj=[b[1] for b in bands], class_proj=class_proj)
    return {"root": root, "ckpt": ckpt, "tokens": tokens, "model": m, "head": head, "ref": {}}


CONFIGS = {
    "none+ctx": (["--sample-break-mode", "none", "--tokens-per-sample", "16", "--context-window", "8", "--max-tokens", "40"], "none", 16, 8),
    "complete": (["--sample-break-mode", "complete", "--tokens-per-sample", "16", "--max-tokens", "40"], "complete", 16, 0),
    "none": (["--sample-break-mode", "none", "--tokens-per-sample", "16", "--max-tokens", "16"], "none", 16, 0),
}


def reference_run(fx, cfg, key="last_inner"):
    """The float64 restatement of a configuration (computed once and shared)."""
    if (cfg, key) not in fx["ref"]:
        from gnnlm_amd.token_blocks import slice_indices                      # (pinned against the reference by tests/test_break_modes_cpu.py)
        _, mode, tps, w = CONFIGS[cfg]
        samples = [(int(s), int(e)) for s, e in slice_indices(SIZES, mode, tps - w)]
        ctx = tr.context_windows([e - s for s, e in samples], tps - w, w) if w else [0] * len(samples)
        fx["ref"][(cfg, key)] = tr.score_split(fx["model"], fx["head"], fx["tokens"], samples, ctx, key) + (ctx,)
    return fx["ref"][(cfg, key)]


def drive(fx, extra):
    from gnnlm_amd.eval_lm import get_parser, main
    args = get_parser().parse_args([str(fx["root"]), "--path", str(fx["ckpt"]), "--gen-subset", "test"] + extra)
    args.keep_pos_scores = True
    return main(args)


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_driver_perplexity(dev, fixture_dir, cfg):
    logp, _, ctx = reference_run(fixture_dir, cfg)
    res = drive(fixture_dir, CONFIGS[cfg][0])
    assert res["count"] == len(fixture_dir["tokens"]) == len(logp)
    assert res["tokens"] == len(logp) + sum(ctx)                               # the context rows are computed, not scored
    assert (cfg == "none+ctx") == (sum(ctx) > 0)
    d = np.abs(res["pos_scores"] - logp).max()
    ppl = float(2 ** (-logp.sum() / len(logp) / np.log(2)))
    print(f"{cfg}: max |d logp| = {d:.3e}, ppl {res['ppl']:.4f} vs {ppl:.4f}")
    assert d <= 2e-5
    assert abs(res["ppl"] - ppl) <= 0.02


@pytest.mark.parametrize("keytype,fp16", [(None, False), ("last_ffn_input", False), (None, True)])
def test_driver_saves_the_datastore(dev, fixture_dir, tmp_path, keytype, fp16):
    import os
    from gnnlm_amd.data_store import DataStore
    extra = CONFIGS["none+ctx"][0] + ["--save-knnlm-dstore", "--dstore-mmap", str(tmp_path)]
    extra += (["--knn-keytype", keytype] if keytype else []) + (["--dstore-fp16"] if fp16 else [])
    drive(fixture_dir, extra)
    sub = tmp_path / ("test_dstore" + (f"-{keytype}" if keytype else ""))
    for f in ("keys.npy", "vals.npy", "info.json"):
        assert os.path.exists(sub / f), f
    ds = DataStore.from_pretrained(str(sub))
    n = len(fixture_dir["tokens"])
    assert ds.dstore_size == n and ds.hidden_size == D and ds.dstore_fp16 == fp16 and ds.vocab_size == V
    assert np.array_equal(np.asarray(ds.vals).reshape(-1), fixture_dir["tokens"])       # every token once, in corpus order
    _, keys, _ = reference_run(fixture_dir, "none+ctx", keytype or "last_inner")
    got = np.asarray(ds.keys)
    if fp16:
        assert got.dtype == np.float16
        want = keys.astype(np.float16)
        ulp = np.abs(np.nextafter(want, np.float16(np.inf)).astype(np.float64) - want.astype(np.float64))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all()
    else:
        assert got.dtype == np.float32
        assert tr.rel_err(got, keys) <= tr.FEATURE_BAR
    if keytype is None and not fp16:                               # the two key types are different tensors
        other = reference_run(fixture_dir, "none+ctx", "last_ffn_input")[1]
        assert tr.rel_err(got, other) > 1e-2


def test_driver_refusals(dev, fixture_dir):
    with pytest.raises(ValueError, match="--knnlm"):
        drive(fixture_dir, CONFIGS["none"][0] + ["--knnlm"])
    with pytest.raises(NotImplementedError, match="use-precompute-feat"):
        drive(fixture_dir, CONFIGS["none"][0] + ["--graph"])
    with pytest.raises(NotImplementedError, match="context-window"):
        drive(fixture_dir, CONFIGS["none+ctx"][0] + ["--graph", "--use-precompute-feat"])
    with pytest.raises(ValueError, match="graph-capture"):
        drive(fixture_dir, CONFIGS["none"][0] + ["--graph-capture"])
