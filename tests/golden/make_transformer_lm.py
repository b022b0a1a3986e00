#!/usr/bin/env python3
"""Golden vectors of the base transformer LM -> tests/golden/transformer_lm.npz.

Needs a source tree of the reference (the tests only read the stored vectors, never the reference):

    python tests/golden/make_transformer_lm.py <reference source tree>

What is executed from the reference tree (nothing of it is copied into this repo), in the manner of make_dense_head.py.  Loaded by
path under stub ``fairseq`` / ``fairseq.utils`` / ``fairseq.modules`` modules:
  * fairseq/incremental_decoding_utils.py              whole (it imports nothing of fairseq)
  * fairseq/modules/multihead_attention.py             whole: ``MultiheadAttention``
  * fairseq/modules/transformer_layer.py               whole: ``TransformerDecoderLayer``
  * fairseq/modules/sinusoidal_positional_embedding.py whole: ``SinusoidalPositionalEmbedding``
  * fairseq/modules/learned_positional_embedding.py    whole: ``LearnedPositionalEmbedding``
  * fairseq/modules/adaptive_input.py                  whole: ``AdaptiveInput``
  * fairseq/utils.py                                   its functions ``softmax``, ``make_positions``, ``fill_with_neg_inf``, by ``ast``
  * fairseq/models/transformer.py                      ``TransformerDecoder`` reduced with ``ast`` to ``extract_features`` (:708-841) and
                                                       ``buffered_future_mask`` (:860-872), bases and annotations dropped
  * fairseq/data/lm_context_window_dataset.py          ``LMContextWindowDataset`` reduced to ``__init__`` and ``collater``
What the stubs stand in for, and what therefore pins those pieces instead of the reference:
  * ``fairseq.modules.LayerNorm`` -> ``torch.nn.LayerNorm`` (the reference's own fallback without apex): pinned by ``F.layer_norm``;
  * ``utils.get_activation_fn`` -> ``F.relu`` / ``F.gelu`` on float32 (what the reference's functions of those names call);
  * ``MultiheadAttention.forward`` itself takes its ``F.multi_head_attention_forward`` branch in this torch (:138-165), so the
    attention arithmetic is pinned by that torch function, driven by the reference's own module and weights layout;
  * the wrapped ``MonolingualDataset`` of the context-window dataset is a stub whose ``collater`` right-pads the samples.

Output is data only: the seeded weights (tests/transformer_lm_ref.py::make_model, stored again so that the fixture stands alone), the
token inputs, and what the reference returned -- features, inner_states[-1], last_ffn_input, the adaptive-input rows, the position
rows, and the collater's context windows for two runs of sample lengths.
"""
import ast
import importlib.util
import math
import os
import sys
import types
from typing import Any, Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import transformer_lm_ref as tr  # noqa: E402

PAD = 1
CASES = {
    # name: make_model arguments + the batch
    "relu_sin_adaptive": dict(seed=211, V=48, d=64, H=4, L=2, ffn=96, act="relu", final_norm=False, emb_norm=False, positions="sinusoidal",
                              bsz=2, T=37, cutoff=[16, 32], factor=2, keytype=None),
    "gelu_learned_norms": dict(seed=212, V=40, d=64, H=2, L=1, ffn=128, act="gelu", final_norm=True, emb_norm=True, positions="learned",
                               bsz=3, T=21, cutoff=None, factor=None, keytype="last_ffn_input"),
}


def _strip(fn):
    for a in fn.args.args + fn.args.kwonlyargs:
        a.annotation = None
    fn.returns = None
    return fn


def _reduced_class(tree, name, methods):
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    cls.body = [_strip(n) for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in methods]
    assert len(cls.body) == len(methods), (name, [n.name for n in cls.body])
    cls.bases, cls.keywords, cls.decorator_list = [], [], []
    return cls


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    utree = ast.parse(open(os.path.join(ref, "fairseq/utils.py")).read())
    fns = [_strip(n) for n in utree.body if isinstance(n, ast.FunctionDef) and n.name in ("softmax", "make_positions", "fill_with_neg_inf")]
    assert len(fns) == 3
    uns = {"torch": torch, "F": F}
    mod = ast.Module(body=fns, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "ref:fairseq/utils.py", "exec"), uns)
    utils = types.ModuleType("fairseq.utils")
    utils.softmax, utils.make_positions, utils.fill_with_neg_inf = uns["softmax"], uns["make_positions"], uns["fill_with_neg_inf"]
    acts = {"relu": F.relu, "gelu": lambda x: F.gelu(x.float()).type_as(x)}
    utils.get_activation_fn = lambda activation: acts[activation]
    fairseq = types.ModuleType("fairseq")
    fairseq.utils = utils
    fairseq.__path__ = []
    modules = types.ModuleType("fairseq.modules")
    modules.LayerNorm = lambda dim, eps=1e-5, elementwise_affine=True, export=False: nn.LayerNorm(dim, eps, elementwise_affine)
    sys.modules.update({"fairseq": fairseq, "fairseq.utils": utils, "fairseq.modules": modules})
    fairseq.incremental_decoding_utils = _load(ref, "fairseq/incremental_decoding_utils.py", "fairseq.incremental_decoding_utils")
    modules.MultiheadAttention = _load(ref, "fairseq/modules/multihead_attention.py", "fairseq.modules.multihead_attention").MultiheadAttention
    layer = _load(ref, "fairseq/modules/transformer_layer.py", "fairseq.modules.transformer_layer").TransformerDecoderLayer
    sin = _load(ref, "fairseq/modules/sinusoidal_positional_embedding.py", "fairseq.modules.sinusoidal_positional_embedding").SinusoidalPositionalEmbedding
    learned = _load(ref, "fairseq/modules/learned_positional_embedding.py", "fairseq.modules.learned_positional_embedding").LearnedPositionalEmbedding
    adaptive = _load(ref, "fairseq/modules/adaptive_input.py", "fairseq.modules.adaptive_input").AdaptiveInput

    tree = ast.parse(open(os.path.join(ref, "fairseq/models/transformer.py")).read())
    dec = _reduced_class(tree, "TransformerDecoder", ("extract_features", "buffered_future_mask"))
    mod = ast.Module(body=[dec], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "F": F, "math": math, "utils": utils, "Optional": Optional, "Dict": Dict, "List": List, "Any": Any, "Tensor": Tensor,
          "EncoderOut": None}
    exec(compile(mod, "ref:fairseq/models/transformer.py", "exec"), ns)

    tree = ast.parse(open(os.path.join(ref, "fairseq/data/lm_context_window_dataset.py")).read())
    ctx = _reduced_class(tree, "LMContextWindowDataset", ("__init__", "collater"))
    mod = ast.Module(body=[ctx], type_ignores=[])
    ast.fix_missing_locations(mod)
    cns = {"np": np, "torch": torch, "MonolingualDataset": StubDataset}
    exec(compile(mod, "ref:fairseq/data/lm_context_window_dataset.py", "exec"), cns)
    return types.SimpleNamespace(Decoder=ns["TransformerDecoder"], Layer=layer, Sin=sin, Learned=learned, Adaptive=adaptive,
                                 CtxDataset=cns["LMContextWindowDataset"])


class StubDataset:
    """Stands in for MonolingualDataset: ``collater`` right-pads (source, target) pairs."""

    def collater(self, samples):
        n = max(len(s) for s, _ in samples)
        pad = lambda a: np.concatenate([a, np.full(n - len(a), PAD, dtype=np.int64)])
        return {"net_input": {"src_tokens": torch.from_numpy(np.stack([pad(s) for s, _ in samples])),
                              "src_lengths": torch.tensor([len(s) for s, _ in samples])},
                "target": torch.from_numpy(np.stack([pad(t) for _, t in samples]))}


def run_case(R, name, c, out):
    m = tr.make_model(c["seed"], c["V"], c["d"], c["H"], c["L"], c["ffn"], c["act"], c["final_norm"], c["emb_norm"], c["positions"], pos_rows=64)
    rs = np.random.RandomState(c["seed"] + 1000)
    tokens = rs.randint(2, c["V"], size=(c["bsz"], c["T"])).astype(np.int64)          # (no <pad>: the stream of a binarised corpus)
    tokens[0, :3] = [2, c["V"] - 1, 3]
    d = c["d"]
    args = types.SimpleNamespace(decoder_embed_dim=d, decoder_attention_heads=c["H"], attention_dropout=0.0, dropout=0.0, activation_fn=c["act"],
                                 activation_dropout=0.0, decoder_normalize_before=True, decoder_ffn_embed_dim=c["ffn"])
    dec = R.Decoder()
    dec.training, dec.dropout, dec.decoder_layerdrop = False, 0.0, 0.0
    dec.cross_self_attention, dec.layer_wise_attention = False, False
    dec.knn_keytype, dec.padding_idx, dec.embed_scale = c["keytype"], PAD, m["scale"]
    dec.project_in_dim = dec.project_out_dim = None
    dec._future_mask = torch.empty(0)
    t = lambda a: torch.from_numpy(np.asarray(a))
    # ---- embed_tokens: the reference's AdaptiveInput, or a plain embedding
    if c["cutoff"]:
        emb = R.Adaptive(c["V"], PAD, d, c["factor"], d, list(c["cutoff"]))
        brs = np.random.RandomState(c["seed"] + 2000)
        with torch.no_grad():
            for i, seq in enumerate(emb.embeddings):
                size, dim = seq[0].weight.shape
                seq[0].weight.copy_(t((brs.randn(size, dim) * dim ** -0.5).astype(np.float32)))
                seq[1].weight.copy_(t((brs.randn(d, dim) * d ** -0.5).astype(np.float32)))
                out[f"{name}.band{i}.emb"], out[f"{name}.band{i}.proj"] = seq[0].weight.numpy().copy(), seq[1].weight.numpy().copy()
        emb.eval()
        with torch.no_grad():
            out[f"{name}.embed_rows"] = emb(torch.arange(c["V"])).numpy()               # AdaptiveInput.forward over the whole vocabulary
    else:
        emb = nn.Embedding(c["V"], d)
        with torch.no_grad():
            emb.weight.copy_(t(m["E"]))
        out[f"{name}.E"] = m["E"]
    dec.embed_tokens = emb
    # ---- positions
    if c["positions"] == "sinusoidal":
        dec.embed_positions = R.Sin(d, PAD, init_size=8)                                # (grows on demand: :70-75)
    else:
        dec.embed_positions = R.Learned(m["P"].shape[0], d, PAD)
        with torch.no_grad():
            dec.embed_positions.weight.copy_(t(m["P"]))
    with torch.no_grad():
        out[f"{name}.pos_rows"] = dec.embed_positions(t(tokens)).numpy()[0]             # [T, d]: rows pad + 1 .. pad + T
    ln = lambda gb: None if gb is None else _ln_module(d, gb)
    dec.layernorm_embedding, dec.layer_norm = ln(m["ln_emb"]), ln(m["ln_out"])
    layers = []
    for w in m["layers"]:
        lay = R.Layer(args, no_encoder_attn=True)
        sd = {"self_attn.q_proj.weight": w["wq"], "self_attn.q_proj.bias": w["bq"], "self_attn.k_proj.weight": w["wk"], "self_attn.k_proj.bias": w["bk"],
              "self_attn.v_proj.weight": w["wv"], "self_attn.v_proj.bias": w["bv"], "self_attn.out_proj.weight": w["wo"], "self_attn.out_proj.bias": w["bo"],
              "self_attn_layer_norm.weight": w["ln1_g"], "self_attn_layer_norm.bias": w["ln1_b"], "final_layer_norm.weight": w["ln2_g"],
              "final_layer_norm.bias": w["ln2_b"], "fc1.weight": w["w1"], "fc1.bias": w["b1"], "fc2.weight": w["w2"], "fc2.bias": w["b2"]}
        lay.load_state_dict({k: t(v) for k, v in sd.items()}, strict=True)
        lay.eval()
        layers.append(lay)
    dec.layers, dec.num_layers = layers, len(layers)
    with torch.no_grad():
        x, extra = dec.extract_features(t(tokens))
    out[f"{name}.tokens"] = tokens
    out[f"{name}.x"] = x.numpy()                                                         # [bsz, T, d]
    out[f"{name}.last_inner"] = extra["inner_states"][-1].transpose(0, 1).numpy()        # T x B x C -> B x T x C
    if c["keytype"]:
        out[f"{name}.last_ffn_input"] = extra[c["keytype"]].transpose(0, 1).numpy()
    # the reference's own model.half() run (fairseq_cli/eval_lm.py:114-115): the yardstick of the --fp16 test, as in make_fp16.py
    for mod in [emb, dec.embed_positions, dec.layernorm_embedding, dec.layer_norm] + layers:
        if mod is not None:
            mod.half()
    dec._future_mask = torch.empty(0)
    with torch.no_grad():
        xh, extra_h = dec.extract_features(t(tokens))
    assert xh.dtype == torch.float16
    out[f"{name}.x_half"] = xh.numpy()
    out[f"{name}.last_inner_half"] = extra_h["inner_states"][-1].transpose(0, 1).numpy()
    # the weights, so that the fixture stands alone
    for k in ("ln_emb", "ln_out"):
        if m[k] is not None:
            out[f"{name}.{k}.g"], out[f"{name}.{k}.b"] = m[k]
    if m["P"] is not None:
        out[f"{name}.P"] = m["P"]
    for i, w in enumerate(m["layers"]):
        for k, v in w.items():
            out[f"{name}.layer{i}.{k}"] = v


def _ln_module(d, gb):
    mod = nn.LayerNorm(d)
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(gb[0]))
        mod.bias.copy_(torch.from_numpy(gb[1]))
    return mod


def run_context(R, out):
    """The collater of LMContextWindowDataset over runs of samples of the given lengths, one sample per batch in corpus order (what
    ``--max-tokens = --tokens-per-sample`` gives): the context every sample got, and the rows themselves for the first run."""
    runs = {"none": (dict(tps=16, w=8), [8, 8, 8, 8, 5]),                                # tokens_per_sample - w = 8: blocks of 8
            "complete": (dict(tps=24, w=10), [14, 9, 3, 30, 12, 14, 1, 40, 2, 2]),       # sentences longer than the block among them
            "wide": (dict(tps=3072, w=2560), [512] * 7 + [300])}
    for name, (cfg, lengths) in runs.items():
        ds = R.CtxDataset(StubDataset(), cfg["tps"] - cfg["w"], cfg["w"], PAD)
        stream = np.arange(100, 100 + sum(lengths), dtype=np.int64)                      # distinct ids: a row names its own tokens
        starts, pos, rows = [], 0, []
        for n in lengths:
            tgt = stream[pos:pos + n]
            src = tgt - 1                                                                # "shifted by one": id k - 1 stands in front of id k
            s = ds.collater([(src, tgt)])
            starts.append(int(s["start_indices"][0]))
            row = s["net_input"]["src_tokens"][0].numpy()
            rows.append(row[row != PAD])
            pos += n
        out[f"ctx.{name}.cfg"] = np.array([cfg["tps"], cfg["w"]])
        out[f"ctx.{name}.lengths"] = np.array(lengths)
        out[f"ctx.{name}.start_indices"] = np.array(starts)
        out[f"ctx.{name}.first_src"] = np.array([int(r[0]) for r in rows])
        out[f"ctx.{name}.row_len"] = np.array([len(r) for r in rows])


def main(ref):
    R = load_reference(ref)
    out = {}
    for name, c in CASES.items():
        run_case(R, name, c, out)
    run_context(R, out)
    np.savez_compressed(os.path.join(HERE, "transformer_lm.npz"), **out)
    print("transformer_lm.npz:", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "transformer_lm.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/make_transformer_lm.py <reference source tree>")
    main(os.path.abspath(sys.argv[1]))
