#!/usr/bin/env python3
"""Golden vectors of the plain (non-adaptive) output layer -> tests/golden/dense_head.npz.

Needs a source tree of the reference (the tests only read the stored vectors, never the reference):

    python tests/golden/make_dense_head.py <reference source tree>

What is executed from the reference tree (nothing of it is copied into this repo), in the manner of make_orig_ratio.py:
  * fairseq/models/transformer.py   loaded by path and reduced with ``ast``: ``TransformerDecoder`` to its method ``output_layer``
                                    (:843-852), ``TokenGraphTransformerDecoder`` to ``forward`` (:943-1009, annotations dropped: the
                                    precomputed-feature branch :974-976, then the branch ``self.adaptive_softmax is None`` of
                                    :987-1009) and ``get_normalized_probs`` (:1064-1085), bases dropped;
  * fairseq/utils.py                its functions ``softmax`` / ``log_softmax`` (:333-344), extracted with ``ast``.
The graph is a stub that carries ``h`` (the base LM's precomputed feature); ``extract_graph_features`` is stubbed to return the
scripted GNN output.

Output is data only: the seeded weights and inputs, and for each case (shared / unshared output weights x xl_bias absent / present
x orig_prob_ratio) the target column the reference returned.
"""
import ast
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
RATIOS = (0.0, 0.1, 0.5, 0.9)


def _strip_annotations(fn):
    for a in fn.args.args + fn.args.kwonlyargs:
        a.annotation = None
    fn.returns = None
    return fn


def _reduced_class(tree, name, methods):
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)
    cls.body = [_strip_annotations(n) for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in methods]
    assert len(cls.body) == len(methods), (name, [n.name for n in cls.body])
    cls.bases, cls.keywords, cls.decorator_list = [], [], []
    return cls


def load_reference(ref):
    """-> a decoder class made of the reference's output_layer, forward and get_normalized_probs only."""
    utree = ast.parse(open(os.path.join(ref, "fairseq/utils.py")).read())
    fns = [n for n in utree.body if isinstance(n, ast.FunctionDef) and n.name in ("softmax", "log_softmax")]
    assert len(fns) == 2
    uns = {"torch": torch, "F": F}
    mod = ast.Module(body=fns, type_ignores=[])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "ref:fairseq/utils.py", "exec"), uns)
    utils = types.SimpleNamespace(softmax=uns["softmax"], log_softmax=uns["log_softmax"])

    tree = ast.parse(open(os.path.join(ref, "fairseq/models/transformer.py")).read())
    base = _reduced_class(tree, "TransformerDecoder", ("output_layer",))
    graph = _reduced_class(tree, "TokenGraphTransformerDecoder", ("forward", "get_normalized_probs"))
    mod = ast.Module(body=[base, graph], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "F": F, "math": math, "utils": utils}
    exec(compile(mod, "ref:fairseq/models/transformer.py", "exec"), ns)
    return type("RefDecoder", (ns["TokenGraphTransformerDecoder"], ns["TransformerDecoder"]), {})


def main(ref):
    Dec = load_reference(ref)
    torch.manual_seed(13)
    V, d, bsz, T = 205, 64, 2, 40
    scale = 2.5 / math.sqrt(d)                    # logits with a standard deviation of ~2.5: far from flat
    embed_tokens = torch.randn(V, d) * scale      # the shared case's output weight (the input embedding)
    embed_out = torch.randn(V, d) * scale         # the unshared case's
    xl_bias = torch.randn(V)                      # Transformer-XL's output bias (transformer.py:665-668), non-zero
    x = torch.randn(bsz, T, d)                    # the GNN output (what extract_graph_features returns)
    h = 1.2 * torch.randn(bsz, T, d)              # the base LM's feature (graph.nodes["tgt"].data["h"])
    tgt = torch.randint(0, V, (bsz, T))
    tgt[0, :6] = torch.tensor([0, V - 1, 31, 32, 127, 128])
    out = {"x": x.numpy(), "h": h.numpy(), "target": tgt.numpy(), "embed_tokens": embed_tokens.numpy(), "embed_out": embed_out.numpy(),
           "xl_bias": xl_bias.numpy(), "ratios": np.array(RATIOS)}
    graph = types.SimpleNamespace(nodes={"tgt": types.SimpleNamespace(data={"h": h.reshape(-1, d)})})
    prev = torch.zeros(bsz, T, dtype=torch.int64)

    def run(shared, bias, ratio):
        dec = Dec()
        dec.adaptive_softmax, dec.onnx_trace, dec.short_cut = None, False, False
        dec.share_input_output_embed = shared
        dec.embed_tokens = types.SimpleNamespace(weight=embed_tokens)
        dec.embed_out = embed_out
        dec.xl_bias = xl_bias if bias else None
        dec.orig_prob_ratio = ratio
        dec.extract_graph_features = lambda feats, tokens, g, enc, inc: x
        net_output = dec.forward(prev, graph=graph)
        dense = dec.get_normalized_probs(net_output, True, {"target": tgt})
        return dense.gather(2, tgt.unsqueeze(-1)).squeeze(-1)

    with torch.no_grad():
        for shared in (True, False):
            for bias in (False, True):
                name = f"{'shared' if shared else 'unshared'}.{'bias' if bias else 'nobias'}"
                for a in RATIOS:
                    out[f"logp.{name}.{a}"] = run(shared, bias, a).numpy()
                # what the reference does at the end of the range on this branch (a fact for DESIGN.md section 6)
                try:
                    at1 = run(shared, bias, 1.0)
                    raised = ""
                    out[f"logp.{name}.1.0"] = at1.numpy()
                except ValueError as err:
                    raised = str(err)
                out[f"alpha_1_raises.{name}"] = np.array(raised)
    np.savez_compressed(os.path.join(HERE, "dense_head.npz"), **out)
    print("dense_head.npz:", {k: v.shape for k, v in out.items()})
    print("alpha = 1 ->", {k: str(v) for k, v in out.items() if k.startswith("alpha_1_raises")})


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/make_dense_head.py <reference source tree>")
    main(os.path.abspath(sys.argv[1]))
