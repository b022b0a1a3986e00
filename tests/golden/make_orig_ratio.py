#!/usr/bin/env python3
"""Golden vectors of the base-LM / GNN mixture (``orig_prob_ratio`` > 0) -> tests/golden/orig_ratio.npz.

Needs a source tree of the reference (the tests only read the stored vectors, never the reference):

    python tests/golden/make_orig_ratio.py <reference source tree>

What is executed from the reference tree (nothing of it is copied into this repo), in the manner of make_golden.py:
  * fairseq/modules/adaptive_softmax.py, adaptive_input.py   loaded by path (AdaptiveSoftmax with tied AdaptiveInput weights);
  * fairseq/models/transformer.py                            ``TokenGraphTransformerDecoder`` reduced with ``ast`` to its two
                                                             methods ``combinetow_probs`` + ``get_normalized_probs`` (bases
                                                             dropped): the mixture exactly as the reference computes it
                                                             (:1056-1062, :1064-1079) on a scripted ``net_output``.

Output is data only: the seeded weights and inputs, and per ratio the target column the reference returned.
"""
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

ALPHAS = (0.1, 0.3, 0.5, 0.9)


def load_decoder_probs():
    """The reference's decoder class with nothing but the two methods of the mixture."""
    src = open(os.path.join(mg.REF, "fairseq/models/transformer.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "TokenGraphTransformerDecoder")
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("combinetow_probs", "get_normalized_probs")]
    assert len(cls.body) == 2
    cls.bases, cls.keywords, cls.decorator_list = [], [], []
    mod = ast.Module(body=[cls], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "math": math}
    exec(compile(mod, "ref:fairseq/models/transformer.py", "exec"), ns)
    return ns["TokenGraphTransformerDecoder"]


def main():
    asm_mod = mg.load_by_path("ref_adaptive_softmax", "fairseq/modules/adaptive_softmax.py")
    ain_mod = mg.load_by_path("ref_adaptive_input", "fairseq/modules/adaptive_input.py")
    Dec = load_decoder_probs()
    torch.manual_seed(11)
    V, d, cutoff = 600, 64, [100, 300]
    ain = ain_mod.AdaptiveInput(V, 1, d, 4, d, cutoff)
    asm = asm_mod.AdaptiveSoftmax(V, d, cutoff, dropout=0.0, factor=4, adaptive_inputs=ain, tie_proj=True).eval()
    with torch.no_grad():                        # (the initialisation's logits are nearly flat: scale the weights so the two branches differ)
        for p in asm.parameters():
            p.mul_(2.0)
    bsz, T = 2, 40
    x = torch.randn(bsz, T, d)                   # the GNN output
    h = 1.2 * torch.randn(bsz, T, d)             # the base LM's feature ("orig_x")
    tgt = torch.randint(0, V, (bsz, T))
    tgt[0, :6] = torch.tensor([0, 99, 100, 299, 300, 599])     # both ends of every band
    out = {"x": x.numpy(), "h": h.numpy(), "target": tgt.numpy(), "cutoff": np.array(cutoff + [V]),
           "class_proj": asm.head.class_proj.weight.detach().numpy(), "alphas": np.array(ALPHAS)}
    for i in range(3):
        e, p = ain.weights_for_band(i)
        out[f"emb{i}"], out[f"proj{i}"] = e.detach().numpy(), p.detach().numpy()
    dec = Dec()
    dec.adaptive_softmax = asm
    with torch.no_grad():
        for a in ALPHAS:
            dec.orig_prob_ratio = a
            dense = dec.get_normalized_probs((x, {"orig_x": h}), True, {"target": tgt})
            out[f"mixed.{a}"] = dense.gather(2, tgt.unsqueeze(-1)).squeeze(-1).numpy()
        # what the reference does at the end of the range (recorded as a fact: DESIGN.md section 6)
        dec.orig_prob_ratio = 1.0
        try:
            dec.get_normalized_probs((x, {"orig_x": h}), True, {"target": tgt})
            raised = ""
        except ValueError as err:
            raised = str(err)
        out["alpha_1_raises"] = np.array(raised)
    np.savez_compressed(os.path.join(HERE, "orig_ratio.npz"), **out)
    print("orig_ratio.npz:", {k: v.shape for k, v in out.items()}, "alpha = 1 ->", repr(raised))


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/make_orig_ratio.py <reference source tree>")
    mg.REF = os.path.abspath(sys.argv[1])
    mg.install_stubs()
    main()
