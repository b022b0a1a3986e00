#!/usr/bin/env python3
"""Golden vectors of ``--reinit-nfeat`` (neighbour features from the token embedding) -> tests/golden/reinit_nfeat.npz.

Needs a source tree of the reference (the tests only read the stored vectors, never the reference):

    python tests/golden/make_reinit_nfeat.py <reference source tree>

What is executed from the reference tree (nothing of it is copied into this repo), in the manner of make_golden.py:
  * fairseq/modules/adaptive_input.py        loaded by path: the reference's own ``AdaptiveInput`` is ``embed_tokens``;
  * fairseq/models/transformer.py            ``TokenGraphTransformerDecoder`` reduced with ``ast`` to its method
                                             ``extract_graph_features`` (bases dropped), i.e. the branch
                                             ``ntgt_feat = self.embed_tokens(graph.nodes["ntgt"].data["labels"])`` (:1041-1053);
  * fairseq/models/hgt.py                    exec'd under make_golden.py's DGL stand-in;
  * fairseq/data/token_block_dataset.py      ``new_build_graph`` with ``quant_neighbor_feats = None`` (only ``labels`` are attached
                                             to the ntgt nodes, :369-371,392-394,407-410).

Output is data only: the seeded weights, inputs and labels, and per case the ``tgt`` / ``ntgt`` states after every layer.
"""
import ast
import logging
import os
import sys
from typing import Dict, Optional

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

V, CUTOFF, FACTOR, D, T, KG, N_STORE, PAD = 24, [8, 16], 4, 32, 8, 4, 50, 1
ETYPES = [("tgt", "intra", "tgt"), ("ntgt", "inter", "tgt"), ("ntgt", "intra", "ntgt")]


def load_decoder():
    """The reference's decoder class with nothing but ``extract_graph_features``."""
    src = open(os.path.join(mg.REF, "fairseq/models/transformer.py")).read()
    cls = next(n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "TokenGraphTransformerDecoder")
    cls.body = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "extract_graph_features"]
    assert len(cls.body) == 1
    cls.bases, cls.keywords, cls.decorator_list = [], [], []
    mod = ast.Module(body=[cls], type_ignores=[])
    ast.fix_missing_locations(mod)
    ns = {"torch": torch, "Tensor": torch.Tensor, "Optional": Optional, "Dict": Dict, "EncoderOut": None,
          "logger": logging.getLogger("ref")}
    exec(compile(mod, "ref:fairseq/models/transformer.py", "exec"), ns)
    return ns["TokenGraphTransformerDecoder"]


class Recorder:
    """Stands where ``self.hgt_decoder`` stands: calls the reference's HGT and keeps what it saw and every layer's states."""

    def __init__(self, model):
        self.model = model

    def __call__(self, graph, etypes=None, features=None, incremental_state=None):
        assert sorted(etypes) == sorted(ETYPES)
        self.ntgt_in = graph.nodes["ntgt"].data["h"].clone()
        h = {"tgt": features["tgt"], "ntgt": graph.nodes["ntgt"].data["h"]}
        self.per_layer = []
        for i in range(self.model.n_layers):                   # the layers one by one exactly as HGT.forward does (hgt.py:510-512)
            h = self.model.gcs[i](graph, h, etypes=ETYPES, incremental_state=None)
            self.per_layer.append(h)
        full = self.model(graph, features=features, etypes=ETYPES, incremental_state=incremental_state)
        assert torch.equal(full["tgt"], self.per_layer[-1]["tgt"])
        return full


def main():
    ain_mod = mg.load_by_path("ref_adaptive_input", "fairseq/modules/adaptive_input.py")
    GB, H, Dec = mg.load_graph_builder(), mg.load_hgt(), load_decoder()
    rs = np.random.RandomState(33)
    torch.manual_seed(33)
    ain = ain_mod.AdaptiveInput(V, PAD, D, FACTOR, D, list(CUTOFF)).eval()
    plain = torch.nn.Embedding(V, D, padding_idx=PAD).eval()
    vals = rs.randint(0, V, size=N_STORE).astype(np.int64)
    vals[:8] = [0, 7, 8, 15, 16, 23, PAD, PAD]                 # both ends of every band, the padding id
    vals[N_STORE - 1] = 20
    out = {"vals": vals.astype(np.int32), "cutoff": np.array(CUTOFF + [V]), "pad": np.array(PAD),
           "plain_weight": plain.weight.detach().numpy()}
    for i in range(3):
        e, p = ain.weights_for_band(i)
        out[f"emb{i}"], out[f"proj{i}"] = e.detach().numpy(), p.detach().numpy()
    assert not out["emb0"][PAD].any()
    cases = []
    for l, r in [(0, 0), (1, 1), (2, 2)]:
        nb = rs.randint(0, N_STORE, size=(T, KG)).astype(np.int64)
        nb[1, 1] = -1
        nb[3, :] = -1                                          # a token without neighbours
        nb[0, 0] = 0                                           # centre at row 0: clipped left context
        nb[2, 0] = N_STORE - 1                                 # centre at row N - 1: clipped right context
        nb[4, 0], nb[4, 1] = 6, 6                              # a repeated centre (a padding label)
        nb[5, 2] = 6
        nb[6, 0], nb[6, 1], nb[6, 2] = 1, 3, 5                 # the three bands side by side
        tag = f"l{l}r{r}"
        out[tag + ".nb"] = nb
        g = mg.ref_build_graph(GB, nb, np.zeros(T, np.int64), None, vals, l, r, N_STORE)
        assert "h" not in g.nodes["ntgt"].data
        out[tag + ".ntgt_labels"] = g.nodes["ntgt"].data["labels"].numpy()
        for n_layers, n_heads in [(1, 2), (2, 8), (3, 2)]:
            cases.append((tag, g, n_layers, n_heads, "adaptive"))
        if (l, r) == (2, 2):
            cases += [(tag, g, 1, 8, "adaptive"), (tag, g, 3, 8, "adaptive"), (tag, g, 2, 2, "plain")]
    for tag, g, n_layers, n_heads, kind in cases:
        torch.manual_seed(300 + n_layers * 10 + n_heads)
        model = H["HGT"](ntype2idx={"tgt": 0, "ntgt": 1}, etype2idx={"intra": 0, "inter": 1}, in_dim=D, hidden_dim=D, out_dim=D,
                         n_layers=n_layers, n_heads=n_heads, dropout=0.1, two_stream=False, attn_drop=0.1).eval()
        with torch.no_grad():
            for nm, p in model.named_parameters():             # move every parameter off its init value
                if "norms" in nm or "relation_pri" in nm or "bias" in nm:
                    p.add_(torch.randn_like(p) * 0.1)
        tgt = torch.from_numpy(rs.randn(T, D).astype(np.float16).astype(np.float32))
        dec = Dec()
        dec.embed_dim, dec.hgt_etypes, dec.tgt_quantizer = D, list(ETYPES), None
        dec.embed_tokens = ain if kind == "adaptive" else plain
        dec.hgt_decoder = rec = Recorder(model)
        with torch.no_grad():
            x = dec.extract_graph_features(tgt.view(1, T, D), torch.zeros(1, T, dtype=torch.long), g)
        assert "h" not in g.nodes["ntgt"].data                 # (local_scope: the graph is handed back as it came)
        assert torch.equal(x.view(T, D), rec.per_layer[-1]["tgt"])
        key = f"{tag}.L{n_layers}H{n_heads}" + ("" if kind == "adaptive" else "plain")
        out[key + ".tgt_in"], out[key + ".ntgt_in"] = tgt.numpy(), rec.ntgt_in.numpy()
        for i, hh in enumerate(rec.per_layer):
            out[key + f".tgt_out{i}"], out[key + f".ntgt_out{i}"] = hh["tgt"].numpy(), hh["ntgt"].numpy()
        for nm, p in model.state_dict().items():                # (seeded per (layers, heads): one copy serves every graph)
            k_sd = f"sd.L{n_layers}H{n_heads}." + nm
            assert k_sd not in out or np.array_equal(out[k_sd], p.numpy())
            out[k_sd] = p.numpy()
    np.savez_compressed(os.path.join(HERE, "reinit_nfeat.npz"), **out)
    print("reinit_nfeat.npz:", len(cases), "cases,", len(out), "arrays,", os.path.getsize(os.path.join(HERE, "reinit_nfeat.npz")), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/make_reinit_nfeat.py <reference source tree>")
    mg.REF = os.path.abspath(sys.argv[1])
    mg.install_stubs()
    main()
