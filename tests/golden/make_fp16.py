#!/usr/bin/env python3
"""Generate tests/golden/hgt_fp16.npz -- the yardstick of `eval_lm --fp16` -- by RUNNING THE REFERENCE ITSELF:

    python tests/golden/make_fp16.py <reference source tree>

The reference's ``HGT.forward`` (fairseq/models/hgt.py, on graphs built by its own ``new_build_graph``) and its
``AdaptiveSoftmax.get_log_prob`` are executed where they lie, under the stand-ins of make_golden.py, twice per case: in float64
(``ref_f64``) and as ``model.half()`` on half inputs (``ref_half``: what `fairseq-eval-lm --fp16` computes).  The inputs are the
seeded arrays of tests/fp16_inputs.py; the fixture stores only the outputs and a float64 checksum of the inputs, so the tests
regenerate the inputs and notice if they drift.  Nothing of the reference is copied into this repository.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg            # noqa: E402  (the stand-ins and loaders)
import fp16_inputs as fi            # noqa: E402

ETYPES = [("tgt", "intra", "tgt"), ("ntgt", "inter", "tgt"), ("ntgt", "intra", "ntgt")]


def edge_softmax_rows(sub, score, norm_by="dst"):
    """make_golden's edge_softmax stand-in (torch.softmax over the in-edges of every destination node, in the scores' own dtype)
    without its Python loop over the nodes: the edges are laid out as one -inf padded row per node and softmax-ed along the row --
    the padding contributes exp(-inf) = 0, every row is the same torch.softmax call as the loop makes."""
    assert norm_by == "dst"
    u, v = sub.g._edges[sub.et]
    order = torch.argsort(v, stable=True)
    vs = v[order]
    n = sub.g._n[sub.et[2]]
    deg = torch.bincount(vs, minlength=n)
    start = torch.cumsum(deg, 0) - deg
    col = torch.arange(vs.numel()) - start[vs]
    pad = torch.full((n, int(deg.max())) + tuple(score.shape[1:]), float("-inf"), dtype=score.dtype)
    pad[vs, col] = score[order]
    sm = torch.softmax(pad, dim=1)
    out = torch.empty_like(score)
    out[order] = sm[vs, col]
    return out


def run_hgt(H, GB, pqw, name):
    c, x = fi.HGT_CASES[name], fi.hgt_inputs(name)
    rs = np.random.RandomState(7)
    vals = rs.randint(0, 30, size=c["n_store"]).astype(np.int32)
    g = mg.ref_build_graph(GB, x["nb"], np.zeros(c["T"], np.int64), x["codes"], vals, c["l"], c["r"], c["n_store"])
    codec = mg.make_ref_codec(pqw, x["cen"], None, None)
    model = H["HGT"](ntype2idx={"tgt": 0, "ntgt": 1}, etype2idx={"intra": 0, "inter": 1}, in_dim=c["d"], hidden_dim=c["d"],
                     out_dim=c["d"], n_layers=c["L"], n_heads=c["H"], dropout=0.1, two_stream=False, attn_drop=0.1).eval()
    ref_sd = model.state_dict()
    assert sorted((k, tuple(v.shape)) for k, v in ref_sd.items()) == fi.hgt_param_shapes(c["d"], c["H"], c["L"]), name
    model.load_state_dict({k: torch.from_numpy(v) for k, v in x["sd"].items()}, strict=True)
    out = {}
    with torch.no_grad():
        ntgt = codec.decode(g.nodes["ntgt"].data["h"])                      # transformer.py:1043-1045 (a gather: exact)
        for tag, conv in (("ref_f64", lambda m: m.double()), ("ref_half", lambda m: m.half())):
            with g.local_scope():
                g.nodes["ntgt"].data["h"] = conv(ntgt)
                y = conv(model)(g, features={"tgt": conv(torch.from_numpy(x["tgt"]))}, etypes=ETYPES)["tgt"]
            out[f"{name}.{tag}"] = y.numpy()
            print(name, tag, y.dtype, tuple(y.shape), flush=True)
        model.float()
    out[f"{name}.checksum"] = fi.checksum(x)
    return out


def run_asm():
    asm_mod = mg.load_by_path("ref_adaptive_softmax", "fairseq/modules/adaptive_softmax.py")
    ain_mod = mg.load_by_path("ref_adaptive_input", "fairseq/modules/adaptive_input.py")
    c, x = fi.ASM_CASE, fi.asm_inputs()
    ain = ain_mod.AdaptiveInput(c["vocab"], 1, c["d"], c["factor"], c["d"], list(c["cutoff"]))
    asm = asm_mod.AdaptiveSoftmax(c["vocab"], c["d"], list(c["cutoff"]), dropout=0.0, factor=c["factor"], adaptive_inputs=ain,
                                  tie_proj=True).eval()
    with torch.no_grad():
        for i in range(len(x["emb"])):
            e, p = ain.weights_for_band(i)
            e.copy_(torch.from_numpy(x["emb"][i]))
            if i:
                p.copy_(torch.from_numpy(x["proj"][i]))
        asm.head.class_proj.weight.copy_(torch.from_numpy(x["class_proj"]))
        tgt = torch.from_numpy(x["target"])[None]
        out = {}
        for tag, conv in (("ref_f64", lambda m: m.double()), ("ref_half", lambda m: m.half())):
            conv(ain)
            lp = conv(asm).get_log_prob(conv(torch.from_numpy(x["x"]))[None], tgt)
            out[f"asm.{tag}"] = lp.gather(2, tgt.unsqueeze(-1)).squeeze(-1)[0].numpy()
            print("asm", tag, lp.dtype, flush=True)
    out["asm.checksum"] = fi.checksum(x)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: python tests/golden/make_fp16.py <reference source tree>")
    mg.REF = os.path.abspath(sys.argv[1])
    mg.install_stubs()
    sys.modules["dgl.ops"].edge_softmax = edge_softmax_rows
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    import knn.pq_wrapper as pqw
    H, GB = mg.load_hgt(), mg.load_graph_builder()
    res = {}
    for name in fi.HGT_CASES:
        res.update(run_hgt(H, GB, pqw, name))
    res.update(run_asm())
    path = os.path.join(HERE, "hgt_fp16.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))
