#!/usr/bin/env python3
"""`--reinit-nfeat` (token store) beside the code store of the same build, on the same neighbour ids.

Recipe shape: d = 1024, 8 heads, blocks of 256 tokens, k_g = 128, context (2, 2); the full-size label table (103,227,021 rows) and
V = 267,744 (WikiText-103): a 1.1-GB embedding table beside a 13.2-GB code table (M = 128, dsub = 8, OPQ).  Content-free operands
(seeded random labels, codes, weights, i.i.d. neighbour ids) -- throughput only, nothing here checks a value.

Reported, each as median and minimum over --reps after a warm-up, the two stores taking turns inside every repetition:
  * tokens/s of the HGT forward (search given: the ids are inputs) for L = 1 (32 blocks) and L = 3 (4 blocks; group merge on,
    centre-state cache off so that every repetition computes the same work);
  * the token gather (`gnnlm_token_gather`) against `gnnlm_pq_gather_decode`: time and bytes moved per second;
  * the star kernel of layer 0 on the embedding table (dense-row route through the label index) against the PQ route.

    python tools/reinit_nfeat_bench.py [--n-store N] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd import ops
from gnnlm_amd.hgt import HGT, CodeStore, NeighborGraph, TokenStore
from gnnlm_amd.synthetic import device_codes


def timed(variants, reps, warm=2):
    """{name: (median ms, min ms)}; the variants take turns inside a repetition."""
    for _ in range(warm):
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, f in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-store", type=int, default=103227021)
    ap.add_argument("--vocab", type=int, default=267744)
    ap.add_argument("--gcn-k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d, H, T, kg, l, r, M, dsub, N, V = 1024, 8, 256, a.gcn_k, 2, 2, 128, 8, a.n_store, a.vocab
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    vals = torch.randint(0, V, (N,), generator=g, device=dev, dtype=torch.int32)
    E = torch.randn(V, d, generator=g, device=dev) * 0.5
    cen = torch.randn(M, 256, dsub, generator=g, device=dev) * 0.5
    A = torch.randn(M * dsub, d, generator=g, device=dev) / (M * dsub) ** 0.5
    tok = TokenStore(embed=E, vals=vals, n_store=N)
    code = CodeStore(codes=device_codes(N, M, dev, 2), centroids=cen, n_store=N, vals=vals, A=A, b=torch.zeros(M * dsub, device=dev))
    res = {"shape": dict(d=d, heads=H, T=T, k_g=kg, left=l, right=r, n_store=N, vocab=V, M=M, dsub=dsub),
           "table_bytes": {"token_embed": E.numel() * 4, "labels": vals.numel() * 4, "codes": code.codes.numel()}}

    for L, blocks in ((1, 32), (3, 4)):
        torch.manual_seed(10 + L)
        model = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=L, n_heads=H)
        model.state_cache_gib = 0.0
        n = blocks * T
        ids = torch.randint(0, N, (n, kg), generator=g, device=dev, dtype=torch.int64)
        feats = torch.randn(n, d, generator=g, device=dev)
        run = lambda st: model(NeighborGraph(ids=ids, n_blocks=blocks, T=T, left=l, right=r, store=st), features={"tgt": feats})
        t = timed([("token_store", lambda: run(tok)), ("code_store", lambda: run(code))], a.reps)
        res[f"forward_L{L}"] = {k: {"blocks": blocks, "median_ms": v[0], "min_ms": v[1], "tokens_per_s_search_given": n / (v[0] * 1e-3)}
                                for k, v in t.items()}
        model.invalidate()
        del model

    G = 4 * T * kg                                                 # the groups of a 4-block step
    ids = torch.randint(0, N, (G,), generator=g, device=dev, dtype=torch.int64)
    S = G * (1 + l + r)
    xt, xc = torch.empty(S, d, device=dev), torch.empty(S, M * dsub, device=dev)
    vt = torch.empty(S, dtype=torch.uint8, device=dev)

    def pq():
        gd = ops._lib.gnnlm_gather_t()
        gd.codes, gd.n_local, gd.n_store, gd.M, gd.dsub, gd.centroids = code.codes.data_ptr(), N, N, M, dsub, cen.data_ptr()
        gd.ids, gd.n_groups, gd.left, gd.right, gd.vals_itemsize = ids.data_ptr(), G, l, r, 4
        gd.out_x, gd.ld_x, gd.out_valid = xc.data_ptr(), M * dsub, vt.data_ptr()
        ops.call_desc("gnnlm_pq_gather_decode", gd)

    t = timed([("token_gather", lambda: ops.token_gather(E, vals, ids, l, r, n_store=N, out_x=xt, want_valid=False)),
               ("pq_gather_decode", pq)], a.reps)
    moved = {"token_gather": S * (8.0 * d + 4), "pq_gather_decode": S * (4.0 * d + M)}
    res["gather"] = {k: {"slots": S, "median_ms": v[0], "min_ms": v[1], "bytes": moved[k], "GB_per_s": moved[k] / (v[0] * 1e-3) / 1e9}
                     for k, v in t.items()}

    n = 4 * T
    nb = torch.randint(0, N, (n, kg), generator=g, device=dev, dtype=torch.int64)
    U = torch.randn(n, H, d, generator=g, device=dev) * 0.05
    lab = ops.neighbor_labels(nb, vals, n_store=N, n_vocab=V)
    t = timed([("star_on_embedding_table", lambda: ops.star_attn(U, nb, X=E, x_group_stride=1, n_store=N, x_index=lab)),
               ("star_on_pq_codes", lambda: ops.star_attn(U, nb, codes=code.codes, centroids=cen, n_store=N))], a.reps)
    moved = {"star_on_embedding_table": n * kg * 4.0 * d + 2 * U.numel() * 4.0, "star_on_pq_codes": n * kg * float(M) + 2 * U.numel() * 4.0}
    res["star_layer0"] = {k: {"tokens": n, "median_ms": v[0], "min_ms": v[1], "bytes": moved[k], "GB_per_s": moved[k] / (v[0] * 1e-3) / 1e9}
                          for k, v in t.items()}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
