#!/usr/bin/env python3
"""Generation from the GNN-LM at the WikiText-103 shapes, synthetic weights: a 16-layer base LM (d = 1024, H = 8, ffn = 4096,
V = 267,744, adaptive softmax 20000 / 60000), an HGT of L layers, k_g = 128 neighbours per token with context (2, 2), a PQ 128x8 + OPQ
code store and a synthetic IVF-PQ index over N keys searched at nprobe 32.

    python tools/generate_gnn_bench.py [--n-keys 4000000] [--layers-hgt 1,3] [--batches 1,8,32] [--prompt 32 --new 128] [--reps 5]
                                       [--out profiles/generate_gnn_bench.txt]

Per (L, B) it reports, device events throughout:
  * tokens/s     ``GnnGenerator.generate`` end to end (greedy, prompt --prompt, --new new tokens): the median of --reps runs and their spread.
  * the stages   of one step at the prefix the run ends at, each bracketed by its own events (median of 20 rounds): base step, search,
                 HGT step, head, pick.  The largest one bounds a step.
  * step vs recompute   ``HGT.step`` against the only thing the build could do before it had the step -- ``GnnLmModel.forward`` over the
                 whole prefix of every sequence as one block, for one new token -- at prefix lengths 64 and 160, the two taking turns in
                 the same call over the same seeded inputs: the ratio of the medians of --reps rounds, with both spreads.
The condition of the run: the step is faster than the recompute at both lengths.  One JSON line per (L, B)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KG, LEFT, RIGHT = 128, 2, 2


def timed(fns, rounds, warmup, before=None):
    """The forms take turns; -> per form (median ms, min, max)."""
    times = [[] for _ in fns]
    for r in range(warmup + rounds):
        for j, fn in enumerate(fns):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[j].append(e0.elapsed_time(e1))
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in times]


def build_head(A, dev, g):
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    cutoff, d = (20000, 60000, A.vocab), A.d
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    emb, proj, prev = [], [], 0
    for i, c in enumerate(cutoff):
        dim = d // 4 ** i
        emb.append(rnd(c - prev, dim) * dim ** -0.5)
        proj.append(None if i == 0 else rnd(d, dim) * d ** -0.5)
        prev = c
    return AdaptiveSoftmax(list(cutoff), emb, proj, rnd(len(cutoff) - 1, d) * d ** -0.5, dev)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n-keys", type=int, default=4000000)
    p.add_argument("--nlist", type=int, default=4096)
    p.add_argument("--layers-hgt", default="1,3")
    p.add_argument("--batches", default="1,8,32")
    p.add_argument("--prompt", type=int, default=32)
    p.add_argument("--new", type=int, default=128)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--prefixes", default="64,160")
    p.add_argument("--layers", type=int, default=16)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--ffn", type=int, default=4096)
    p.add_argument("--vocab", type=int, default=267744)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--out", default=None)
    A = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_gnn_bench needs the GPU: a timing taken elsewhere says nothing about it")
    import generate_bench
    from gnnlm_amd import ops
    from gnnlm_amd.generate_gnn import GnnGenerator, IndexSearch
    from gnnlm_amd.hgt import HGT, CodeStore, NeighborGraph
    from gnnlm_amd.model import GnnLmModel
    from gnnlm_amd.synthetic import synthetic_ivfpq_index
    dev = torch.device("cuda:0")
    d, N = A.d, A.n_keys
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    t0 = time.time()
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    lm = generate_bench.build(A, dev)
    head = build_head(A, dev, g)
    if A.fp16:
        head.gemm_precision = ops.precision_value("fp16")
    M, dsub = 128, 8
    store = CodeStore(codes=torch.randint(0, 256, (N, M), dtype=torch.uint8, device=dev, generator=g),
                      centroids=torch.randn(M, 256, dsub, device=dev, generator=g) * 0.5, n_store=N,
                      A=torch.randn(M * dsub, d, device=dev, generator=g) / (M * dsub) ** 0.5, b=torch.randn(M * dsub, device=dev, generator=g) * 0.1)
    index = synthetic_ivfpq_index(N, d, A.nlist, 64, dev, nprobe=32)
    knn = IndexSearch(index)
    torch.cuda.synchronize()
    log(f"set-up: base LM {A.layers} x d {d}, V {A.vocab}; code store N = {N} x PQ {M}x{dsub} + OPQ; IVF-PQ index nlist {A.nlist}, nprobe 32: "
        f"{time.time() - t0:.1f} s")
    log(f"{'L':>2} {'B':>3} | {'tokens/s':>9} {'(min .. max)':>19} | {'base':>7} {'search':>7} {'HGT':>7} {'head':>7} {'pick':>7} ms | "
        + " | ".join(f"prefix {n}: step ms, recompute ms, ratio" for n in A.prefixes.split(",")))
    ok = True
    for L in [int(v) for v in A.layers_hgt.split(",")]:
        torch.manual_seed(L)
        hgt = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=L, n_heads=A.heads)
        if A.fp16:
            hgt.gemm_precision = ops.precision_value("fp16")
        gnn = GnnLmModel(hgt, head)
        gen = GnnGenerator(lm, gnn, knn, KG, LEFT, RIGHT, store=store)
        for B in [int(v) for v in A.batches.split(",")]:
            prompts = [[int(t) for t in torch.randint(4, A.vocab, (A.prompt,), generator=g, device=dev).tolist()] for _ in range(B)]
            # ---- end to end
            rates = []
            for r in range(A.reps + 1):
                torch.cuda.synchronize()
                t1 = time.time()
                _, _, lengths = gen.generate(prompts, A.new)
                n_tok = int(lengths.sum().item())
                torch.cuda.synchronize()
                if r:                                                    # (the first run sizes workspaces and tables)
                    rates.append(n_tok / (time.time() - t1))
            # ---- the stages of one step, on the caches the last run left (prefix = prompt + new - 1)
            cache, gcache = gen.lm_cache, gen.gnn_cache
            n_at = A.prompt + A.new - 2
            tok = torch.randint(4, A.vocab, (B,), device=dev, generator=g)
            bv, bi = torch.empty(B, 1, device=dev), torch.empty(B, 1, dtype=torch.int64, device=dev)
            nxt = torch.empty(B, dtype=torch.int64, device=dev)
            hold = {}

            def rewind():
                cache.len.fill_(n_at), gcache.len.fill_(n_at), cache.done.zero_()
                cache.steps = gcache.steps = n_at

            def s_base():
                hold["x"] = lm.step(tok, cache, want_inner=False, want_ffn_input=False)[0]

            def s_search():
                hold["ids"] = knn.search_sims(hold["x"], k=KG)[1].contiguous()

            def s_hgt():
                hold["g"] = gnn.step_rows(hold["x"], hold["ids"], gcache, store, LEFT, RIGHT)

            def s_head():
                hold["lp"] = head.log_probs(hold["g"])

            def s_pick():
                ops.topk_merge(hold["lp"], bv, bi, init=True)
                ops.sample_topk(bv, bi, u=None, out=nxt)

            stage_names = ["base", "search", "hgt", "head", "pick"]
            stages = [[] for _ in stage_names]
            for r in range(25):
                rewind()
                for j, fn in enumerate((s_base, s_search, s_hgt, s_head, s_pick)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if r >= 5:
                        stages[j].append(e0.elapsed_time(e1))
            stage_ms = {n: float(np.median(t)) for n, t in zip(stage_names, stages)}
            # ---- step against recompute over the whole prefix, the two taking turns
            versus = {}
            for n in [int(v) for v in A.prefixes.split(",")]:
                feats = torch.randn(B * (n + 1), d, device=dev, generator=g)
                ids = torch.randint(0, N, (B * (n + 1), KG), device=dev, generator=g)
                rows_new = torch.arange(B, device=dev) * (n + 1) + n
                rows_old = (torch.arange(B, device=dev)[:, None] * (n + 1) + torch.arange(n, device=dev)[None]).reshape(-1)
                kv = gnn.new_cache(B, n + 2, device=dev)
                Gp = NeighborGraph(ids=ids[rows_old].contiguous(), n_blocks=B, T=0, left=LEFT, right=RIGHT, store=store,
                                   block_off=[i * n for i in range(B + 1)])
                hgt.prefill(Gp, {"tgt": feats[rows_old].contiguous()}, kv)
                x_new, ids_new = feats[rows_new].contiguous(), ids[rows_new].contiguous()
                Gs = NeighborGraph(ids=ids_new, n_blocks=B, T=1, left=LEFT, right=RIGHT, store=store)
                Gf = NeighborGraph(ids=ids, n_blocks=B, T=n + 1, left=LEFT, right=RIGHT, store=store, tgt_h=feats)
                src = torch.zeros(B, n + 1, dtype=torch.int64, device=dev)
                out = {}

                def back():
                    kv.len.fill_(n)
                    kv.steps = n

                def f_step():
                    out["step"] = hgt.step(Gs, {"tgt": x_new}, kv)["tgt"]

                def f_full():
                    out["full"] = gnn(src, graph=Gf)[0].view(B, n + 1, d)[:, n]

                (t_s, t_f) = timed([f_step, f_full], A.reps, 2, before=back)
                diff = float((out["step"] - out["full"]).abs().max())
                versus[n] = {"step_ms": [round(v, 4) for v in t_s], "recompute_ms": [round(v, 4) for v in t_f],
                             "ratio": round(t_f[0] / t_s[0], 2), "max_abs_diff": diff}
                ok = ok and t_s[0] < t_f[0]
                del kv
            bound = max(stage_ms, key=stage_ms.get)
            log(f"{L:>2} {B:>3} | {np.median(rates):>9.1f} ({min(rates):>8.1f} .. {max(rates):>8.1f}) | "
                + " ".join(f"{stage_ms[n]:>7.3f}" for n in stage_names) + "    | "
                + " | ".join(f"{v['step_ms'][0]:.3f} ({v['step_ms'][1]:.3f} .. {v['step_ms'][2]:.3f}), {v['recompute_ms'][0]:.3f} "
                             f"({v['recompute_ms'][1]:.3f} .. {v['recompute_ms'][2]:.3f}), x{v['ratio']}" for v in versus.values())
                + f" | bound by {bound}")
            print(json.dumps({"L": L, "B": B, "N": N, "prompt": A.prompt, "new": A.new, "precision": gnn.precision,
                              "tokens_per_s": round(float(np.median(rates)), 1), "tokens_per_s_min_max": [round(min(rates), 1), round(max(rates), 1)],
                              "stage_ms": {k: round(v, 4) for k, v in stage_ms.items()}, "bound_by": bound,
                              "step_vs_recompute": {str(k): v for k, v in versus.items()}}), flush=True)
            torch.cuda.empty_cache()
    log("HGT.step against GnnLmModel.forward over the whole prefix for one new token (median (min .. max) of the rounds): "
        + ("the step is faster at every prefix length, L and B." if ok else "THE STEP IS NOT FASTER SOMEWHERE."))
    if A.out:
        with open(A.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
