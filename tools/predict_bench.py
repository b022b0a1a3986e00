#!/usr/bin/env python3
"""The three stages of a dense prediction per chunk of rows at the WikiText-103 head, beside a torch restatement
of each on the same GPU.

Shapes: 1024 rows, d = 1024, cutoffs 20000 / 60000 / 267744 with tail dims 256 / 64 (factor 4), k = 1024 neighbours, N = 10.

    stage        this build                                   torch restatement
    head         gnnlm_adaptive_log_probs -> [rows, V]        matmuls + log_softmax per band + cat
    mix          gnnlm_knn_mix_dense                          softmax over the neighbours + scatter_add_ + logaddexp
    top-N+rank   gnnlm_topk_merge (ncols = V) + gnnlm_row_rank   topk + (row > target value).sum

Device events after a warm-up; the two variants of a stage take turns inside every repetition; median and minimum.  Every stage
writes or reads the [rows, V] float32 tensor at least once: its "floor" is rows * V * 4 bytes at 6.3 TB/s (what a float4 copy
reaches on this part), and the share is floor / median.  Before timing the two variants' results are compared.

    python tools/predict_bench.py [--rows 1024] [--reps 20] [--out profiles/r16_predict_bench.txt]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd import ops
from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax

CUTOFF, D, K, TOPN = (20000, 60000, 267744), 1024, 1024, 10
HBM_BYTES_PER_US = 6.3e6          # achievable HBM rate (float4 copy)


def timed(variants, reps, warm=3):
    """{name: (median us, min us)}; the variants take turns inside a repetition."""
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
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the lines and the figures (JSON) to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, V = a.rows, CUTOFF[-1]
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    emb, proj, prev = [], [], 0
    for i, c in enumerate(CUTOFF):
        dim = D // 4 ** i
        emb.append(rnd(c - prev, dim) * dim ** -0.5)
        proj.append(None if i == 0 else rnd(D, dim) * D ** -0.5)
        prev = c
    class_proj = rnd(len(CUTOFF) - 1, D) * D ** -0.5
    asm = AdaptiveSoftmax(list(CUTOFF), emb, proj, class_proj, dev)
    x = rnd(n, D)
    sims = torch.sort(torch.rand(n, K, generator=g, device=dev) * 0.7 + 0.2, dim=1, descending=True).values.contiguous()
    labels = torch.clamp((torch.exp(torch.rand(n, K, generator=g, device=dev) * math.log(V + 1.0)) - 1.0).long(), max=V - 1)   # Zipf-like
    knn_vals = labels.to(torch.int32).contiguous()
    ids = torch.arange(n * K, device=dev, dtype=torch.int64).view(n, K)
    targets = labels[:, 0].contiguous()
    t, lmbda = 1.0, 0.25
    head_w = torch.cat([emb[0], class_proj], 0)

    def torch_head():
        head = torch.log_softmax(x @ head_w.t(), dim=1)
        parts = [head[:, :CUTOFF[0]]]
        for i in range(1, len(CUTOFF)):
            parts.append(torch.log_softmax((x @ proj[i]) @ emb[i].t(), dim=1) + head[:, CUTOFF[0] + i - 1, None])
        return torch.cat(parts, 1)

    def torch_mix(lm):
        p = torch.softmax(sims / t, dim=-1)
        pk = torch.zeros(n, V, device=dev).scatter_add_(1, labels, p)
        return torch.logaddexp(lm + math.log(1 - lmbda), torch.log(pk + 1e-10) + math.log(lmbda))

    def torch_top(dense):
        v, i = torch.topk(dense, TOPN, dim=1)
        tv = dense.gather(1, targets[:, None])
        return v, i, (dense > tv).sum(1)

    lm = asm.log_probs(x)
    mixed = torch.empty_like(lm)
    bv, bi = torch.empty(n, TOPN, device=dev), torch.empty(n, TOPN, device=dev, dtype=torch.int64)
    rank = torch.empty(n, device=dev, dtype=torch.int32)

    def our_top(dense):
        ops.topk_merge(dense, bv, bi, init=True)
        ops.row_rank(dense, targets, out=rank)

    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    d_head = float((lm - torch_head()).abs().max())
    ops.knn_mix_dense(lm, sims, ids, t, lmbda, knn_vals=knn_vals, out=mixed)
    d_mix = float((mixed - torch_mix(lm)).abs().max())
    our_top(mixed)
    tv_, ti_, tr_ = torch_top(mixed)
    d_top = float((bv - tv_).abs().max())
    same_rank = float((rank.long() >= tr_).float().mean())          # ours counts ties with a smaller id too: never below torch's count
    floor = n * V * 4 / HBM_BYTES_PER_US
    log(f"dense prediction, {n} rows, V = {V} (cutoffs {CUTOFF[0]} / {CUTOFF[1]}), d = {D}, k = {K}, N = {TOPN}; {a.reps} repetitions, "
        f"device events; us = median (min); floor = rows * V * 4 B at 6.3 TB/s = {floor:.0f} us")
    log(f"max |ours - torch|: head {d_head:.2e}, mix {d_mix:.2e}, top-N values {d_top:.2e}; rank >= torch's strict count on {same_rank:.3f} of the rows")
    log(f"{'stage':>12} | {'this build us':>20} {'floor/median':>12} | {'torch us':>20} {'floor/median':>12} | {'ours/torch':>10}")
    stages = [("head", lambda: asm.log_probs(x, out=lm), torch_head),
              ("mix", lambda: ops.knn_mix_dense(lm, sims, ids, t, lmbda, knn_vals=knn_vals, out=mixed), lambda: torch_mix(lm)),
              ("top-N+rank", lambda: our_top(mixed), lambda: torch_top(mixed))]
    total = [0.0, 0.0]
    for name, ours, ref in stages:
        r = timed([("ours", ours), ("torch", ref)], a.reps)
        mo, mt = r["ours"][0], r["torch"][0]
        total[0] += mo
        total[1] += mt
        log(f"{name:>12} | {mo:10.1f} ({r['ours'][1]:8.1f}) {floor / mo:12.3f} | {mt:10.1f} ({r['torch'][1]:8.1f}) {floor / mt:12.3f} | {mo / mt:10.3f}")
        rows.append({"stage": name, "rows": n, "ours_us": r["ours"], "torch_us": r["torch"], "floor_us": floor, "ratio": mo / mt})
    log(f"{'sum':>12} | {total[0]:10.1f} {'':10} {'':12} | {total[1]:10.1f} {'':10} {'':12} | {total[0] / total[1]:10.3f}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
