#!/usr/bin/env python3
"""What batches of sentence-like blocks cost against the equal-length step.

    python tools/ragged_step_bench.py [--small] [--no-search] [--out FILE.json]

The SAME 32768 tokens (ids, features, targets, given search results: bench.py's seeded generators) are scored
  equal    as 128 blocks of 256 tokens: the parent's step (causal_attn_256x128_kernel)
  ragged   cut into sentence-like blocks (seeded lengths, mean ~27, a few of several hundred) in ONE step (causal_attn_varlen)
  runs     the same blocks through the only route there was before: one step per run of equally long consecutive blocks
with the search given, and (unless --no-search) with the device-side IVF-PQ search inside the step.  Device events, the timed
shapes warmed up first, three alternating rounds; the spread is the largest deviation of a round from the median.  Kernel (a):
the varlen kernel on 128 x 256 tokens, d_k = 128, against the fused kernel on the same Q / K' / V'.  Kernel times of the two
attention kernels inside the step come from a separate `rocprofv3 --kernel-trace --stats` run of this script (--profile-pass:
no timing, a few steps of each kind)."""
import argparse
import json
import os
import sys
from argparse import Namespace
from dataclasses import replace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sentence_lengths(total, seed=5):
    """Seeded sentence-like block lengths summing to `total`: geometric with mean ~27, one in ~150 several hundred tokens."""
    rs = np.random.RandomState(seed)
    out, left = [], total
    while left > 0:
        n = int(rs.randint(300, 900)) if rs.rand() < 1 / 150 else int(rs.geometric(1 / 27.0))
        n = min(n, left)
        out.append(n)
        left -= n
    return np.asarray(out, dtype=np.int64)


def timed(fns, rounds=3, reps=5):
    """{name: fn} -> {name: (median ms per call, spread ms)}: every fn warmed up, then `rounds` alternating rounds of `reps` calls."""
    for f in fns.values():
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    return {k: (float(np.median(v)), float(np.max(np.abs(np.asarray(v) - np.median(v))))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="tiny shapes (plumbing check)")
    ap.add_argument("--no-search", action="store_true", help="skip the legs with the device-side search inside the step")
    ap.add_argument("--profile-pass", action="store_true", help="a few untimed steps of each kind (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--n-store", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gnnlm_amd import ops
    from gnnlm_amd.ragged import BlockTable
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    T, B = (32, 8) if a.small else (256, 128)
    args = Namespace(small=a.small, n_store=a.n_store or (200000 if a.small else 103227021), store="replicated", force_exchange=False, shard_vals=False,
                     layers=1, precision="f32", tokens_per_sample=T, blocks=B, streams=1, gcn_k=16 if a.small else 128, k=64 if a.small else 1024,
                     pool=1, ids="uniform")
    eng, _, _, _, (d, vocab) = bench.build(args, dev, 0, 1)
    equal = bench.make_batches(args, dev, 0, d, vocab)[0]
    n = T * B
    lengths = sentence_lengths(n)
    table = BlockTable(lengths, dev)
    ragged = replace(equal, n_blocks=len(lengths), T=0, block_off=table.batch(0))
    # the parent's only route: one step per run of equally long consecutive blocks
    off, runs, i = np.concatenate([[0], np.cumsum(lengths)]), [], 0
    while i < len(lengths):
        j = i
        while j + 1 < len(lengths) and lengths[j + 1] == lengths[i]:
            j += 1
        sl = slice(int(off[i]), int(off[j + 1]))
        runs.append(replace(equal, ids=equal.ids[sl].contiguous(), tgt_feats=equal.tgt_feats[sl].contiguous(), targets=equal.targets[sl].contiguous(),
                            knn_sims=equal.knn_sims[sl].contiguous(), knn_ids=equal.knn_ids[sl].contiguous(), n_blocks=j - i + 1, T=int(lengths[i])))
        i = j + 1
    lam, temp = 0.25, 0.01
    res = {"tokens": n, "blocks": int(len(lengths)), "mean_len": float(lengths.mean()), "max_len": int(lengths.max()), "runs": len(runs)}
    # ---- (a) the kernels alone on 128 x 256, d_k = 128
    H, dk = (8, 16) if a.small else (8, 128)
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    Q, K, V = (torch.randn(n, H * dk, generator=g, device=dev) * s for s in (1.0, dk ** -0.5, 1.0))
    eq_table = BlockTable([T] * B, dev).batch(0)
    kern = {"varlen": lambda: ops.causal_attn_varlen(Q, K, V, eq_table, H, 0)}
    if not a.small:
        kern["fused_256x128"] = lambda: ops.causal_attn(Q, K, V, B, T, H, 0)
        assert (kern["varlen"]() - kern["fused_256x128"]()).abs().max().item() < 1e-4
    kern["varlen_sentences"] = lambda: ops.causal_attn_varlen(Q, K, V, table.batch(0), H, 0)
    step = {"equal": lambda: eng.score(equal, lam, temp), "ragged": lambda: eng.score(ragged, lam, temp)}
    if a.profile_pass:
        for f in list(kern.values()) + list(step.values()):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        return
    res["kernel_ms"] = timed(kern, reps=20)
    # ---- (b) the step, search given
    res["step_given_ms"] = timed(step)
    # ---- (c) the same blocks, one step per run of equal lengths (timed once over all runs: it is long)
    def by_runs():
        for r in runs:
            eng.score(r, lam, temp)
    res["step_runs_given_ms"] = timed({"runs": by_runs}, rounds=3, reps=1)["runs"]
    if not a.no_search:
        from gnnlm_amd.synthetic import synthetic_ivfpq_index
        idx = synthetic_ivfpq_index(args.n_store, eng.hgt.hidden_dim, 256 if a.small else 4096, 16 if a.small else 64, dev, nprobe=8 if a.small else 32)
        idx.attach_vals(eng.store.vals)
        res["step_search_ms"] = timed({"equal": lambda: eng.score(equal, lam, temp, knn_index=idx, k=args.k),
                                       "ragged": lambda: eng.score(ragged, lam, temp, knn_index=idx, k=args.k)})
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
