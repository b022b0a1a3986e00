#!/usr/bin/env python3
"""Removing keys from an IVF-PQ index against the yardstick of moving the same rows, on a synthetic index (2^24 keys, 4096 lists,
M = 64; the values are random, the time does not depend on them):

  (a) ``ivfpq_train.remove_rows`` of 1 % of the keys, given as 256-id ranges;
  (b) ``ivfpq_train.remove_rows`` of every second key;
  (c) ``ops.ivfpq_list_merge`` relocating the same N0 rows with zero new rows: the add path's kernel with the same traffic.

(a) and (b) are the whole removal as a user runs it: flags, cumulative sum, the two reads of a number (total, n_bad), compaction and
the allocation of the outputs; their stages (``gnnlm_ivfpq_keep_flags``, ``gnnlm_ivfpq_list_compact``) are timed again on their own
with device events.  One process, everything warmed, then the three take turns; per repeat one wall-clock time around a synchronised
call.  Reports medians and spread and the achieved GB/s over N0 * (8 + M) bytes read plus N1 * (8 + M) bytes written (N1 the rows
left), and the expectation (a), (b) <= 2 x (c)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnlm_amd import ivfpq_train, ops  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 24)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    N0, M, nlist = args.rows, args.M, args.nlist
    gen = torch.Generator(device=dev).manual_seed(0)
    lens = torch.bincount(torch.randint(0, nlist, (N0,), device=dev, generator=gen), minlength=nlist)
    off = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    ids = torch.randperm(N0, device=dev, generator=gen)                       # a document's tokens are scattered over the lists
    codes = torch.randint(0, 256, (N0, M), dtype=torch.uint8, device=dev, generator=gen)
    starts = torch.randperm(N0 // 256, device=dev, generator=gen)[:max(1, N0 // 25600)] * 256
    cases = {"a": ivfpq_train.normalize_ranges(ranges=torch.stack([starts, starts + 256], 1), device=dev),
             "b": ivfpq_train.normalize_ranges(ids=torch.arange(0, N0, 2, device=dev), device=dev)}
    no_rows = (torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
               torch.empty(0, M, dtype=torch.uint8, device=dev))
    run = {"a": lambda: ivfpq_train.remove_rows(off, ids, codes, cases["a"]),
           "b": lambda: ivfpq_train.remove_rows(off, ids, codes, cases["b"]),
           "c": lambda: ops.ivfpq_list_merge(off, ids, codes, *no_rows, off)}
    left = {}
    for _ in range(args.warmup):
        for p in run:
            out = run[p]()
            left[p] = int(out[-1].shape[0])
            del out
    ms = {p: [] for p in run}
    for _ in range(args.repeats):
        for p in run:                                                         # the three take turns
            t, out = timed(run[p])
            del out
            ms[p].append(t)
    stage = {}
    for p in ("a", "b"):                                                      # the two entries on their own
        fl, cp = [], []
        for _ in range(args.repeats):
            t, (keep, list_keep) = events(lambda: ops.ivfpq_keep_flags(ids, off, cases[p]))
            fl.append(t)
            new_off = torch.zeros(nlist + 1, dtype=torch.int64, device=dev)
            new_off[1:] = torch.cumsum(list_keep, 0)
            t, out = events(lambda: ops.ivfpq_list_compact(off, ids, codes, keep, new_off))
            cp.append(t)
            del out
        stage[p] = (float(np.median(fl)), float(np.median(cp)))
    print(f"IVF-PQ removal: {N0} keys, {nlist} lists, M = {M}; {args.warmup} warm-up rounds, {args.repeats} repeats, the three alternating; "
          f"wall clock around a synchronised call, median (min .. max)")
    names = {"a": f"(a) remove 1 % in 256-id ranges ({cases['a'].shape[0]} ranges)", "b": f"(b) remove every second key ({cases['b'].shape[0]} ranges)",
             "c": "(c) ivfpq_list_merge of the same rows, no new rows"}
    med = {}
    for p in run:
        v = np.array(ms[p])
        med[p] = float(np.median(v))
        traffic = (N0 + left[p]) * (8 + M)
        print(f"{names[p]}\n    {med[p]:8.3f} ms ({v.min():.3f} .. {v.max():.3f})   {left[p]} rows left   {traffic / med[p] / 1e6:8.1f} GB/s over {traffic / 1e9:.3f} GB")
        if p in stage:
            print(f"    of it gnnlm_ivfpq_keep_flags {stage[p][0]:.3f} ms, gnnlm_ivfpq_list_compact (with its output allocation and one read) {stage[p][1]:.3f} ms")
    for p in ("a", "b"):
        print(f"({p}) / (c) = {med[p] / med['c']:.2f}  (expected: at most 2)")


if __name__ == "__main__":
    main()
