#!/usr/bin/env python3
"""L2 IVF-PQ search at the reference's index shape (`IVF4096,PQ64`, nprobe 32, k = 1024, 8192 queries per search, d = 1024;
`IndexBuilder`'s default metric, knn/index_builder.py:26,118) over a synthetic index of as many keys as tools/ivfpq_bench.py
searches (103,227,021; shape-true, content-free): the two routes of DESIGN.md 7.12 over the SAME arrays, taking turns inside every
repetition --

    (a) scan="rowmajor": the per-list table `list_term`, one 2 x 64 KiB table fill per (query, list) task, row-major look-ups
    (b) the default at M = 64: one `key_term` per key, the packed float32 scan (tables per query, conflict-free look-ups)

and, for scale, (c) the inner-product int8 matrix-core search of the same arrays.  Device events around whole searches after a
warm-up of every route; medians and minima.  One process, one GPU; run it under a time limit and keep the output:

    timeout -k 10 900 python tools/ivfpq_l2_bench.py --out profiles/r14_ivfpq_l2_bench.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gnnlm_amd.ivfpq import IVFPQIndex
from gnnlm_amd.synthetic import synthetic_ivfpq_index

ARRAYS = ("R", "coarse", "pq", "list_off", "list_ids", "list_codes")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--keys", type=int, default=103227021)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    new = synthetic_ivfpq_index(args.keys, args.d, args.nlist, 64, dev, nprobe=args.nprobe, metric="l2")
    arrs = [getattr(new, a) for a in ARRAYS]
    old = IVFPQIndex(*arrs, nprobe=args.nprobe, cosine=False, metric="l2", scan="rowmajor")
    ip8 = IVFPQIndex(*arrs, nprobe=args.nprobe, cosine=True)
    assert new.key_term is not None and new.packed_codes is not None and new.list_term is None
    assert old.list_term is not None and old.packed_codes is None and old.key_term is None and ip8.tiles is not None
    routes = (("a  L2 list_term, row-major scan", old), ("b  L2 key_term, packed f32 scan", new), ("c  IP int8 matrix-core search", ip8))
    torch.manual_seed(0)
    q = torch.randn(args.queries, args.d, device=dev)
    q = q / q.norm(dim=1, keepdim=True)
    say(f"L2 IVF-PQ search: IVF{args.nlist},PQ64, d = {args.d}, {args.keys} keys, nprobe {args.nprobe}, k = {args.k}, {args.queries} queries per search; "
        f"{torch.cuda.get_device_name(dev)}")
    res = {}
    for name, idx in routes:                                                # warm-up: the timed shapes, once per route
        res[name] = idx.search_device(q, args.k)
        torch.cuda.synchronize()
    # the two L2 routes find the same neighbours (float32 sums in two orders: near-ties at the k-th place may differ)
    da, ia = res[routes[0][0]]
    db, ib = res[routes[1][0]]
    same = float((torch.sort(ia, dim=1).values == torch.sort(ib, dim=1).values).float().mean().item())
    say(f"routes a / b: {same:.6f} of the sorted id columns equal, max |d dist| = {float((da - db).abs().max().item()):.3e} "
        f"at distances up to {float(da.max().item()):.3f}")
    ms = {name: [] for name, _ in routes}
    for _ in range(args.reps):
        for name, idx in routes:                                            # the routes take turns inside every repetition
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            idx.search_device(q, args.k)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    for name, idx in routes:
        st = idx.stats
        say(f"{name:34s} median {statistics.median(ms[name]):9.2f} ms  min {min(ms[name]):9.2f} ms  of {args.reps}: "
            + " ".join(f"{v:.2f}" for v in ms[name])
            + f"   (pairs/query {st['pairs'] / args.queries:.0f}, candidates/query {st['candidates'] / args.queries:.0f}, searched again {st['requeried']})")
    a, b, c = (statistics.median(ms[name]) for name, _ in routes)
    say(f"median a / median b = {a / b:.2f}x;  median b / median c = {b / c:.2f}x (the distance to the inner-product int8 search)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if b <= a else 1


if __name__ == "__main__":
    sys.exit(main())
