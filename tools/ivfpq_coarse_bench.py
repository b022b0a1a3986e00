#!/usr/bin/env python3
"""The coarse step of an IVF-PQ index with many lists (the One Billion Word recipe: `OPQ16_64,IVF1048576,PQ16`, nprobe 32, k = 256,
gnnlm_scripts/one_billion/find_knn.sh:8-21): the DENSE route -- `gnnlm_gemm_nt` writes the [queries, nlist] scores, the probe
selection reads them back, in blocks of 1024 queries as `IVFPQIndex._block_begin` runs it -- against the FUSED route,
`gnnlm_ivfpq_coarse_probes` (csrc/ivfpq_coarse.hip), in one call over the batch as `IVFPQIndex._coarse_fused` runs it and, for
scale, in the dense route's blocks.  The routes take turns inside every repetition; device events around each; medians and minima.

    coarse step alone, P = 32:  8192 x 64 x 1,048,576 / 65,536 / 16,384 lists, and 8192 x 1024 x 4096
    whole `IVFPQIndex.search`:  `synthetic_ivfpq_index` with 1,048,576 lists, d = 64, M = 16, k = 256 over --keys keys
    one k-means assignment step: 2^18 rows x 1,048,576 centroids, P = 1 with the bias -|c|^2 / 2

`ivfpq_train.COARSE_FUSED_MIN_LISTS` is the smallest timed list count from which "fused, one call" is no slower than dense
(never below 16384); the exit status is 1 if fused loses at 1,048,576 lists.  GPU only; reads nothing outside the tree.

    timeout -k 10 900 python tools/ivfpq_coarse_bench.py --out profiles/r25_coarse_bench.txt
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from gnnlm_amd import ivfpq_train, ops
from gnnlm_amd.synthetic import synthetic_ivfpq_index

BLOCK = 1024                                                               # queries per block of the float32 routes (``plan_search``)
FLOOR_MS_PER_TFLOP = 1e3 / 155.0                                           # the f32 matrix rate of the chip: 155 TFLOP/s


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--keys", type=int, default=1 << 26, help="keys of the searched index (64 per list)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-search", action="store_true")
    ap.add_argument("--skip-kmeans", action="store_true")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps: at least 5")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    n, P = args.queries, 32
    say(f"IVF-PQ coarse step, dense (gemm_nt + probe selection, blocks of {BLOCK} queries) against fused (gnnlm_ivfpq_coarse_probes); "
        f"{n} queries, P = {P}; {torch.cuda.get_device_name(dev)}; {args.reps} repetitions, the routes take turns")
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    wins = {}
    for d, nlist in ((64, 1 << 20), (64, 65536), (64, 16384), (1024, 4096)):
        x = torch.randn(n, d, generator=g, device=dev)
        coarse = torch.randn(nlist, d, generator=g, device=dev) / d ** 0.5
        out = {r: (torch.empty(n, P, device=dev), torch.empty(n, P, dtype=torch.int64, device=dev)) for r in ("dense", "fused", "fused1")}

        def dense():
            for s in range(0, n, BLOCK):
                cs = ops.gemm_nt(x[s:s + BLOCK], coarse)
                ops.ivfpq_select_probes(cs, out["dense"][0][s:s + BLOCK], out["dense"][1][s:s + BLOCK], None, True)

        def fused():
            for s in range(0, n, BLOCK):
                ops.ivfpq_coarse_probes(x[s:s + BLOCK], coarse, out["fused"][0][s:s + BLOCK], out["fused"][1][s:s + BLOCK])

        def fused1():
            ops.ivfpq_coarse_probes(x, coarse, *out["fused1"])

        routes = (("dense", dense), ("fused", fused), ("fused1", fused1))
        for _, fn in routes:                                                # warm-up: the timed shapes, once per route
            fn()
        torch.cuda.synchronize()
        same = float((out["dense"][1] == out["fused"][1]).float().mean().item())
        same1 = bool(torch.equal(out["fused"][1], out["fused1"][1]))
        ms = {name: [] for name, _ in routes}
        for _ in range(args.reps):
            for name, fn in routes:
                ms[name].append(timed(fn))
        med = {name: statistics.median(v) for name, v in ms.items()}
        floor = 2.0 * n * d * nlist / 1e12 * FLOOR_MS_PER_TFLOP
        say(f"\n{n} x {d} x {nlist}: the scores alone are {floor:.2f} ms at 155 TFLOP/s; dense image {8.0 * n * nlist / 1e9:.1f} GB out and back")
        for name, label in (("dense", f"dense, blocks of {BLOCK}"), ("fused1", "fused, one call"), ("fused", f"fused, blocks of {BLOCK}")):
            say(f"  {label:24s} median {med[name]:9.3f} ms  min {min(ms[name]):9.3f} ms  ({floor / med[name] * 100:5.1f} % of the floor)  of {args.reps}: "
                + " ".join(f"{v:.3f}" for v in ms[name]))
        say(f"  dense / fused = {med['dense'] / med['fused1']:.2f}x (one call), {med['dense'] / med['fused']:.2f}x (blocks); "
            f"probe ids equal to the dense route's: {same:.6f} (float32 sums in two orders); blocks and one call agree: {same1}")
        wins[(d, nlist)] = med["fused1"] <= med["dense"]
        del x, coarse, out
        flush()
    timed_counts = sorted(nl for (d, nl) in wins if d == 64)
    ok_from = None
    for nl in reversed(timed_counts):
        if not wins[(64, nl)]:
            break
        ok_from = nl
    say(f"\nfused no slower than dense from {ok_from} lists on (of the counts timed at d = 64: {timed_counts}); "
        f"COARSE_FUSED_MIN_LISTS = {ivfpq_train.COARSE_FUSED_MIN_LISTS}")

    if not args.skip_search:
        nlist, d, M, k = 1 << 20, 64, 16, 256
        fz = synthetic_ivfpq_index(args.keys, d, nlist, M, dev, nprobe=32, coarse_route="fused")
        dn = type(fz)(fz.R, fz.coarse, fz.pq, fz.list_off, fz.list_ids, fz.list_codes, nprobe=32, cosine=True, coarse_route="dense")
        assert fz.coarse_route == "fused" and dn.coarse_route == "dense" and fz.route == dn.route
        q = torch.randn(n, d, generator=g, device=dev)
        q = q / q.norm(dim=1, keepdim=True)
        res = {}
        for name, ix in (("dense", dn), ("fused", fz)):
            res[name] = ix.search_device(q, k)
            torch.cuda.synchronize()
        same = float((torch.sort(res["dense"][1], dim=1).values == torch.sort(res["fused"][1], dim=1).values).float().mean().item())
        ms = {"dense": [], "fused": []}
        for _ in range(args.reps):
            for name, ix in (("dense", dn), ("fused", fz)):
                ms[name].append(timed(lambda ix=ix: ix.search_device(q, k)))
        say(f"\nwhole IVFPQIndex.search: {nlist} lists, d = {d}, M = {M} (route {fz.route}), N = {args.keys} keys, nprobe 32, k = {k}, {n} queries")
        for name in ("dense", "fused"):
            say(f"  coarse_route={name:6s} median {statistics.median(ms[name]):9.2f} ms  min {min(ms[name]):9.2f} ms  of {args.reps}: "
                + " ".join(f"{v:.2f}" for v in ms[name]))
        say(f"  dense / fused = {statistics.median(ms['dense']) / statistics.median(ms['fused']):.2f}x; sorted id columns equal: {same:.6f}")
        del fz, dn, res
        flush()

    if not args.skip_kmeans:
        rows, k, d = 1 << 18, 1 << 20, 64
        x = torch.randn(rows, d, generator=g, device=dev)
        cen = torch.randn(k, d, generator=g, device=dev)
        bias = (-0.5 * (cen ** 2).sum(1)).contiguous()
        pv, pi = torch.empty(rows, 1, device=dev), torch.empty(rows, 1, dtype=torch.int64, device=dev)
        fn = lambda: ops.ivfpq_coarse_probes(x, cen, pv, pi, col_bias=bias)
        fn()
        torch.cuda.synchronize()
        t = [timed(fn) for _ in range(args.reps)]
        floor = 2.0 * rows * d * k / 1e12 * FLOOR_MS_PER_TFLOP
        say(f"\none k-means assignment step, {rows} rows x {k} centroids, d = {d}: fused median {statistics.median(t):.1f} ms  min {min(t):.1f} ms "
            f"({floor / statistics.median(t) * 100:.1f} % of the {floor:.0f} ms the scores take at 155 TFLOP/s)")
        need = 4.0 * rows * k / 1e9
        free = torch.cuda.mem_get_info(dev)[0] / 1e9
        say(f"  the dense step's [rows, centroids] float32 image is {need:.0f} GB, {free:.0f} GB are free: "
            + ("set aside, it does not fit" if need > 0.8 * free else "it would fit, not timed"))
    flush()
    return 0 if wins[(64, 1 << 20)] else 1


if __name__ == "__main__":
    sys.exit(main())
