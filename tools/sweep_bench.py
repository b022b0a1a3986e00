#!/usr/bin/env python3
"""What the kNN-LM tuning sweep costs: `knn_interp_grid` against `knn_interp`, and the with-search step with and without a grid.

Kernel part, at the bench's shape (32768 queries x k = 1024, labels delivered with the neighbours, seeded inputs): the
single-setting kernel, the grid kernel with G = 1 and with the 5 x 5 x 3 grid (5 lmbdas x 5 temperatures x 3 values of k = 75
points), timed with device events after a warm-up, the variants taking turns inside every repetition.
Step part, at the full synthetic store, two lanes as bench.py runs them (HGT features -> on-device IVF-PQ search -> adaptive
softmax -> interpolation -> score sums): the plain step against the step that also scores the 75-point grid, in alternating rounds.

    python tools/sweep_bench.py [--no-step] [--reps 20] [--steps 12] [--rounds 3] [--out FILE] [bench.py's shape options]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd import ops

KS, TS, LS = [64, 256, 1024], [1.0, 0.3, 0.1, 0.03, 0.01], [0.05, 0.1, 0.15, 0.2, 0.25]


def kernel_part(dev, n, k, reps, log):
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    vocab = 267744
    kv = torch.randint(0, vocab, (n, k), generator=g, device=dev, dtype=torch.int32)
    ids = torch.randint(0, 103227021, (n, k), generator=g, device=dev, dtype=torch.int64)
    ids[::7, -2:] = -1
    sims = torch.sort(torch.rand(n, k, generator=g, device=dev) * 0.7 + 0.2, dim=1, descending=True).values.contiguous()
    tg = kv[:, 3].long().contiguous()
    lm = torch.log(torch.rand(n, generator=g, device=dev) * 0.9 + 0.01)
    ks = [min(v, k) for v in KS]
    variants = [("knn_interp (one setting)", 1, lambda: ops.knn_interp(lm, sims, ids, tg, 0.01, 0.25, knn_vals=kv)),
                ("knn_interp_grid G = 1", 1, lambda: ops.knn_interp_grid(lm, sims, ids, tg, [k], [0.01], [0.25], knn_vals=kv)),
                (f"knn_interp_grid G = {len(ks) * len(TS) * len(LS)}", len(ks) * len(TS) * len(LS),
                 lambda: ops.knn_interp_grid(lm, sims, ids, tg, ks, TS, LS, knn_vals=kv))]
    one, g1 = variants[0][2](), variants[1][2]()
    assert all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(one, g1)), "G = 1 differs from knn_interp"
    for _ in range(3):                                            # warm-up: allocations, code objects, clocks
        for _, _, f in variants:
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name, _, _ in variants}
    for _ in range(reps):
        for name, _, f in variants:                               # the variants take turns: drift hits them alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3)
    res = {}
    for name, G, _ in variants:
        v = sorted(ts[name])
        med, mn = v[len(v) // 2], v[0]
        moved = n * k * 16.0 + n * (12.0 + 4.0 * G + (12.0 if G == 1 else 4.0 * len(ks) * len(TS) + 8.0 * len(ks)))
        res[name] = {"median_us": med, "min_us": mn, "points": G, "bytes": moved, "GBps": moved / med / 1e3}
        log(f"{name:28s}: median {med:8.1f} us  min {mn:8.1f} us  ({moved / 1e6:.1f} MB moved, {moved / med / 1e3:7.1f} GB/s; "
            f"{med / (n / 8192):.1f} us per 8192 tokens)")
    return res


def step_part(argv, steps, rounds, log):
    import bench
    from gnnlm_amd.synthetic import synthetic_ivfpq_index
    sys.argv = [sys.argv[0], "--pool", "4"] + argv
    args = bench.parse()
    dev = torch.device("cuda:0")
    eng, shard, sharded, cpu_model, (d, vocab) = bench.build(args, dev, 0, 1)
    batches = bench.make_batches(args, dev, 0, d, vocab)
    idx = synthetic_ivfpq_index(args.n_store, eng.hgt.hidden_dim, 4096, 64, dev, nprobe=32)
    idx.attach_vals(eng.store.vals)
    sweep = ([min(v, args.k) for v in KS], TS, LS)
    G = len(ops.grid_points(*sweep))
    lanes = 2
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream(device=dev) for _ in range(lanes - 1)]
    for s_ in streams[1:]:
        s_.wait_stream(streams[0])
    accs = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(lanes)]
    gaccs = [torch.zeros(G, device=dev, dtype=torch.float64) for _ in range(lanes)]

    def finish(p, j):
        out = eng.score_finish(p)
        ops.masked_sum_f64(out["logp"], None, accs[j])
        if "sweep_logp" in out:
            ops.rows_sum_f64(out["sweep_logp"], gaccs[j])

    def run(n, sw):
        pend = [None] * lanes
        for i in range(n):
            j = i % lanes
            with torch.cuda.stream(streams[j]):
                if pend[j] is not None:
                    finish(pend[j], j)
                pend[j] = eng.score_begin(batches[i % len(batches)], args.lmbda, args.temperature, knn_index=idx, k=args.k, sweep=sw)
        for j in range(lanes):
            if pend[j] is not None:
                with torch.cuda.stream(streams[j]):
                    finish(pend[j], j)
        torch.cuda.synchronize()

    run(2 * lanes, None)                                           # warm-up of both variants: allocations of every lane
    for t_ in accs + gaccs:
        t_.zero_()
    run(2 * lanes, sweep)
    # the grid's row at the step's own setting is the step's own score, bit for bit
    own = ops.grid_points(*sweep).index((args.k, args.temperature, args.lmbda))
    same = all(bool(ga[own] == a_[0]) for ga, a_ in zip(gaccs, accs))
    log(f"grid row of the step's own setting == the step's score sum on every lane: {same}")
    times = {"plain": [], "sweep": []}
    for _ in range(rounds):
        for name, sw in (("plain", None), ("sweep", sweep)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps, sw)
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    n_tok = batches[0].targets.shape[0]
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    for k_ in ("plain", "sweep"):
        log(f"step {k_:5s} ({n_tok} tokens, {lanes} lanes{', ' + str(G) + '-point grid' if k_ == 'sweep' else ''}): median {med[k_]:.3f} ms per step "
            f"({[round(t, 3) for t in times[k_]]})")
    log(f"sweep step / plain step = {med['sweep'] / med['plain']:.4f}  (re-running costs {G} plain steps)")
    return {"tokens": n_tok, "lanes": lanes, "points": G, "plain_ms": times["plain"], "sweep_ms": times["sweep"],
            "ratio": med["sweep"] / med["plain"], "own_point_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--kernel-k", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines and the figures (JSON) to this file")
    a, rest = ap.parse_known_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda:0")
    res = {}
    if not a.no_kernel:
        res["kernel"] = kernel_part(dev, a.n, a.kernel_k, a.reps, log)
        torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_part(rest, a.steps, a.rounds, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
