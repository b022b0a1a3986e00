#!/usr/bin/env python3
"""What `orig_prob_ratio` > 0 (the base-LM / GNN mixture) and its sweep cost.

Kernel part, at the bench's shape (32768 tokens, k = 1024, labels delivered with the neighbours, seeded inputs), device events after
a warm-up, the variants taking turns inside every repetition:
  * the adaptive softmax alone over 32768 seeded rows, twice over two inputs (the two-call form of the base branch, which the step uses)
    and once over the stacked [2n, d] rows (the one-call form, which was measured and dropped);
  * `logp_mix` at 1 and 4 ratios;
  * `knn_interp_grid` with the 75-point grid, one lm row (the kernel of the plain sweep) against 4 lm rows (300 points).
Step part, at the full synthetic store, two lanes as bench.py runs them, alternating rounds: the step at alpha = 0 and at alpha = 0.3,
with the search inside the step and with the search given; the alpha = 0.3 step against the same step that also scores 4 alphas x the
75-point grid and adds up its 300 score sums.  The yardstick for the increment of alpha = 0.3 is the adaptive softmax alone over the
step's own 32768 rows (the batch's features and targets), event-timed here.

    python tools/orig_ratio_bench.py [--no-step] [--no-kernel] [--reps 20] [--steps 12] [--rounds 3] [--out FILE] [bench.py's shape options]"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd import ops

KS, TS, LS = [64, 256, 1024], [1.0, 0.3, 0.1, 0.03, 0.01], [0.05, 0.1, 0.15, 0.2, 0.25]
ALPHAS = [0.0, 0.3, 0.6, 1.0]
ALPHA = 0.3


def timed(variants, reps, log, unit_rows=None):
    """median / min of every variant in us; the variants take turns inside a repetition (drift hits them alike)."""
    for _ in range(3):                                            # warm-up: allocations, code objects, clocks
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
    res = {}
    for name, _ in variants:
        v = sorted(ts[name])
        res[name] = {"median_us": v[len(v) // 2], "min_us": v[0]}
        log(f"{name:58s}: median {v[len(v) // 2]:9.1f} us  min {v[0]:9.1f} us")
    return res


def kernel_part(argv, dev, n, k, reps, log):
    import bench
    sys.argv = [sys.argv[0], "--pool", "4"] + argv
    args = bench.parse()
    eng, shard, sharded, cpu_model, (d, vocab) = bench.build(args, dev, 0, 1)
    asm = eng.asm
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    x, h = torch.randn(n, d, generator=g, device=dev), torch.randn(n, d, generator=g, device=dev)
    tg_asm = torch.randint(0, vocab, (n,), generator=g, device=dev)
    x2, t2 = torch.cat([x, h]), torch.cat([tg_asm, tg_asm])
    two = (asm.target_log_prob(x, tg_asm), asm.target_log_prob(h, tg_asm))
    one = asm.target_log_prob(x2, t2)
    log(f"stacked [2n, d] softmax == the two n-row calls, bit for bit: {bool(torch.equal(one[:n], two[0]) and torch.equal(one[n:], two[1]))}")
    res = {"softmax": timed([(f"adaptive softmax, {n} rows", lambda: asm.target_log_prob(x, tg_asm)),
                             (f"adaptive softmax, two calls of {n} rows", lambda: (asm.target_log_prob(x, tg_asm), asm.target_log_prob(h, tg_asm))),
                             (f"adaptive softmax, one call of {2 * n} stacked rows (no cat)", lambda: asm.target_log_prob(x2, t2)),
                             (f"adaptive softmax, one call of {2 * n} stacked rows + the two cats", lambda: asm.target_log_prob(torch.cat([x, h]), torch.cat([tg_asm, tg_asm])))],
                            reps, log)}
    gnn, base = two
    res["mix"] = timed([("logp_mix, 1 ratio", lambda: ops.logp_mix(gnn, base, [ALPHA])),
                        ("logp_mix, 4 ratios", lambda: ops.logp_mix(gnn, base, ALPHAS))], reps, log)
    del eng, x2, one
    torch.cuda.empty_cache()
    kv = torch.randint(0, 267744, (n, k), generator=g, device=dev, dtype=torch.int32)
    ids = torch.randint(0, 103227021, (n, k), generator=g, device=dev, dtype=torch.int64)
    ids[::7, -2:] = -1
    sims = torch.sort(torch.rand(n, k, generator=g, device=dev) * 0.7 + 0.2, dim=1, descending=True).values.contiguous()
    tg = kv[:, 3].long().contiguous()
    lm = torch.log(torch.rand(4, n, generator=g, device=dev) * 0.9 + 0.01)
    lm0 = lm[0].contiguous()
    ks = [min(v, k) for v in KS]
    G = len(ks) * len(TS) * len(LS)
    a4, a1 = ops.knn_interp_grid(lm, sims, ids, tg, ks, TS, LS, knn_vals=kv)[0], ops.knn_interp_grid(lm0, sims, ids, tg, ks, TS, LS, knn_vals=kv)[0]
    log(f"row block 0 of the 4-row grid == the 1-row grid, bit for bit: {bool(torch.equal(a4[:G], a1))}")
    res["grid"] = timed([(f"knn_interp_grid G = {G}, 1 lm row", lambda: ops.knn_interp_grid(lm0, sims, ids, tg, ks, TS, LS, knn_vals=kv)),
                         (f"knn_interp_grid G = {G}, 4 lm rows ({4 * G} points)", lambda: ops.knn_interp_grid(lm, sims, ids, tg, ks, TS, LS, knn_vals=kv))],
                        reps, log)
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
    sweep = ([min(v, args.k) for v in KS], TS, LS, ALPHAS)
    G = len(ops.grid_points(*sweep))
    lanes = 2
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream(device=dev) for _ in range(lanes - 1)]
    for s_ in streams[1:]:
        s_.wait_stream(streams[0])
    accs = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(lanes)]
    gaccs = [torch.zeros(G, device=dev, dtype=torch.float64) for _ in range(lanes)]
    # search-given batches: the neighbours of one in-step search, handed back with the batch (what a driver with a host-side search does)
    given = []
    for b in batches[:lanes]:
        o = eng.score(b, args.lmbda, args.temperature, knn_index=idx, k=args.k)
        given.append(dataclasses.replace(b, knn_sims=o["knn_sims"].contiguous(), knn_ids=o["knn_ids"].contiguous(), knn_vals=o["knn_vals"].contiguous()))
    torch.cuda.synchronize()

    def finish(p, j):
        out = eng.score_finish(p)
        ops.masked_sum_f64(out["logp"], None, accs[j])
        if "sweep_logp" in out:
            ops.rows_sum_f64(out["sweep_logp"], gaccs[j])

    def run(n, alpha, sw, search):
        pend = [None] * lanes
        for i in range(n):
            j = i % lanes
            with torch.cuda.stream(streams[j]):
                if pend[j] is not None:
                    finish(pend[j], j)
                if search:
                    pend[j] = eng.score_begin(batches[i % len(batches)], args.lmbda, args.temperature, knn_index=idx, k=args.k, sweep=sw, orig_prob_ratio=alpha)
                else:
                    pend[j] = eng.score_begin(given[i % len(given)], args.lmbda, args.temperature, sweep=sw, orig_prob_ratio=alpha)
        for j in range(lanes):
            if pend[j] is not None:
                with torch.cuda.stream(streams[j]):
                    finish(pend[j], j)
        torch.cuda.synchronize()

    # the yardstick: the softmax alone over the step's own rows (the base branch is this call, on these rows)
    b0 = batches[0]
    h0 = b0.tgt_feats
    h0 = ops.half_to_float(h0.contiguous()) if h0.dtype == torch.float16 else h0.float()
    x0 = eng.features(b0)
    yard = timed([(f"adaptive softmax alone, the step's {x0.shape[0]} GNN rows", lambda: eng.asm.target_log_prob(x0, b0.targets)),
                  (f"adaptive softmax alone, the step's {x0.shape[0]} feature rows (the yardstick)", lambda: eng.asm.target_log_prob(h0, b0.targets))], 20, log)
    yard_us = list(yard.values())[1]["median_us"]
    del x0, h0

    variants = [("alpha = 0, with search", (0.0, None, True)), (f"alpha = {ALPHA}, with search", (ALPHA, None, True)),
                (f"alpha = {ALPHA}, with search, + {G}-point sweep", (ALPHA, sweep, True)),
                ("alpha = 0, search given", (0.0, None, False)), (f"alpha = {ALPHA}, search given", (ALPHA, None, False))]
    for _, v in variants:                                          # warm-up of every variant: allocations of every lane
        run(2 * lanes, *v)
    for t_ in accs + gaccs:
        t_.zero_()
    run(2 * lanes, ALPHA, sweep, True)
    own = ops.grid_points(*sweep).index((ALPHA, args.k, args.temperature, args.lmbda))
    same = all(bool(ga[own] == a_[0]) for ga, a_ in zip(gaccs, accs))
    log(f"grid row of the step's own setting == the step's score sum on every lane: {same}")
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps, *v)
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    n_tok = batches[0].targets.shape[0]
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    for name, _ in variants:
        log(f"step, {name:48s} ({n_tok} tokens, {lanes} lanes): median {med[name]:.3f} ms per step ({[round(t, 3) for t in times[name]]})")
    names = [n_ for n_, _ in variants]
    inc = [1e3 * (med[names[1]] - med[names[0]]), 1e3 * (med[names[4]] - med[names[3]])]
    log(f"yardstick (the softmax alone over the step's own rows): {yard_us:.1f} us; the bar for the increment is 1.25 x that = {1.25 * yard_us:.1f} us")
    log(f"increment of alpha = {ALPHA}, with search: {inc[0]:.1f} us = {inc[0] / yard_us:.3f} x the yardstick")
    log(f"increment of alpha = {ALPHA}, search given: {inc[1]:.1f} us = {inc[1] / yard_us:.3f} x the yardstick")
    log(f"sweep step / alpha = {ALPHA} step = {med[names[2]] / med[names[1]]:.4f}  (re-running costs {G} steps)")
    return {"tokens": n_tok, "lanes": lanes, "points": G, "ms": times, "median_ms": med, "own_point_equal": same, "yardstick": yard,
            "increment_us": inc}


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
        res["kernel"] = kernel_part(rest, dev, a.n, a.kernel_k, a.reps, log)
        torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_part(rest, a.steps, a.rounds, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
