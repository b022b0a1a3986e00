#!/usr/bin/env python3
"""What `--knn-sim-func ip | l2` costs: the similarity recompute (`ops.knn_recompute_sims`) over a key table in HBM.

A synthetic fp16 key table of `--key-rows` x 1024 (default 16 Mi rows = 34.4 GB: far larger than the Infinity Cache, so rows come
from HBM), uniformly random ids, timed with device events after a warm-up, the variants taking turns inside every repetition.

Kernel part: `ip`, cosine `ip` and `l2` at n = 32768, k = 1024, d = 1024 -> time, n k d x 2 bytes of key rows, TB/s.
Parent part: the torch path this kernel replaced (`keys[idx].float()`, broadcast product, sum: three [n, k, d] temporaries, 10 n k d
bytes) against the kernel at `--parent-n` queries (1024 needs 10 GiB of temporaries), per query.
Step part: the with-search step of tools/sweep_bench.py (two lanes, full synthetic store, HGT features -> on-device IVF-PQ search ->
adaptive softmax -> interpolation -> score sum) with and without the recompute, in alternating rounds.  The synthetic index names 103 M
keys, the key table here has fewer rows: BOTH variants fold the returned ids into the table (`ids % key_rows`, one small torch kernel,
tool plumbing), so the labels no longer belong to the ids -- a timing run, not a scoring one.

    python tools/knn_resim_bench.py [--no-step] [--no-parent] [--reps 10] [--steps 12] [--rounds 3] [--out FILE] [bench.py's shape options]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd import ops

MODES = [("ip", "ip", False), ("ip cosine", "ip", True), ("l2", "l2", False)]


def make_keys(rows, d, dev):
    keys = torch.empty(rows, d, dtype=torch.float16, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    for r0 in range(0, rows, 1 << 20):
        keys[r0:r0 + (1 << 20)].normal_(generator=g)
    return keys


def timed(variants, reps):
    for _ in range(2):                                              # warm-up: allocations, code objects, clocks
        for _, f in variants:
            f()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in variants}
    for _ in range(reps):
        for name, f in variants:                                    # the variants take turns: drift hits them alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[name].append(e0.elapsed_time(e1))
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in ts.items()}


def kernel_part(keys, n, k, reps, log):
    dev, (rows, d) = keys.device, keys.shape
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    q = torch.randn(n, d, generator=g, device=dev)
    q = q / (q ** 2).sum(-1, keepdim=True).sqrt()
    ids = torch.randint(0, rows, (n, k), generator=g, device=dev, dtype=torch.int64)
    ids[::7, -2:] = -1
    out = torch.empty(n, k, device=dev, dtype=torch.float32)
    variants = [(name, (lambda m=m, nk=nk: ops.knn_recompute_sims(q, ids, keys, m, nk, out=out))) for name, m, nk in MODES]
    res = {}
    moved = float(n) * k * d * 2
    for name, (med, mn) in timed(variants, reps).items():
        res[name] = {"median_ms": med, "min_ms": mn, "key_bytes": moved, "TBps": moved / med / 1e9}
        log(f"knn_recompute_sims {name:9s} n={n} k={k} d={d}: median {med:7.3f} ms  min {mn:7.3f} ms  ({moved / 1e9:.1f} GB of key rows, "
            f"{moved / med / 1e9:.2f} TB/s; {med / (n / 8192):.3f} ms per 8192 queries)")
    return res


def parent_sims(keys, knns, queries, fn, cosine):
    """KNNModel._sims of the parent commit, in-HBM path, verbatim."""
    def sims_of(vecs, q):
        if fn == "l2":
            return -1 * torch.sum((q[:, None, :] - vecs) ** 2, dim=2)
        if cosine:
            vecs = vecs / (vecs ** 2).sum(-1, keepdims=True).sqrt()
        return (vecs * q[:, None, :]).sum(dim=-1)
    idx = torch.where(knns < 0, knns + keys.shape[0], knns)
    return sims_of(keys[idx].float(), queries)


def parent_part(keys, n, k, reps, log):
    dev, (rows, d) = keys.device, keys.shape
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    q = torch.randn(n, d, generator=g, device=dev)
    q = q / (q ** 2).sum(-1, keepdim=True).sqrt()
    ids = torch.randint(0, rows, (n, k), generator=g, device=dev, dtype=torch.int64)
    ids[::7, -2:] = -1
    res = {}
    for name, m, nk in MODES:
        variants = [("parent torch path", lambda: parent_sims(keys, ids, q, m, nk)),
                    ("kernel", lambda: ops.knn_recompute_sims(q, ids, keys, m, nk))]
        diff = float((variants[0][1]() - variants[1][1]()).abs().max())
        t = timed(variants, reps)
        (pm, _), (km, _) = t["parent torch path"], t["kernel"]
        res[name] = {"n": n, "parent_ms": pm, "kernel_ms": km, "ratio": km / pm, "max_abs_diff": diff}
        log(f"{name:9s} n={n} k={k} d={d}: parent torch path {pm:8.3f} ms ({pm / n * 1e3:7.2f} us per query)  kernel {km:7.3f} ms "
            f"({km / n * 1e3:6.2f} us per query)  kernel / parent = {km / pm:.4f}  (max |difference| {diff:.2e})")
        torch.cuda.empty_cache()
    return res


class FoldedIndex:
    """The synthetic index with its ids folded into the key table of this tool (see the module docstring)."""

    class Handle:
        def __init__(self, h, rows):
            self.h, self.rows = h, rows

        def result(self):
            sims, ids, vals = self.h.result()
            return sims, torch.where(ids < 0, ids, ids % self.rows), vals

    def __init__(self, index, rows):
        self.index, self.rows = index, rows

    def search_begin(self, q, k, return_vals=True):
        return FoldedIndex.Handle(self.index.search_begin(q, k, return_vals=return_vals), self.rows)


def step_part(argv, keys, steps, rounds, log):
    import bench
    from gnnlm_amd.synthetic import synthetic_ivfpq_index
    sys.argv = [sys.argv[0], "--pool", "4"] + argv
    args = bench.parse()
    dev = keys.device
    eng, shard, sharded, cpu_model, (d, vocab) = bench.build(args, dev, 0, 1)
    assert eng.hgt.hidden_dim == keys.shape[1], "the key table must have the model's width"
    batches = bench.make_batches(args, dev, 0, d, vocab)
    idx = synthetic_ivfpq_index(args.n_store, eng.hgt.hidden_dim, 4096, 64, dev, nprobe=32)
    idx.attach_vals(eng.store.vals)
    idx = FoldedIndex(idx, keys.shape[0])
    lanes = 2
    streams = [torch.cuda.current_stream()] + [torch.cuda.Stream(device=dev) for _ in range(lanes - 1)]
    for s_ in streams[1:]:
        s_.wait_stream(streams[0])
    accs = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(lanes)]

    def run(n, fn):
        pend = [None] * lanes
        kw = dict(knn_keys=keys, knn_sim_func=fn) if fn else {}
        for i in range(n):
            j = i % lanes
            with torch.cuda.stream(streams[j]):
                if pend[j] is not None:
                    ops.masked_sum_f64(eng.score_finish(pend[j])["logp"], None, accs[j])
                pend[j] = eng.score_begin(batches[i % len(batches)], args.lmbda, args.temperature, knn_index=idx, k=args.k, **kw)
        for j in range(lanes):
            if pend[j] is not None:
                with torch.cuda.stream(streams[j]):
                    ops.masked_sum_f64(eng.score_finish(pend[j])["logp"], None, accs[j])
        torch.cuda.synchronize()

    names = [("do_not_recomp_ip", None), ("ip", "ip"), ("l2", "l2")]
    for _, fn in names:
        run(2 * lanes, fn)                                         # warm-up of every variant: allocations of every lane
    times = {name: [] for name, _ in names}
    for _ in range(rounds):
        for name, fn in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(steps, fn)
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    n_tok = batches[0].targets.shape[0]
    med = {k_: sorted(v)[len(v) // 2] for k_, v in times.items()}
    for name, _ in names:
        log(f"step --knn-sim-func {name:16s} ({n_tok} tokens, k={args.k}, {lanes} lanes): median {med[name]:.3f} ms per step "
            f"({[round(t, 3) for t in times[name]]})")
    for name in ("ip", "l2"):
        log(f"step {name} - step do_not_recomp_ip = {med[name] - med['do_not_recomp_ip']:.3f} ms  (ratio {med[name] / med['do_not_recomp_ip']:.4f})")
    return {"tokens": n_tok, "lanes": lanes, "k": args.k, "ms": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--kernel-k", type=int, default=1024)
    ap.add_argument("--dim", type=int, default=1024)
    ap.add_argument("--key-rows", type=int, default=1 << 24)
    ap.add_argument("--parent-n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines and the figures (JSON) to this file")
    a, rest = ap.parse_known_args()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    dev = torch.device("cuda:0")
    keys = make_keys(a.key_rows, a.dim, dev)
    log(f"key table: {a.key_rows} x {a.dim} fp16 = {keys.numel() * 2 / 1e9:.1f} GB in HBM, uniformly random ids")
    res = {"key_rows": a.key_rows, "dim": a.dim}
    if not a.no_kernel:
        res["kernel"] = kernel_part(keys, a.n, a.kernel_k, a.reps, log)
    if not a.no_parent:
        res["parent"] = parent_part(keys, a.parent_n, a.kernel_k, a.reps, log)
        torch.cuda.empty_cache()
    if not a.no_step:
        res["step"] = step_part(rest, keys, a.steps, a.rounds, log)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
