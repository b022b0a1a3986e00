#!/usr/bin/env python3
"""What `--fp16` (precision 3: float16 GEMM operands, f32 accumulation) buys and costs.

One process per part, device events after a warm-up, the variants taking turns inside every repetition:
  --part gemm   the recipe's ntgt projection 655360 x 1024 x 1024 with a row map and a device-side M, and the 32768 x 20002 x 1024
                LSE head, each under f32, bf16x3 and fp16: time, issued-MFMA TFLOP/s, algorithmic bytes / time against the HBM figure
                of bench.py
  --part step   GnnLmEngine.score at the WikiText-103 shapes of bench.py (--layers 1 or 3, search results given), f32 against fp16 on
                the same engine, alternating; tokens/s; max and RMS |dlogp| of fp16 against f32 on one batch
Run on a build without the mode (the parent commit: --root <its tree>) the fp16 variants are left out and the f32 figures are the
parent's, to lay beside this build's.  A driver script runs every part under its own time limit and stops at the first failure.

    python tools/fp16_bench.py --part gemm|step [--layers 1] [--reps 10] [--steps 8] [--rounds 3] [--root DIR] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--part", choices=["gemm", "step"], required=True)
ap.add_argument("--layers", type=int, default=1)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--small", action="store_true", help="tiny shapes (plumbing check only)")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="tree whose build is measured")
ap.add_argument("--out", default=None, help="append the lines and the figures (JSON) to this file")
A = ap.parse_args()
sys.path.insert(0, os.path.abspath(A.root))
import torch  # noqa: E402

from gnnlm_amd import ops  # noqa: E402

HBM_GBS, PRODUCTS = 8000.0, {"f32": 1, "bf16x3": 3, "bf16x6": 6, "fp16": 1}     # (bench.py's PEAK["hbm_gbs"])
PRECS = [p for p in ("f32", "bf16x3", "fp16") if p in ops.PRECISIONS]
LINES = []


def log(s):
    print(s, flush=True)
    LINES.append(s)


def timed(variants, reps):
    for _ in range(2):
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
    return {name: {"median_us": sorted(v)[len(v) // 2], "min_us": min(v)} for name, v in ts.items()}


def gemm_part(dev):
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    res = {}
    M, N, K = (8192, 256, 256) if A.small else (655360, 1024, 1024)
    src = torch.randn(M // 2, K, generator=g, device=dev)                    # merged groups: the row map reads half as many distinct rows
    W = torch.randn(N, K, generator=g, device=dev) / K ** 0.5
    rows = torch.randint(0, M // 2, (M,), generator=g, device=dev, dtype=torch.int32)
    rows[::97] = -1
    m_dev = torch.tensor([M - 1000], dtype=torch.int32, device=dev)
    out = torch.empty(M, N, device=dev)
    bias = torch.randn(N, generator=g, device=dev)
    kernels = {}
    for p in PRECS:
        from gnnlm_amd import _lib
        ops.gemm_nt(src, W, bias=bias, a_rows=rows, m_dev=m_dev, out=out, precision=p)
        torch.cuda.synchronize()
        _lib.profile_begin()
        ops.gemm_nt(src, W, bias=bias, a_rows=rows, m_dev=m_dev, out=out, precision=p)
        torch.cuda.synchronize()
        kernels[p] = {k: round(v["total_ms"], 4) for k, v in _lib.profile_end().items()}
    t = timed([(p, (lambda p=p: ops.gemm_nt(src, W, bias=bias, a_rows=rows, m_dev=m_dev, out=out, precision=p))) for p in PRECS], A.reps)
    m = M - 1000
    for p in PRECS:
        us = t[p]["median_us"]
        byts = 4.0 * (m * K + N * K + m * N)
        log(f"store  {M} x {N} x {K}, row map + device-side M, {p:7s}: median {us:9.1f} us  min {t[p]['min_us']:9.1f} us  "
            f"{PRODUCTS[p] * 2.0 * m * N * K / us / 1e6:8.1f} TFLOP/s issued  {byts / us / 1e3:7.1f} GB/s algorithmic = {byts / us / 1e3 / HBM_GBS:.3f} of HBM  kernels (ms) {kernels[p]}")
    res["store"] = {"shape": [M, N, K], "us": t, "kernels_ms": kernels}
    del src, out, rows
    torch.cuda.empty_cache()
    M, N, K = (2048, 5000, 128) if A.small else (32768, 20002, 1024)
    X = torch.randn(M, K, generator=g, device=dev)
    W = torch.randn(N, K, generator=g, device=dev) / K ** 0.5
    pick = torch.randint(0, N, (M,), generator=g, device=dev, dtype=torch.int32)
    t = timed([(p, (lambda p=p: ops.gemm_lse(X, W, pick, alpha=1.0, precision=p))) for p in PRECS], A.reps)
    for p in PRECS:
        us = t[p]["median_us"]
        byts = 4.0 * (M * K + N * K) + 8.0 * M * 2 * ((N + 127) // 128)
        log(f"LSE head {M} x {N} x {K} (+ lse_reduce), {p:7s}: median {us:9.1f} us  min {t[p]['min_us']:9.1f} us  "
            f"{PRODUCTS[p] * 2.0 * M * N * K / us / 1e6:8.1f} TFLOP/s issued  {byts / us / 1e3:7.1f} GB/s algorithmic = {byts / us / 1e3 / HBM_GBS:.3f} of HBM")
    res["lse"] = {"shape": [M, N, K], "us": t}
    return res


def step_part(dev):
    import bench
    sys.argv = [sys.argv[0], "--layers", str(A.layers), "--search", "given", "--pool", "2"] + (["--small"] if A.small else [])
    args = bench.parse()
    eng, shard, sharded, cpu_model, (d, vocab) = bench.build(args, dev, 0, 1)
    batches = bench.make_batches(args, dev, 0, d, vocab)
    n_tok = batches[0].targets.shape[0]
    precs = [p for p in ("f32", "fp16") if p in ops.PRECISIONS]

    def setp(p):
        eng.hgt.gemm_precision = eng.asm.gemm_precision = ops.PRECISIONS[p]

    def run(n):
        for i in range(n):
            eng.score(batches[i % len(batches)], args.lmbda, args.temperature)
        torch.cuda.synchronize()
    outs = {}
    for p in precs:
        setp(p)
        run(2)
        o = eng.score(batches[0], args.lmbda, args.temperature)
        outs[p] = {k: o[k].double().clone() for k in ("lm_logp", "logp")}
    times = {p: [] for p in precs}
    for _ in range(A.rounds):
        for p in precs:
            setp(p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(A.steps)
            times[p].append((time.perf_counter() - t0) / A.steps)
    res = {"layers": A.layers, "tokens": n_tok, "s_per_step": times}
    for p in precs:
        med = sorted(times[p])[len(times[p]) // 2]
        res[p + "_tokens_per_s"] = n_tok / med
        log(f"step, L = {A.layers}, {n_tok} tokens, search given, {p:5s}: median {med * 1e3:9.3f} ms per step = {n_tok / med:10.0f} tokens/s  ({[round(t * 1e3, 3) for t in times[p]]})")
    if "fp16" in outs:
        for k in ("lm_logp", "logp"):
            dl = outs["fp16"][k] - outs["f32"][k]
            res["dlogp_" + k] = [float(dl.abs().max()), float((dl * dl).mean().sqrt())]
            log(f"accuracy, L = {A.layers}, {k:8s} fp16 - f32 on one batch of {n_tok} tokens: max |d| = {dl.abs().max().item():.3e}  RMS = {(dl * dl).mean().sqrt().item():.3e}")
        log(f"step, L = {A.layers}: fp16 / f32 tokens/s = {res['fp16_tokens_per_s'] / res['f32_tokens_per_s']:.3f}")
    return res


def main():
    dev = torch.device("cuda:0")
    log(f"# fp16_bench --part {A.part}" + (f" --layers {A.layers}" if A.part == "step" else "") + f"  (tree: {os.path.basename(os.path.abspath(A.root))}, precisions: {PRECS})")
    res = gemm_part(dev) if A.part == "gemm" else step_part(dev)
    if A.out:
        os.makedirs(os.path.dirname(os.path.abspath(A.out)), exist_ok=True)
        with open(A.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n" + json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
