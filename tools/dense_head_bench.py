#!/usr/bin/env python3
"""The dense output layer's two routes against each other.

Shapes: n = 32768 rows, d in {512, 1024}, V in {205, 260, 512}, with and without bias, gemm_precision 0 (f32 MFMA) and 3 (fp16
operands): route 1 (the one-launch kernel, csrc/dense_logp.hip) against route 2 (the general route: LSE-epilogue GEMM + reduce, or
with a bias the storing GEMM + row pass).  Also V in {8192, 50000} on the general route with and without bias (d = 1024, precision 0),
so that what the bias costs there -- the logits written to memory and read back -- is a measured number.

Device events after a warm-up, seeded random operands (x ~ N(0, 1), w ~ N(0, 1) 2 / sqrt(d), bias ~ N(0, 1)); the variants of a
shape take turns inside every repetition, so clock drift and neighbours on the machine hit them alike; median and minimum are
reported.  Before timing, the two routes' results are compared (max |difference|).  The FLOP rate is 2 n V d over the median.

    python tools/dense_head_bench.py [--n 32768] [--reps 30] [--out FILE]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from gnnlm_amd.dense_softmax import DenseSoftmax


def timed(variants, reps, warm=5):
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


def problem(dev, n, d, V, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn(n, d, generator=g, device=dev)
    w = torch.randn(V, d, generator=g, device=dev) * (2.0 / math.sqrt(d))
    b = torch.randn(V, generator=g, device=dev)
    t = torch.randint(0, V, (n,), generator=g, device=dev)
    return x, w, b, t


def head(w, b, route, precision, dev):
    ds = DenseSoftmax(w, b, dev)
    ds.route, ds.gemm_precision = route, precision
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the lines and the figures (JSON) to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda:0")
    lines, rows = [], []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    n = a.n
    log(f"dense head, n = {n} rows, {a.reps} repetitions, device events; us = median (min)")
    log(f"{'d':>5} {'V':>6} {'bias':>4} {'prec':>4} | {'route 1 us':>18} {'TF/s':>6} | {'route 2 us':>18} {'TF/s':>6} | {'r1/r2':>6} | max |r1 - r2|")
    for d in (512, 1024):
        for V in (205, 260, 512):
            x, w, b, t = problem(dev, n, d, V)
            for with_bias in (False, True):
                for prec in (0, 3):
                    h1, h2 = head(w, b if with_bias else None, 1, prec, dev), head(w, b if with_bias else None, 2, prec, dev)
                    diff = float((h1.target_log_prob(x, t) - h2.target_log_prob(x, t)).abs().max())
                    r = timed([("route1", lambda: h1.target_log_prob(x, t)), ("route2", lambda: h2.target_log_prob(x, t))], a.reps)
                    fl = 2.0 * n * V * d
                    m1, m2 = r["route1"][0], r["route2"][0]
                    log(f"{d:5d} {V:6d} {'yes' if with_bias else 'no':>4} {prec:4d} | {m1:9.1f} ({r['route1'][1]:7.1f}) {fl / m1 * 1e-6:6.1f} | "
                        f"{m2:9.1f} ({r['route2'][1]:7.1f}) {fl / m2 * 1e-6:6.1f} | {m1 / m2:6.3f} | {diff:.2e}")
                    rows.append({"d": d, "V": V, "bias": with_bias, "precision": prec, "route1_us": r["route1"], "route2_us": r["route2"],
                                 "ratio": m1 / m2, "max_abs_diff": diff})
                    del h1, h2
            del x, w, b, t
            torch.cuda.empty_cache()
    log("")
    log("general route only, d = 1024, precision 0: what the bias (logits through memory, 64 MiB chunks) costs")
    log(f"{'V':>6} | {'no bias us':>18} {'TF/s':>6} | {'bias us':>18} {'TF/s':>6} | {'bias/no bias':>12} | logits bytes per call")
    d = 1024
    for V in (8192, 50000):
        x, w, b, t = problem(dev, n, d, V)
        h0, hb = head(w, None, 2, 0, dev), head(w, b, 2, 0, dev)
        r = timed([("nobias", lambda: h0.target_log_prob(x, t)), ("bias", lambda: hb.target_log_prob(x, t))], max(5, a.reps // 3), warm=2)
        fl = 2.0 * n * V * d
        m0, mb = r["nobias"][0], r["bias"][0]
        log(f"{V:6d} | {m0:9.1f} ({r['nobias'][1]:7.1f}) {fl / m0 * 1e-6:6.1f} | {mb:9.1f} ({r['bias'][1]:7.1f}) {fl / mb * 1e-6:6.1f} | {mb / m0:12.3f} | "
            f"{4.0 * n * ((V + 3) // 4 * 4) / 2 ** 20:.0f} MiB written + read")
        rows.append({"d": d, "V": V, "general_nobias_us": r["nobias"], "general_bias_us": r["bias"], "ratio": mb / m0})
        del h0, hb, x, w, b, t
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n" + json.dumps(rows) + "\n")


if __name__ == "__main__":
    main()
