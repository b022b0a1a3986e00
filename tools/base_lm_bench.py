#!/usr/bin/env python3
"""Base transformer LM forward at the shape of the "save features" loop (gnnlm_scripts/wiki103/prepare_wiki103.sh:69-78):
16 layers, d = 1024, H = 8, ffn = 4096, one sample of 3072 rows per batch of which --context-window 2560 are context -- 512 scored.

    python tools/base_lm_bench.py [--steps 20 --warmup 3] > profiles/r17_base_lm_bench.txt

Reports, each named for what it is:
  * tokens/s computed and scored: device events around `steps` forwards, profiler off;
  * the per-kernel split of one forward from the library's event profiler (a run of its own: bracketing every launch with
    events serialises the stream), with the algorithmic FLOP of the GEMMs over their kernel time against the f32-MFMA peak
    read from the device (compute units x 4 SIMDs x 64 FLOP/clk x the reported clock);
  * the error of one sample against the float64 restatement (tests/transformer_lm_ref.py), max|dev - ref64| / max|ref64|;
  * the baseline: the float32 torch-CPU evaluation of that restatement, timed in the same run.
Seeded synthetic weights; no output layer (the head's cost is tools/dense_head_bench.py's subject).

    python tools/base_lm_bench.py --no-reference --knnlm > profiles/r18_base_knnlm_bench.txt

adds the kNN-LM leg (``knnlm_leg``): forward, pack, search, head, interpolation and the whole batch at --max-tokens
3072 and 36000 over a synthetic IVF-PQ index of --knn-keys keys (a plain tied output layer stands in for the head); the driver with
and without --knnlm; gnnlm_pack_rows against the torch form it replaces at 1, 11 and 256 samples per batch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import transformer_lm_ref as tr  # noqa: E402


def device_clock_hz(props, index):
    """The device's peak engine clock as the runtime reports it: torch's property where it has one, else hipDeviceGetAttribute
    (hipDeviceAttributeClockRate = 5, kHz) on the HIP runtime this process already runs on."""
    khz = getattr(props, "clock_rate", 0)
    if not khz:
        import ctypes
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                hip = ctypes.CDLL(name)
            except OSError:
                continue
            v = ctypes.c_int(0)
            if hip.hipDeviceGetAttribute(ctypes.byref(v), 5, index) == 0:
                khz = v.value
            break
    return float(khz) * 1e3


def median_ms(fns, steps, warmup):
    """Device-event time of every callable of ``fns``, the callables taking turns (one round = each of them once, so that clock and
    cache state are shared): ``warmup`` rounds, then the median of ``steps`` rounds each, in ms."""
    times = [[] for _ in fns]
    for r in range(warmup + steps):
        for j, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warmup:
                times[j].append(e0.elapsed_time(e1))
    return [float(np.median(t)) for t in times], [(float(min(t)), float(max(t))) for t in times]


class SyntheticKnn:
    """The ``KNNModel`` the driver talks to, over a shape-true synthetic IVF-PQ index with labels attached (no files)."""

    def __new__(cls, index, vals, k, d, dev):
        from gnnlm_amd.knn_model import KNNModel
        m = KNNModel.__new__(KNNModel)
        m.index, m.k, m.metric_type, m.index_file = index, k, "do_not_recomp_ip", "synthetic.cosine"
        m.dstore_size, m.hidden_size, m.device, m._vals_dev, m.data_store = int(vals.shape[0]), d, dev, vals, None
        index.attach_vals(vals)
        return m


def knnlm_leg(A, model, m, dev):
    """--knnlm: the stages of a batch of the recipe's shape (forward, pack, search, interpolation) and the whole batch through the
    driver with and without --knnlm, at --max-tokens = one sample and 36000; then gnnlm_pack_rows against the torch form it
    replaces.  Device events, the median of --steps rounds after --warmup, the compared forms taking turns."""
    import tempfile
    from gnnlm_amd import eval_base_lm, ops
    from gnnlm_amd.dense_softmax import DenseSoftmax
    from gnnlm_amd.eval_lm import get_parser
    from gnnlm_amd.ragged import BlockTable
    from gnnlm_amd.synthetic import synthetic_ivfpq_index
    n, d, ctx = A.sample, A.d, A.context
    scored = n - ctx
    model.head = DenseSoftmax(torch.from_numpy(m["E"]), None, dev)
    t0 = time.perf_counter()
    index = synthetic_ivfpq_index(A.knn_keys, d, A.nlist, 64, dev, nprobe=A.nprobe)
    vals = torch.randint(4, A.vocab, (A.knn_keys,), device=dev, dtype=torch.int32)
    knn = SyntheticKnn(index, vals, A.k, d, dev)
    torch.cuda.synchronize()
    print(f"\n--knnlm leg: synthetic IVF-PQ index of {A.knn_keys:,} keys ({A.nlist} lists, PQ64, nprobe {A.nprobe}, k = {A.k}), built in "
          f"{time.perf_counter() - t0:.1f} s; cosine (unit queries from gnnlm_pack_rows); do_not_recomp_ip")
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    for max_tokens in (n, 36000):
        ns = max(1, max_tokens // n)
        rb = BlockTable([n] * ns, dev).batch(0)
        tokens = torch.randint(0, A.vocab, (ns * n,), device=dev, generator=gen)
        skip = torch.full((ns,), ctx, device=dev, dtype=torch.int32)
        out_off = (torch.arange(ns + 1, device=dev, dtype=torch.int32) * scored).contiguous()
        target = torch.randint(4, A.vocab, (ns * scored,), device=dev, generator=gen)
        state = {}

        def forward():
            state["x"], state["extra"] = model.extract_features(tokens, rb, want_inner=True, want_ffn_input=False, check=False)

        def pack():
            state["q"] = ops.pack_rows(state["extra"]["inner_states"][-1], rb.block_off, skip, out_off, d, want_rows=False, want_unit=True,
                                       n_bad=bad, out=(None, qbuf))[1]

        def search():
            state["found"] = knn.search_finish(knn.interpolate_begin(state["q"], unit=True))

        def head():
            state["lm"] = torch.cat([model.target_logp(state["x"][j * n + ctx:(j + 1) * n], target[j * scored:(j + 1) * scored]) for j in range(ns)])

        def interp():
            knn.interpolate_finish(state["found"], target, state["lm"], 1.0, 0.25)

        bad = torch.zeros(1, device=dev, dtype=torch.int32)
        qbuf = torch.empty(ns * scored, d, device=dev)

        def batch():
            forward(), pack()
            pending = knn.interpolate_begin(state["q"], unit=True)
            head()
            knn.interpolate_finish(pending, target, state["lm"], 1.0, 0.25)

        med, span = median_ms([forward, pack, search, head, interp, batch], A.steps, A.warmup)
        print(f"  --max-tokens {max_tokens}: {ns} sample(s) of {n} rows, {ns * scored} scored (= searched; the reference searches all {ns * n})")
        for name, v, (lo, hi) in zip(("forward", "pack (unit rows)", "search", "head (target log-probs)", "interpolation", "whole batch"), med, span):
            print(f"    {name:26s} {v:9.3f} ms   (min {lo:.3f}, max {hi:.3f})")
        print(f"    tokens/s scored: {ns * scored / med[5] * 1e3:,.0f} with kNN; forward + head alone {ns * scored / (med[0] + med[3]) * 1e3:,.0f}")
    # ---- the driver itself, with and without --knnlm, over a synthetic split of 22 samples
    with tempfile.TemporaryDirectory() as td:
        n_tok = 22 * scored
        # DATA/test.bin/.idx in fairseq's mmap format: one sentence of n_tok int32 tokens
        import struct
        with open(os.path.join(td, "test.idx"), "wb") as f:
            f.write(b"MMIDIDX\x00\x00" + struct.pack("<Q", 1) + struct.pack("<B", 4) + struct.pack("<Q", 1))
            f.write(np.asarray([n_tok], np.int32).tobytes() + np.asarray([0], np.int64).tobytes())
        np.random.RandomState(4).randint(4, A.vocab, size=n_tok).astype(np.int32).tofile(os.path.join(td, "test.bin"))
        for max_tokens in (n, 36000):
            for with_knn in (False, True):
                args = get_parser().parse_args([td, "--path", "-", "--gen-subset", "test", "--sample-break-mode", "none", "--tokens-per-sample", str(n),
                                                "--context-window", str(ctx), "--max-tokens", str(max_tokens), "--softmax-batch", "1024"] +
                                               (["--knnlm", "--k", str(A.k), "--lmbda", "0.25", "--probe", str(A.nprobe)] if with_knn else []))
                args.knn_model = knn if with_knn else None
                import contextlib
                import io
                runs = []
                with contextlib.redirect_stdout(io.StringIO()):
                    for _ in range(1 + 3):
                        runs.append(eval_base_lm.main(args, model=model))
                r = sorted(runs[1:], key=lambda r_: r_["seconds"])[1]
                print(f"  driver, --max-tokens {max_tokens}{' --knnlm' if with_knn else ''}: {r['count']} scored of {r['tokens']} computed in {r['seconds'] * 1e3:.1f} ms "
                      f"(median of 3 after 1 warm-up, batch event timers) = {r['count'] / r['seconds']:,.0f} tokens/s scored")
    # ---- gnnlm_pack_rows against the torch form it replaces (per-sample slices + cat + the four-op normalisation)
    print("  gnnlm_pack_rows (unit rows of the scored runs) against the torch form (slices + cat, then q / (q ** 2).sum(-1, keepdims=True).sqrt()):")
    for ns in (1, 11, 256):
        feats = torch.randn(ns * n, d, device=dev, generator=gen)
        rb = BlockTable([n] * ns, dev).batch(0)
        skip = torch.full((ns,), ctx, device=dev, dtype=torch.int32)
        out_off = (torch.arange(ns + 1, device=dev, dtype=torch.int32) * scored).contiguous()
        qbuf = torch.empty(ns * scored, d, device=dev)
        bad = torch.zeros(1, device=dev, dtype=torch.int32)

        def kernel():
            ops.pack_rows(feats, rb.block_off, skip, out_off, d, want_rows=False, want_unit=True, n_bad=bad, out=(None, qbuf))

        def torch_form():
            q = torch.cat([feats[j * n + ctx:(j + 1) * n] for j in range(ns)])
            return q / (q ** 2).sum(-1, keepdims=True).sqrt()

        (tk, tt), _ = median_ms([kernel, torch_form], A.steps, A.warmup)
        moved = 2.0 * ns * scored * d * 4
        print(f"    {ns:4d} sample(s): kernel {tk * 1e3:8.1f} us ({moved / tk / 1e6:7.1f} GB/s of the {moved / 1e6:.1f} MB it must move)   "
              f"torch {tt * 1e3:8.1f} us   ratio {tt / tk:.2f}x")
        assert int(bad.item()) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--knnlm", action="store_true", help="add the kNN-LM leg (knnlm_leg)")
    ap.add_argument("--knn-keys", type=int, default=103227021, help="keys of the synthetic IVF-PQ index (WikiText-103 train: 103,227,021)")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=16)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--ffn", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=3072, help="rows per sample (--tokens-per-sample)")
    ap.add_argument("--context", type=int, default=2560, help="of which context (--context-window)")
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--no-reference", action="store_true", help="skip the float64 / float32 CPU evaluations")
    A = ap.parse_args()
    assert torch.cuda.is_available(), "base_lm_bench needs an MI355X: there is no CPU fallback"
    from gnnlm_amd import _lib
    from gnnlm_amd.ragged import BlockTable
    from gnnlm_amd.token_embed import TokenEmbedding
    from gnnlm_amd.transformer_lm import TransformerLM
    dev = torch.device("cuda:0")
    n, d, L, ffn = A.sample, A.d, A.layers, A.ffn
    m = tr.make_model(seed=17, V=A.vocab, d=d, H=A.heads, L=L, ffn=ffn, act="relu", final_norm=True, positions="sinusoidal", pos_rows=n + 2)
    layers = []
    for w in m["layers"]:
        lw = {k: torch.from_numpy(w[k]) for k in ("ln1_g", "ln1_b", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2")}
        lw["wqkv"] = torch.from_numpy(np.concatenate([w["wq"], w["wk"], w["wv"]], 0))
        lw["bqkv"] = torch.from_numpy(np.concatenate([w["bq"], w["bk"], w["bv"]], 0))
        layers.append(lw)
    pair = lambda p: (torch.from_numpy(p[0]), torch.from_numpy(p[1]))
    model = TransformerLM(TokenEmbedding(torch.from_numpy(m["E"]).to(dev), "plain"), layers, A.heads, act="relu", scale=m["scale"],
                          pos=torch.from_numpy(m["P"]), learned_pos=True, ln_out=pair(m["ln_out"]), device=dev, precision=A.precision)
    tokens_np = np.random.RandomState(18).randint(0, A.vocab, size=n).astype(np.int64)
    tokens = torch.from_numpy(tokens_np).to(dev)
    rb = BlockTable([n], dev).batch(0)
    fwd = lambda: model.extract_features(tokens, rb, want_inner=True, want_ffn_input=False, check=False)
    for _ in range(A.warmup):
        fwd()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(A.steps):
        fwd()
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) / 1e3 / A.steps
    # algorithmic work of one forward: the four GEMMs of a layer, and the causal attention (scores + P.V over the lower triangle)
    gemm_flop = L * 2.0 * n * (4.0 * d * d + 2.0 * d * ffn)
    attn_flop = L * 4.0 * d * n * (n + 1) / 2
    props = torch.cuda.get_device_properties(dev)
    clock_hz = device_clock_hz(props, dev.index or 0)
    peak = props.multi_processor_count * 4 * 64 * clock_hz if clock_hz else float("nan")
    print(f"device: {props.name}, {props.multi_processor_count} CUs, reported clock {clock_hz / 1e9:.2f} GHz -> f32-MFMA peak {peak / 1e12:.1f} TFLOP/s")
    print(f"shape: L={L} d={d} H={A.heads} ffn={ffn}, sample {n} rows = {A.context} context + {n - A.context} scored, precision {model.precision}")
    print(f"forward (device events, {A.steps} steps after {A.warmup} warm-up, profiler off): {sec * 1e3:.2f} ms per sample")
    print(f"  tokens/s computed: {n / sec:,.0f}    tokens/s scored: {(n - A.context) / sec:,.0f}")
    print(f"  whole-forward rate: {(gemm_flop + attn_flop) / sec / 1e12:.1f} TFLOP/s algorithmic ({gemm_flop / 1e12:.2f} GEMM + {attn_flop / 1e12:.2f} attention TFLOP) "
          f"= {(gemm_flop + attn_flop) / sec / peak:.1%} of the f32-MFMA peak (an end-to-end figure, not a kernel's share)")
    # ---- per-kernel split: one forward under the library's event profiler
    torch.cuda.synchronize()
    _lib.profile_begin()
    fwd()
    torch.cuda.synchronize()
    prof = _lib.profile_end()
    total = sum(v["total_ms"] for v in prof.values())
    print(f"per-kernel split of one forward (library event profiler, every launch bracketed; sum {total:.2f} ms):")
    for name, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"]):
        # (the attention launcher's own count is an estimate made for many short blocks: the lower-triangle count of this file is used)
        flops = attn_flop if name == "causal_attn_kernel" else v["flops"]
        matrix = name in ("gemm_nt_f32_kernel", "causal_attn_kernel")
        rate = f"{flops / v['total_ms'] / 1e9:8.1f} TFLOP/s" if matrix else f"{v['bytes'] / v['total_ms'] / 1e6:8.1f} GB/s  "
        print(f"  {name:28s} {v['launches']:4d} launches {v['total_ms']:9.3f} ms {v['total_ms'] / total:6.1%}  {rate}")
    g = prof.get("gemm_nt_f32_kernel")
    if g:
        print(f"  GEMMs: {g['flops'] / g['total_ms'] / 1e9:.1f} TFLOP/s over their kernel time = {g['flops'] / g['total_ms'] / 1e9 * 1e12 / peak:.1%} of the f32-MFMA peak "
              f"(compute-bound: {gemm_flop / 1e12:.2f} TFLOP over {4.0 * L * (4 * d * d + 2 * d * ffn) / 1e9:.2f} GB of weights)")
    res = {"ms_per_sample": sec * 1e3, "tokens_per_s_computed": n / sec, "tokens_per_s_scored": (n - A.context) / sec, "precision": model.precision,
           "peak_tflops": peak / 1e12, "kernels": prof}
    if not A.no_reference:
        x, extra = fwd()
        torch.cuda.synchronize()
        got = {"out": x.cpu().numpy(), "last_inner": extra["inner_states"][-1].cpu().numpy()}
        off = [0, n]
        t0 = time.perf_counter()
        ref = tr.forward(m, tokens_np, off, torch.float64)
        t64 = time.perf_counter() - t0
        t0 = time.perf_counter()
        f32 = tr.forward(m, tokens_np, off, torch.float32)
        t32 = time.perf_counter() - t0
        for key in ("out", "last_inner"):
            print(f"error of the sample, {key}: max|dev - ref64| / max|ref64| = {tr.rel_err(got[key], ref[key]):.3e}   "
                  f"(float32 torch-CPU: {tr.rel_err(f32[key], ref[key]):.3e})")
        print(f"baseline, float32 torch-CPU evaluation of the restatement ({torch.get_num_threads()} threads): {t32:.2f} s per sample = "
              f"{n / t32:,.0f} tokens/s computed -> the device forward is {t32 / sec:,.0f}x faster   (float64: {t64:.2f} s)")
        res.update({"err_out": tr.rel_err(got["out"], ref["out"]), "cpu_f32_s": t32, "cpu_f64_s": t64})
    print(json.dumps({k: v for k, v in res.items() if k != "kernels"}))
    if A.knnlm:
        knnlm_leg(A, model, m, dev)


if __name__ == "__main__":
    main()
