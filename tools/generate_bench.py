#!/usr/bin/env python3
"""One decoding step of the base LM at the shape of adaptive_lm_wiki103 (16 layers, d = 1024, H = 8 so d_k = 128, ffn = 4096; the
embedding table has V = 267,744 rows) against what the build could do before it had a K/V cache.

    python tools/generate_bench.py [--steps 30 --warmup 5] [--batches 1,8,32] [--lengths 512,3072]
    python tools/generate_bench.py --pick [--steps 30 --warmup 5] [--batches 1,8,32,128] [--out profiles/FILE.txt]

For every (B, cached length) it reports, each named for what it is (device events, the median of --steps rounds after --warmup, the
timed forms taking turns):
  * step        ``TransformerLM.step`` for B sequences: embed, 16 x (LayerNorm, q|k|v GEMM, gnnlm_decode_attn, out-projection,
                LayerNorm, fc1, activation, fc2), len += 1.  No output layer (tools/dense_head_bench.py's subject).
  * step, replayed   the same step captured once in a HIP graph and replayed: what is left when the host enqueues nothing; and the
                step's kernels by the library's event profiler.
  * attention   ``gnnlm_decode_attn`` alone, one layer per call and the 16 layers in turn (16 layers of K + V are far beyond the
                Infinity Cache at every size but the smallest, so the rate is an HBM rate), on the same cache: the call (host
                included), and its two launches bracketed by the library's own events.
  * forward     ``extract_features`` over ONE sample of length + 1 tokens: the only way to the next token's features without a cache
                (B sequences cost B of them, or one packed batch of B samples).
Beside the attention time: the bytes it must move, 2 * B * len * d * 4 per layer, over the achievable HBM rate (6.3 TB/s) = the least
time, and the share of that rate reached.  Beside the step: the same with the weights (16 x (4 d^2 + 2 d ffn) x 4 bytes) added.
Seeded synthetic weights and cache contents.  One JSON line per (B, length).

``--pick`` times the per-token pick instead, on rows [B, V] at V = 267,744 with two profiles -- "peaked": the softmax of Zipf-like logits
(-1.1 log rank, the ranks permuted per row); "flat": the softmax of unit normal logits, whose nucleus at 0.9 is tens of thousands of
entries -- the same method, the forms taking turns:
  * head        ``head.log_probs`` of B rows under the adaptive softmax at the WikiText-103 shape (cutoffs 20000 / 60000, d = 1024)
  * top-k pick  the existing pick: ``gnnlm_topk_merge`` at k = 10 plus ``gnnlm_sample_topk``
  * top-p 0.9   ``gnnlm_sample_topp`` at p = 0.9
  * top-p inf   ``gnnlm_sample_topp`` at p = inf (the whole vocabulary: no refinement sweeps)
and beside each top-p time the row bytes (B * V * 4) over it, next to the achievable HBM rate (6.3 TB/s) and the L2 rate (34.5 TB/s)
of the chip.  The condition of the run: at every B the top-p pick costs no more than the head of the same rows."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_RATE = 6.3e12                # bytes / s, achievable


def median_ms(fns, steps, warmup):
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


def build(A, dev):
    from gnnlm_amd.token_embed import TokenEmbedding
    from gnnlm_amd.transformer_lm import TransformerLM, sinusoidal_table
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    d, ffn = A.d, A.ffn
    layers = []
    for _ in range(A.layers):
        layers.append({"ln1_g": 1 + 0.1 * r(d), "ln1_b": 0.1 * r(d), "wqkv": r(3 * d, d) / d ** 0.5, "bqkv": 0.1 * r(3 * d),
                       "wo": r(d, d) / d ** 0.5, "bo": 0.1 * r(d), "ln2_g": 1 + 0.1 * r(d), "ln2_b": 0.1 * r(d),
                       "w1": r(ffn, d) / d ** 0.5, "b1": 0.1 * r(ffn), "w2": r(d, ffn) / ffn ** 0.5, "b2": 0.1 * r(d)})
    E = TokenEmbedding(r(A.vocab, d) / d ** 0.5, "plain")
    # the table a loaded checkpoint starts with (max_target_positions = 1024); new_cache grows it to what a cache holds
    return TransformerLM(E, layers, A.heads, act="relu", pos=sinusoidal_table(1026, d), learned_pos=False, ln_out=(1 + 0.1 * r(d), 0.1 * r(d)),
                         device=dev, precision="fp16" if A.fp16 else None)


def pick_bench(A, dev):
    from gnnlm_amd import ops
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    cutoff, d, V = (20000, 60000, A.vocab), A.d, A.vocab
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev)
    emb, proj, prev = [], [], 0
    for i, c in enumerate(cutoff):
        dim = d // 4 ** i
        emb.append(rnd(c - prev, dim) * dim ** -0.5)
        proj.append(None if i == 0 else rnd(d, dim) * d ** -0.5)
        prev = c
    head = AdaptiveSoftmax(list(cutoff), emb, proj, rnd(len(cutoff) - 1, d) * d ** -0.5, dev)
    batches = [int(v) for v in A.batches.split(",")]
    Bmax = max(batches)
    zipf = -1.1 * torch.log(torch.arange(1, V + 1, device=dev, dtype=torch.float32))
    rows = {"peaked": torch.log_softmax(torch.stack([zipf[torch.randperm(V, generator=g, device=dev)] for _ in range(Bmax)]), dim=1),
            "flat": torch.log_softmax(rnd(Bmax, V), dim=1)}
    x = rnd(Bmax, d)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"the pick of one decoding step, rows [B, {V}]; device events, median of {A.steps} after {A.warmup}, the forms taking turns; us")
    log(f"{'profile':>7} {'B':>4} | {'head':>9} | {'top-k pick':>10} | {'top-p 0.9':>9} {'TB/s':>6} {'mean n':>8} | {'top-p inf':>9} {'TB/s':>6} | "
        f"{'top-p <= head':>13}")
    ok = True
    for name, R in rows.items():
        for B in batches:
            lp, xb = R[:B], x[:B]
            out = torch.empty(B, V, device=dev)
            bv, bi = torch.empty(B, 10, device=dev), torch.empty(B, 10, dtype=torch.int64, device=dev)
            u = torch.rand(B, generator=g, device=dev)
            nxt, nlp = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, device=dev)
            n_keep = torch.zeros(B, dtype=torch.int32, device=dev)

            def f_head():
                head.log_probs(xb, out=out)

            def f_topk():
                ops.topk_merge(lp, bv, bi, init=True)
                ops.sample_topk(bv, bi, u=u, out=nxt, out_logp=nlp)

            def f_p09():
                ops.sample_topp(lp, 0.9, u, out=nxt, out_logp=nlp, n_keep=n_keep)

            def f_pinf():
                ops.sample_topp(lp, float("inf"), u, out=nxt, out_logp=nlp)

            (t_head, t_topk, t_p09, t_pinf), _ = median_ms([f_head, f_topk, f_p09, f_pinf], A.steps, A.warmup)
            f_p09()
            mean_n = float(n_keep.float().mean())
            rate = lambda ms: B * V * 4 / (ms * 1e-3) / 1e12
            good = max(t_p09, t_pinf) <= t_head
            ok = ok and good
            log(f"{name:>7} {B:>4} | {t_head * 1e3:>9.1f} | {t_topk * 1e3:>10.1f} | {t_p09 * 1e3:>9.1f} {rate(t_p09):>6.3f} {mean_n:>8.0f} | "
                f"{t_pinf * 1e3:>9.1f} {rate(t_pinf):>6.3f} | {'yes' if good else 'NO':>13}")
            print(json.dumps({"pick": name, "B": B, "V": V, "head_us": round(t_head * 1e3, 1), "topk_pick_us": round(t_topk * 1e3, 1),
                              "topp09_us": round(t_p09 * 1e3, 1), "topp_inf_us": round(t_pinf * 1e3, 1), "mean_nucleus": mean_n,
                              "topp09_row_TBps": round(rate(t_p09), 4), "topp_inf_row_TBps": round(rate(t_pinf), 4),
                              "topp_le_head": bool(good)}), flush=True)
    log(f"row bytes / pick time above; for scale: achievable HBM rate {HBM_RATE / 1e12} TB/s, L2 34.5 TB/s (chip-wide; one workgroup per row "
        "uses one CU of 256).  " + ("At every B the top-p pick costs no more than the head." if ok else "THE TOP-P PICK COSTS MORE THAN THE HEAD SOMEWHERE."))
    if A.out:
        with open(A.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batches", default="1,8,32")
    p.add_argument("--lengths", default="512,3072")
    p.add_argument("--layers", type=int, default=16)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--ffn", type=int, default=4096)
    p.add_argument("--vocab", type=int, default=267744)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--pick", action="store_true", help="time the per-token pick (head, top-k pick, top-p pick) instead of the step")
    p.add_argument("--out", default=None, help="--pick: also write the table to this file")
    A = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("generate_bench needs the GPU: a timing taken elsewhere says nothing about it")
    if A.pick:
        if A.batches == "1,8,32":
            A.batches = "1,8,32,128"
        return pick_bench(A, torch.device("cuda:0"))
    from gnnlm_amd import _lib, ops
    dev = torch.device("cuda:0")
    lm = build(A, dev)
    d, L, H = A.d, A.layers, A.heads
    rounds = A.steps + A.warmup
    weight_bytes = L * (4 * d * d + 2 * d * A.ffn) * 4
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    for n in [int(v) for v in A.lengths.split(",")]:
        sample = torch.randint(4, A.vocab, (n + 1,), device=dev, generator=g)
        for B in [int(v) for v in A.batches.split(",")]:
            cache = lm.new_cache(B, n + rounds + 2)
            cache.k.normal_(generator=g).mul_(0.3)
            cache.v.normal_(generator=g)
            cache.len.fill_(n)
            cache.steps = n
            tok = torch.randint(4, A.vocab, (B,), device=dev, generator=g)
            qkv = 0.3 * torch.randn(B, 3 * d, device=dev, generator=g)
            out = torch.empty(B, d, device=dev)
            ws = torch.empty(max(16, _lib.lib().gnnlm_decode_attn_workspace_bytes(B, H, d // H, n + 1)), dtype=torch.uint8, device=dev)
            turn = [0]
            len_attn = torch.full((B,), n, dtype=torch.int32, device=dev)

            def step():
                lm.step(tok, cache, want_inner=False, want_ffn_input=False)

            def attention():
                # a layer per call, in turn: L layers of K + V are far more than the Infinity Cache holds, one layer's may not be
                ops.decode_attn(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], cache.k, cache.v, len_attn, turn[0] % L, H, out=out, workspace=ws,
                                max_len=n + 1)
                turn[0] += 1

            def forward():
                lm.extract_features(sample, [0, n + 1], want_inner=False, want_ffn_input=False, check=False)

            (t_step, t_attn, t_fwd), spread = median_ms([step, attention, forward], A.steps, A.warmup)
            # the two launches of the attention alone, bracketed by the library's own events (a run of its own: no host time in it)
            _lib.profile_begin(1 << 4)
            for _ in range(2 * L):
                attention()
            prof = list(_lib.profile_end().values())[0]
            t_kern = prof["total_ms"] / prof["launches"]
            assert abs(prof["bytes"] / prof["launches"] / (2 * B * (n + 1) * d * 4) - 1) < 0.05      # the profiler books the keys held
            # the kernels of one step, same profiler (every launch bracketed: the sum has no gaps between kernels in it)
            _lib.profile_begin()
            step()
            split = {k: round(v["total_ms"], 4) for k, v in _lib.profile_end().items()}
            # the same step captured once and replayed: what is left when the host enqueues nothing
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            bound = n + 3 * rounds
            with torch.cuda.stream(side):
                gcache = lm.new_cache(B, bound)
                gcache.k.normal_(generator=g).mul_(0.3)
                gcache.v.normal_(generator=g)
                gcache.len.fill_(n)
                lm.step(tok, gcache, want_inner=False, want_ffn_input=False, max_len=bound)      # this stream's workspace
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    lm.step(tok, gcache, want_inner=False, want_ffn_input=False, max_len=bound)
                (t_graph,), _ = median_ms([graph.replay], A.steps, A.warmup)
                side.synchronize()
            torch.cuda.current_stream().wait_stream(side)
            del graph, gcache
            kv_layer = 2 * B * n * d * 4
            floor_attn = kv_layer / HBM_RATE * 1e3
            floor_step = (weight_bytes + L * kv_layer) / HBM_RATE * 1e3
            print(json.dumps({"B": B, "len": n, "precision": lm.precision,
                              "step_ms": round(t_step, 4), "step_ms_min_max": [round(v, 4) for v in spread[0]],
                              "step_graph_replay_ms": round(t_graph, 4), "step_kernels_ms": split,
                              "step_bytes": weight_bytes + L * kv_layer, "step_floor_ms": round(floor_step, 4),
                              "step_share_of_hbm_rate": round(floor_step / t_step, 3),
                              "attn_ms_one_layer": round(t_attn, 4), "attn_ms_min_max": [round(v, 4) for v in spread[1]],
                              "attn_bytes_one_layer": kv_layer, "attn_floor_ms": round(floor_attn, 5),
                              "attn_kernels_ms": round(t_kern, 5), "attn_share_of_hbm_rate": round(floor_attn / t_kern, 3),
                              "forward_ms_one_sample": round(t_fwd, 3), "forward_over_step": round(t_fwd / t_step, 1),
                              "final_len": int(cache.len[0].item())}), flush=True)
            del cache, ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
