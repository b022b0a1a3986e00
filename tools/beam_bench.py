#!/usr/bin/env python3
"""One beam-search step of the base LM at the shape of adaptive_lm_wiki103 (16 layers, d = 1024, H = 8 so d_k = 128, ffn = 4096)
against what a transcription of the reference's beam search would do on the same cache.

    python tools/beam_bench.py [--steps 20 --warmup 3] [--beams 5,16] [--batches 1,8] [--lengths 512,3072] [--groups 4 --strength 0.5]

For every (beam, B, prompt length) it reports (device events, the median of --steps rounds after --warmup, the timed forms taking
turns -- the protocol of tools/generate_bench.py):
  * beam step            ``ops.beam_select`` + ``TransformerLM.step(src=table)`` for the B * beam hypotheses, eager; and the same pair
                         captured once in a HIP graph and replayed.  No output layer and no top-k (tools/dense_head_bench.py's subjects).
  * attention, table     ``gnnlm_beam_attn`` alone, one layer per call and the 16 layers in turn, on the cache the steps left: the
                         prompt's rows held once per sentence (slot b * beam), the generated rows wherever their hypothesis wrote them.
  * attention, plain     ``gnnlm_decode_attn`` on the same memory with the same lengths: every hypothesis reads its own slot, i.e. beam
                         copies of the prompt -- what the attention costs after the reference's reorder.
  * reorder              the index-select of one layer's K and V rows [0, len) by parent: ``reorder_incremental_state``, the copy the
                         table replaces.
  * select               ``gnnlm_beam_select`` alone (2 * beam candidates per hypothesis), the table update included.
  * select, diverse      (``--groups`` G > 1) ``gnnlm_beam_select_diverse`` with G groups on the same buffers, taking turns with the plain
                         select; the candidates' tokens are then drawn from 4 * beam ids per sentence, so that the groups' rows share tokens
                         and the penalty reorders them (the plain select's work does not depend on the ids).
Beside the attention times: the bytes each must move over the achievable HBM rate.  The plain attention reads 2 * B * beam * len * d * 4
per layer; the table one reads the same rows but only 2 * (B * prompt + B * beam * generated) * d * 4 of them are distinct, the rest
hits in cache.  Seeded synthetic weights, cache contents and candidates (none of them eos: no sentence ends).  One JSON line per case."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from generate_bench import HBM_RATE, build, median_ms  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--beams", default="5,16")
    p.add_argument("--batches", default="1,8")
    p.add_argument("--lengths", default="512,3072")
    p.add_argument("--layers", type=int, default=16)
    p.add_argument("--d", type=int, default=1024)
    p.add_argument("--heads", type=int, default=8)
    p.add_argument("--ffn", type=int, default=4096)
    p.add_argument("--vocab", type=int, default=267744)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--groups", type=int, default=1, help="> 1: also time gnnlm_beam_select_diverse with this many groups")
    p.add_argument("--strength", type=float, default=0.5)
    A = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_bench needs the GPU: a timing taken elsewhere says nothing about it")
    from gnnlm_amd import _lib, ops
    from gnnlm_amd.beam_search import BeamState
    dev = torch.device("cuda:0")
    lm = build(A, dev)
    d, L, H = A.d, A.layers, A.heads
    rounds = A.steps + A.warmup
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    for beam in [int(v) for v in A.beams.split(",")]:
        for n in [int(v) for v in A.lengths.split(",")]:
            for B in [int(v) for v in A.batches.split(",")]:
                S, N = B * beam, 2 * beam
                cap = n + 2 * rounds + 8
                cache = lm.new_cache(S, cap)
                cache.k.normal_(generator=g).mul_(0.3)
                cache.v.normal_(generator=g)
                cache.len.fill_(n)
                state = BeamState(B, beam, 8 * rounds + 16, cache.len, cache.done, dev)
                table = torch.zeros(S, cap, dtype=torch.int32, device=dev)
                # sorted candidates, none of them eos, redrawn never: the selection's work does not depend on their values
                cv = -torch.sort(torch.rand(S, N, device=dev, generator=g), dim=1).values
                pool = A.vocab - 4 if A.groups <= 1 else 2 * N
                ci = torch.stack([torch.randperm(pool, device=dev, generator=g)[:N] + 4 for _ in range(S)])

                def pair():
                    ops.beam_select(cv, ci, state, src=table)
                    lm.step(state.next, cache, want_inner=False, want_ffn_input=False, max_len=cap, src=table)

                ops.beam_select(cv[:B].contiguous(), ci[:B].contiguous(), state, src=table)          # the first step: beam_in = 1
                lm.step(state.next, cache, want_inner=False, want_ffn_input=False, max_len=cap, src=table)
                (t_step,), spread = median_ms([pair], A.steps, A.warmup)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    pair()                                                                           # this stream's workspace
                    side.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=side):
                        pair()
                    (t_graph,), _ = median_ms([graph.replay], A.steps, A.warmup)
                    side.synchronize()
                torch.cuda.current_stream().wait_stream(side)
                del graph
                now = int(cache.len[0].item())                                                     # prompt + the steps taken
                assert now == n + 2 * rounds + 2 and int(cache.n_bad.item()) == 0 and int(state.finished.sum().item()) == 0
                len_attn = torch.full((S,), now, dtype=torch.int32, device=dev)
                qkv = 0.3 * torch.randn(S, 3 * d, device=dev, generator=g)
                out = torch.empty(S, d, device=dev)
                ws = torch.empty(max(16, _lib.lib().gnnlm_decode_attn_workspace_bytes(S, H, d // H, now + 1)), dtype=torch.uint8, device=dev)
                parent = state.parent.long()
                bufk, bufv = torch.empty(S, now, d, device=dev), torch.empty(S, now, d, device=dev)
                turn = [0, 0, 0]

                def attn_table():
                    ops.beam_attn(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], cache.k, cache.v, len_attn, table, turn[0] % L, H, out=out,
                                  workspace=ws, max_len=now + 1)
                    turn[0] += 1

                def attn_plain():
                    ops.decode_attn(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], cache.k, cache.v, len_attn, turn[1] % L, H, out=out,
                                    workspace=ws, max_len=now + 1)
                    turn[1] += 1

                def reorder():
                    l = turn[2] % L
                    torch.index_select(cache.k[l, :, :now], 0, parent, out=bufk)
                    torch.index_select(cache.v[l, :, :now], 0, parent, out=bufv)
                    turn[2] += 1

                def select():
                    ops.beam_select(cv, ci, state, src=table)

                (t_tab, t_plain, t_reorder), spread2 = median_ms([attn_table, attn_plain, reorder], A.steps, A.warmup)
                kern = []
                for fn in (attn_table, attn_plain):                                                # the launches alone, the library's own events
                    _lib.profile_begin(1 << 4)
                    for _ in range(2 * L):
                        fn()
                    prof = list(_lib.profile_end().values())[0]
                    kern.append(prof["total_ms"] / prof["launches"])
                def select_diverse():
                    ops.beam_select_diverse(cv, ci, state, src=table, groups=A.groups, strength=A.strength)

                if A.groups > 1:
                    (t_select, t_diverse), _ = median_ms([select, select_diverse], A.steps, A.warmup)
                else:
                    (t_select,), _ = median_ms([select], A.steps, A.warmup)
                assert int(cache.n_bad.item()) == 0
                gen = now - n
                plain_bytes = 2 * S * now * d * 4
                distinct = 2 * (B * n + S * gen) * d * 4
                reorder_bytes = 2 * plain_bytes                                                     # K and V rows read and written
                print(json.dumps({"beam": beam, "B": B, "prompt": n, "len": now, "precision": lm.precision,
                                  "beam_step_ms": round(t_step, 4), "beam_step_ms_min_max": [round(v, 4) for v in spread[0]],
                                  "beam_step_graph_replay_ms": round(t_graph, 4),
                                  "attn_table_ms_one_layer": round(t_tab, 4), "attn_table_kernels_ms": round(kern[0], 5),
                                  "attn_plain_ms_one_layer": round(t_plain, 4), "attn_plain_kernels_ms": round(kern[1], 5),
                                  "reorder_ms_one_layer": round(t_reorder, 4),
                                  "plain_plus_reorder_ms_one_layer": round(kern[1] + t_reorder, 4),
                                  "table_over_plain_plus_reorder": round(kern[0] / (kern[1] + t_reorder), 3),
                                  "attn_plain_bytes_one_layer": plain_bytes, "attn_table_distinct_bytes_one_layer": distinct,
                                  "attn_table_index_bytes_one_layer": 4 * S * now * H, "reorder_bytes_one_layer": reorder_bytes,
                                  "attn_plain_floor_ms": round(plain_bytes / HBM_RATE * 1e3, 5),
                                  "attn_table_floor_ms": round(distinct / HBM_RATE * 1e3, 5),
                                  "reorder_floor_ms": round(reorder_bytes / HBM_RATE * 1e3, 5),
                                  "select_ms": round(t_select, 4),
                                  **({"groups": A.groups, "select_diverse_ms": round(t_diverse, 4),
                                      "select_diverse_share_of_graph_step": round(t_diverse / t_graph, 4)} if A.groups > 1 else {})}), flush=True)
                del cache, ws, bufk, bufv, table, state
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
