#!/usr/bin/env python3
"""A/B of the IVF-PQ add phase at the shape a user runs (d = 1024, M = 64, nlist = 4096, chunks of 262144 rows):

  (a) the add loop as ``ivfpq_train.build_arrays`` had it before ``add_rows``: torch matmuls for the rotation and the coarse scores,
      argmax, the residual materialised, ``gnnlm_pq_encode`` (one wave per row), ``torch.sort`` + a gather at the end -- kept HERE
      as the old side of the comparison;
  (b) ``ivfpq_train.add_rows``'s stages: ``gnnlm_gemm_nt`` twice, the search's probe selection at one probe,
      ``gnnlm_ivfpq_encode_rows``, one placement and one ``gnnlm_ivfpq_list_merge``.

One process, seeded inputs generated on the device, both paths warmed, then the two alternate; device events around every stage with
one synchronise per repeat.  Reports median and spread (min .. max) of keys/s and of the per-stage milliseconds, the encode kernel's
achieved FLOP/s against the bound it sits under (computed from the shapes), and checks that both paths file the same keys with
the same codes wherever their assignments agree (bit for bit once both encoders read the same rotated rows).  The index's values are random (the time of neither path depends on them)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnnlm_amd import _lib, ops  # noqa: E402

F32_PEAK = 157.3e12                      # FLOP/s, vector = matrix f32 rate of the MI355X
LDS_PEAK = 256 * 256 * 2.4e9             # B/s: 256 CUs x 256 B/clk at 2.4 GHz


class Stages:
    """device events around named stages, summed per repeat"""

    def __init__(self):
        self.pairs = []

    def __call__(self, name, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.pairs.append((name, a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        t = {}
        for name, a, b in self.pairs:
            t[name] = t.get(name, 0.0) + a.elapsed_time(b)
        return t


def normalise(x):
    return x / (x ** 2).sum(1, keepdim=True).sqrt()


def old_path(keys, R, coarse, pq, norm2, chunk, st):
    N, M, dsub = keys.shape[0], pq.shape[0], pq.shape[2]
    assign = torch.empty(N, dtype=torch.int64, device=keys.device)
    codes = torch.empty(N, M, dtype=torch.uint8, device=keys.device)
    for s in range(0, N, chunk):
        x = st("normalise", lambda: normalise(keys[s:s + chunk]))
        xr = st("rotate", lambda: x @ R.t())
        a = st("coarse+assign", lambda: (xr @ coarse.t()).argmax(1))
        assign[s:s + chunk] = a
        r = st("residual", lambda: (xr - coarse[a]).contiguous())
        st("encode", lambda: _lib.call("gnnlm_pq_encode", _lib.ptr(r), r.stride(0), _lib.ptr(pq), _lib.ptr(norm2), M, dsub, r.shape[0],
                                       _lib.ptr(codes[s:s + chunk]), _lib.stream()))

    def file():
        order = torch.sort(assign, stable=True).indices
        off = torch.zeros(coarse.shape[0] + 1, dtype=torch.int64, device=keys.device)
        off[1:] = torch.cumsum(torch.bincount(assign, minlength=coarse.shape[0]), 0)
        return off, order.contiguous(), codes[order].contiguous()
    return (assign, codes) + st("file", file)


def new_path(keys, R, coarse, pq, norm2, chunk, st, empty, ids):
    N, M = keys.shape[0], pq.shape[0]
    assign = torch.empty(N, dtype=torch.int64, device=keys.device)
    codes = torch.empty(N, M, dtype=torch.uint8, device=keys.device)
    for s in range(0, N, chunk):
        x = st("normalise", lambda: normalise(keys[s:s + chunk]))
        xr = st("rotate", lambda: ops.gemm_nt(x, R))
        cs = st("coarse", lambda: ops.gemm_nt(xr, coarse))
        a = assign[s:s + chunk]

        def pick():
            pv = torch.empty(xr.shape[0], 1, dtype=torch.float32, device=keys.device)
            pi = torch.empty(xr.shape[0], 1, dtype=torch.int64, device=keys.device)
            ops.ivfpq_select_probes(cs, pv, pi)
            a.copy_(pi[:, 0])
        st("assign", pick)
        st("encode", lambda: ops.ivfpq_encode_rows(xr, a, coarse, pq, norm2, out=codes[s:s + chunk]))

    def file():
        new_off, dest = ops.ivfpq_list_place(assign, empty[0])
        return (new_off,) + ops.ivfpq_list_merge(*empty, dest, ids, codes, new_off)
    return (assign, codes) + st("file", file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--d", type=int, default=1024)
    ap.add_argument("--M", type=int, default=64)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["a", "b"], default=None, help="one path alone (kernel traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    N, d, M, nlist = args.rows, args.d, args.M, args.nlist
    dsub = d // M
    gen = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn(2048, d, device=dev, generator=gen)
    keys = torch.empty(N, d, device=dev)
    for s in range(0, N, 1 << 18):
        n = min(N, s + (1 << 18)) - s
        keys[s:s + n] = centres[torch.randint(0, 2048, (n,), device=dev, generator=gen)] + 0.7 * torch.randn(n, d, device=dev, generator=gen)
    R = torch.linalg.qr(torch.randn(d, d, device=dev, generator=gen))[0].contiguous()
    coarse = (normalise(keys[torch.randperm(N, device=dev, generator=gen)[:nlist]]) @ R.t()).contiguous()
    pq = (0.05 * torch.randn(M, 256, dsub, device=dev, generator=gen)).contiguous()
    norm2 = (pq ** 2).sum(2).contiguous()
    empty = (torch.zeros(nlist + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
             torch.empty(0, M, dtype=torch.uint8, device=dev))
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    run = {"a": lambda st: old_path(keys, R, coarse, pq, norm2, args.chunk, st),
           "b": lambda st: new_path(keys, R, coarse, pq, norm2, args.chunk, st, empty, ids)}
    which = [args.only] if args.only else ["a", "b"]
    warm = min(N, 2 * args.chunk)
    for p in which:                                                           # warm both paths on the shapes they time
        {"a": lambda: old_path(keys[:warm], R, coarse, pq, norm2, args.chunk, Stages()),
         "b": lambda: new_path(keys[:warm], R, coarse, pq, norm2, args.chunk, Stages(), empty, ids[:warm])}[p]()
    torch.cuda.synchronize()
    times, last = {p: [] for p in which}, {}
    for _ in range(args.repeats):
        for p in which:                                                       # the two take turns
            st = Stages()
            last[p] = run[p](st)
            times[p].append(st.totals())
            if len(times[p]) < args.repeats:
                last[p] = None                                                # (free the arrays before the other side runs)
    print(f"IVF-PQ add phase: {N} keys, d = {d}, M = {M} (dsub {dsub}), nlist = {nlist}, chunks of {args.chunk}; device events, "
          f"{args.repeats} repeats, the paths alternating; median (min .. max)")
    names = {"a": "(a) torch matmul + argmax + residual + gnnlm_pq_encode + sort", "b": "(b) gnnlm_gemm_nt + select_probes + gnnlm_ivfpq_encode_rows + list_merge"}
    med = {}
    for p in which:
        tot = np.array([sum(t.values()) for t in times[p]])
        med[p] = float(np.median(tot))
        rate = N / (tot / 1e3)
        print(f"{names[p]}\n    total {np.median(tot):9.1f} ms ({tot.min():.1f} .. {tot.max():.1f})    {np.median(rate) / 1e6:7.3f} M keys/s ({rate.min() / 1e6:.3f} .. {rate.max() / 1e6:.3f})")
        for stage in times[p][0]:
            v = np.array([t[stage] for t in times[p]])
            print(f"    {stage:<14s}{np.median(v):9.1f} ms ({v.min():.1f} .. {v.max():.1f})")
    if "b" in which:
        enc = np.array([t["encode"] for t in times["b"]]) / 1e3
        flops, lds = 2.0 * N * M * 256 * dsub, 256.0 * N * M * dsub          # LDS: 4 x 16-byte reads per thread per (tile, m, e) = 256 B per row
        floor_f, floor_l = flops / F32_PEAK, lds / LDS_PEAK
        print(f"encode kernel: {flops:.3e} FLOP in {np.median(enc) * 1e3:.1f} ms = {flops / np.median(enc) / 1e12:.1f} TFLOP/s; least time by the f32 rate "
              f"({F32_PEAK / 1e12:.1f} TF) {floor_f * 1e3:.1f} ms, by LDS reads ({lds:.3e} B at {LDS_PEAK / 1e12:.0f} TB/s) {floor_l * 1e3:.1f} ms: bound by "
              f"{'the f32 rate' if floor_f >= floor_l else 'LDS bandwidth'}, {100 * max(floor_f, floor_l) / np.median(enc):.0f} % of it")
    if len(which) == 2:
        (aa, ca, offa, ida, lca), (ab, cb, offb, idb, lcb) = last["a"], last["b"]
        same = aa == ab
        diff = int((ca[same] != cb[same]).sum())
        print(f"assignments agree on {int(same.sum())} of {N} keys (the others: float32 near-ties between two lists, the coarse scores come from "
              f"another GEMM); on the agreeing keys {diff} of {int(same.sum()) * M} codes differ (near-ties between two centroids: the rotated "
              f"rows of the two GEMMs differ in their last bits)")
        # the bit rule on the timed data: gnnlm_pq_encode over the residual of (b)'s OWN rotated rows and lists gives (b)'s codes
        bad = 0
        for s0 in range(0, N, args.chunk):
            xr = ops.gemm_nt(normalise(keys[s0:s0 + args.chunk]), R)
            r = (xr - coarse[ab[s0:s0 + args.chunk]]).contiguous()
            chk = torch.empty(r.shape[0], M, dtype=torch.uint8, device=dev)
            _lib.call("gnnlm_pq_encode", _lib.ptr(r), r.stride(0), _lib.ptr(pq), _lib.ptr(norm2), M, dsub, r.shape[0], _lib.ptr(chk), _lib.stream())
            bad += int((chk != cb[s0:s0 + args.chunk]).sum())
        every = bool(torch.equal(torch.sort(ida).values, ids) and torch.equal(torch.sort(idb).values, ids) and int(offa[-1]) == int(offb[-1]) == N)
        print(f"both paths file every key once: {every}; gnnlm_pq_encode on the materialised residual of (b)'s rotated rows: {bad} of {N * M} codes differ from (b)'s")
        print(f"(b) / (a) total time: {med['b'] / med['a']:.3f}")
        assert bad == 0 and every and diff <= 1e-5 * N * M


if __name__ == "__main__":
    main()
