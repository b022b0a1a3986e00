"""Which kernels one gnnlm_hgt_forward enqueues, route by route: the launches per profile id (the library's own event profiler)
of one forward through gnnlm_amd.hgt.HGT, against a table recorded from the library as it was while the forward was one function
(`PYTHONPATH=. python tests/test_hgt_launch_census_gpu.py` in a fresh process, GNNLM_LIB pointing at that build, prints it), and the
output of the profiled call against an un-profiled one, bit for bit.  A stage that went missing, ran twice or took the other
branch changes a count; the numbers themselves are the other HGT tests' business."""
import numpy as np
import pytest
import torch

from gnnlm_amd import _lib
from gnnlm_amd.hgt import HGT, CodeStore, NeighborGraph, TokenStore

pytestmark = pytest.mark.gpu

BASE = dict(d=64, H=4, M=8, dsub=8, T=8, kg=6, nblk=2)
LEFT = RIGHT = 2
N_STORE = 600

# route -> what differs from BASE / the plain forward.  calls: forwards profiled one after the other (the cache: a miss, then a hit)
ROUTES = {
    "L1": dict(L=1),
    "L2": dict(L=2),
    "L3": dict(L=3),
    "merged": dict(L=2, dedup=True),
    "row-keyed": dict(L=2, dedup=True, rows=True),
    "cache": dict(L=2, dedup=True, slots=4096, calls=2),
    "token-store": dict(L=2, token=True),
    "dense0-out_ntgt": dict(L=2, in_dim=32, return_ntgt=True),
    "ragged": dict(L=2, lengths=[5, 1, 8]),
    "fused-causal": dict(L=2, d=128, H=1, M=16, dsub=8, T=256, kg=4, nblk=1),
}

# launches per kernel id (gnnlm_kernel_name) of every profiled call
CAUSAL, CHAIN, GATHER, GEMM, LN, MISC, STAR = (
    "causal_attn_kernel", "chain_attn_kernel", "gather_decode_kernel", "gemm_nt_f32_kernel", "layernorm_kernel", "misc", "star_attn_kernel")
EXPECTED = {
    "L1": [{CAUSAL: 1, GEMM: 8, LN: 1, STAR: 1}],
    "L2": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 21, LN: 3, STAR: 2}],
    "L3": [{CAUSAL: 3, CHAIN: 2, GATHER: 1, GEMM: 33, LN: 5, STAR: 3}],
    "merged": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 21, LN: 3, MISC: 1, STAR: 2}],
    "row-keyed": [{CAUSAL: 2, CHAIN: 1, GATHER: 2, GEMM: 21, LN: 3, MISC: 2, STAR: 2}],
    "cache": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 21, LN: 3, MISC: 1, STAR: 2}, {CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 21, LN: 3, MISC: 1, STAR: 2}],
    "token-store": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 20, LN: 3, MISC: 1, STAR: 2}],
    "dense0-out_ntgt": [{CAUSAL: 2, CHAIN: 2, GATHER: 1, GEMM: 27, LN: 4, STAR: 2}],
    "ragged": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 13, LN: 3, STAR: 2}],
    "fused-causal": [{CAUSAL: 2, CHAIN: 1, GATHER: 1, GEMM: 13, LN: 3, STAR: 2}],
}


def _route(name, dev):
    """-> (model, graph, features, forward kwargs, profiled calls)"""
    r = dict(BASE, **ROUTES[name])
    d, H, M, dsub, kg = r["d"], r["H"], r["M"], r["dsub"], r["kg"]
    lengths = r.get("lengths")
    n_tok = sum(lengths) if lengths else r["nblk"] * r["T"]
    in_dim = r.get("in_dim", d)
    rs = np.random.RandomState(len(name) * 7 + r["L"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if r.get("token"):
        store = TokenStore(embed=t((rs.randn(50, d) * 0.5).astype(np.float32)), vals=t(rs.randint(0, 50, N_STORE).astype(np.int32)),
                           n_store=N_STORE)
    else:
        store = CodeStore(codes=t(rs.randint(0, 256, size=(N_STORE, M)).astype(np.uint8)),
                          centroids=t((rs.randn(M, 256, dsub) * 0.5).astype(np.float32)), n_store=N_STORE,
                          A=t((rs.randn(M * dsub, in_dim) / np.sqrt(M * dsub)).astype(np.float32)),
                          b=t((rs.randn(M * dsub) * 0.1).astype(np.float32)))
    # neighbour lists in runs with repeats: distinct centres that share rows, and equal centres -- something for every merge
    start = rs.randint(0, N_STORE - n_tok, size=(1, kg))
    nb = (start + np.arange(n_tok).reshape(n_tok, 1)).astype(np.int64)
    nb[n_tok // 2] = nb[0]
    nb[1, 0], nb[2] = -1, -1
    torch.manual_seed(11)
    model = HGT(in_dim=in_dim, hidden_dim=d, out_dim=d, n_layers=r["L"], n_heads=H)
    model.dedup_groups, model.dedup_rows = bool(r.get("dedup")), bool(r.get("rows"))
    model.state_cache_slots, model.state_cache_gib = r.get("slots"), 1.0 if r.get("slots") else 0.0
    if lengths:
        G = NeighborGraph(ids=t(nb), n_blocks=len(lengths), T=0, left=LEFT, right=RIGHT, store=store,
                          block_off=np.concatenate([[0], np.cumsum(lengths)]))
    else:
        G = NeighborGraph(ids=t(nb), n_blocks=r["nblk"], T=r["T"], left=LEFT, right=RIGHT, store=store)
    feats = {"tgt": t(rs.randn(n_tok, in_dim).astype(np.float16).astype(np.float32))}
    return model, G, feats, dict(return_ntgt=bool(r.get("return_ntgt"))), r.get("calls", 1)


def census(name, dev):
    """-> (launch counts of every profiled call, outputs of the profiled calls, outputs of the same calls un-profiled)"""
    model, G, feats, kw, calls = _route(name, dev)
    with torch.no_grad():
        plain = [{k: v.clone() for k, v in model(G, features=feats, **kw).items()} for _ in range(calls)]
        model.state_cache = None                                              # the profiled calls start where the plain ones did
        counts, outs = [], []
        for _ in range(calls):
            torch.cuda.synchronize()
            _lib.profile_begin()
            try:
                out = model(G, features=feats, **kw)
            finally:
                prof = _lib.profile_end()
            counts.append({k: v["launches"] for k, v in sorted(prof.items())})
            outs.append({k: v.clone() for k, v in out.items()})
    return counts, outs, plain


@pytest.mark.parametrize("name", list(ROUTES))
def test_launches_per_kernel_id(name):
    counts, outs, plain = census(name, torch.device("cuda:0"))
    print(name, counts)
    assert counts == EXPECTED[name]
    for o, p in zip(outs, plain):
        assert sorted(o) == sorted(p) and all(torch.equal(o[k], p[k]) for k in o)
        assert all(torch.isfinite(v).all() for v in o.values())


if __name__ == "__main__":
    import pprint
    pprint.pprint({name: census(name, torch.device("cuda:0"))[0] for name in ROUTES}, width=150, sort_dicts=False)
