"""A float64 restatement of generation from the GNN-LM, for tiny sizes (tests only; imports neither the package under test nor the
reference):

  the base LM of tests/decode_ref.py, one token at a time             -> the feature row x of every token
  brute-force top-kg of x over unit keys, ties to the lower id        -> the token's neighbour rows
  oracle.hgt.hgt_forward over the WHOLE prefix as one block           -> the GNN row of the last token
  the head's log-softmax (dense or adaptive, tied to the base LM's)   -> log-probs; pad = -inf; argmax

Nothing is cached between steps: every new token recomputes the graph decoder over its whole prefix, which is what a caller without
the incremental step has to do.  tests/test_gnn_decode_ref_cpu.py pins the identity the incremental step rests on.
"""
import numpy as np
import torch

import decode_ref as dr
from oracle import graph as og
from oracle import hgt as ohgt
from oracle import pq as opq

GNN_SEED = 301
# the seed of the keys and the code store, per head (the two heads are two models): the first seeds, counted from 0, under which the
# float64 chain itself meets the gap conditions of tests/test_generate_gnn_gpu.py with a fifth to spare
GNN_STORE_SEED = {"dense": 0, "adaptive": 3}
GNN_PROMPT_LENS = [1, 5, 40]
GNN_NEW = 24
GNN_LAYERS, GNN_KG, GNN_LEFT, GNN_RIGHT = 2, 8, 1, 1
GNN_KEYS, GNN_M, GNN_DSUB = 2000, 8, 8
GAP = 1e-3
_CACHE = {}


def hgt_rows(sd, L, H, tgt, nb, codes, cen, A, b, n_store, l, r):
    """The tgt rows [n, d] float64 of ONE block: features ``tgt`` [n, d], neighbour rows ``nb`` [n, kg] (-1: none)."""
    gr = og.build_graph(nb, np.zeros(nb.shape[0], np.int64), n_store, l, r)
    ntgt = opq.pq_lookup(codes[gr["ntgt_offsets"]], cen).astype(np.float64)
    if A is not None:
        ntgt = (ntgt - (b.astype(np.float64) if b is not None else 0)) @ A.astype(np.float64)
    feats = {"tgt": torch.from_numpy(np.asarray(tgt, np.float64)), "ntgt": torch.from_numpy(ntgt)}
    sdd = {k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}
    return ohgt.hgt_forward(sdd, L, H, feats, gr)["tgt"].numpy()


def top_neighbours(keys64, x, kg):
    """-> (ids [kg] by descending score, ties to the lower id; the gap between the kg-th and the (kg + 1)-th score)."""
    s = keys64 @ np.asarray(x, np.float64)
    order = np.lexsort((np.arange(s.shape[0]), -s))
    return order[:kg].astype(np.int64), float(s[order[kg - 1]] - s[order[kg]])


def gnn_store(head="dense", seed=GNN_SEED):
    """Seeded unit keys, a PQ 8x8 + OPQ code store over as many rows, and 2-layer HGT weights at the base LM's width."""
    if ("store", seed, head) not in _CACHE:
        d, H = dr.GEN_MODEL["d"], dr.GEN_MODEL["H"]
        rs = np.random.RandomState(GNN_STORE_SEED[head])
        keys = rs.randn(GNN_KEYS, d)
        keys = (keys / np.linalg.norm(keys, axis=1, keepdims=True)).astype(np.float32)
        dpq = GNN_M * GNN_DSUB
        st = dict(keys=keys, codes=rs.randint(0, 256, size=(GNN_KEYS, GNN_M)).astype(np.uint8),
                  cen=(rs.randn(GNN_M, 256, GNN_DSUB) * 0.5).astype(np.float32),
                  A=(rs.randn(dpq, d) / np.sqrt(dpq)).astype(np.float32), b=(rs.randn(dpq) * 0.1).astype(np.float32),
                  sd={k: v.numpy() for k, v in ohgt.init_hgt_weights(GNN_LAYERS, d, H, seed=seed).items()}, H=H)
        _CACHE["store", seed, head] = st
    return _CACHE["store", seed, head]


def gnn_prompts(seed=GNN_SEED):
    rs = np.random.RandomState(seed + 23)
    return [[int(t) for t in rs.randint(4, dr.GEN_MODEL["V"], size=n)] for n in GNN_PROMPT_LENS]


def head_logp(m, hw, g):
    return dr.dense_logp(m, g) if hw is None else dr.adaptive_dense_logp(g, **hw)


def gnn_greedy_chain(m, hw, st, prompt, n_new, pad=dr.PAD, eos=dr.EOS):
    """-> dict(tokens, logp [steps], gaps [steps] (best minus second-best log-prob), nb_gaps [prompt + steps - 1 .. ] (kg-th minus
    (kg + 1)-th neighbour score of every token fed), ids: the neighbour rows of every token fed [n, kg])."""
    inc = dr.Incremental(m)
    keys64 = st["keys"].astype(np.float64)
    xs, nbs, nb_gaps = [], [], []

    def feed(tok):
        x = inc.step(tok)["out"]
        ids, gap = top_neighbours(keys64, x, GNN_KG)
        xs.append(x), nbs.append(ids), nb_gaps.append(gap)

    for t in prompt:
        feed(t)
    toks, lps, gaps = [], [], []
    for _ in range(n_new):
        g = hgt_rows(st["sd"], GNN_LAYERS, st["H"], np.stack(xs), np.stack(nbs), st["codes"], st["cen"], st["A"], st["b"], GNN_KEYS,
                     GNN_LEFT, GNN_RIGHT)[-1]
        lp = head_logp(m, hw, g)
        lp[pad] = -np.inf
        order = np.argsort(-lp, kind="stable")
        toks.append(int(order[0])), lps.append(float(lp[order[0]])), gaps.append(float(lp[order[0]] - lp[order[1]]))
        if toks[-1] == eos or len(toks) == n_new:
            break
        feed(toks[-1])
    return dict(tokens=toks, logp=np.asarray(lps), gaps=np.asarray(gaps), nb_gaps=np.asarray(nb_gaps), ids=np.stack(nbs))


def gnn_chain(i, head="dense", seed=GNN_SEED):
    """The reference chain of prompt i under ``head`` (computed once, shared)."""
    if ("chain", seed, i, head) not in _CACHE:
        m, hw = dr.gen_model(seed, head)
        _CACHE["chain", seed, i, head] = gnn_greedy_chain(m, hw, gnn_store(head, seed), gnn_prompts(seed)[i], GNN_NEW)
    return _CACHE["chain", seed, i, head]
