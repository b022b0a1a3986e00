"""Float64 restatement of ``--reinit-nfeat`` (neighbour features from the token embedding), test infrastructure only.

What the reference computes (fairseq/tasks/language_modeling.py:151-153,273-278; fairseq/data/token_block_dataset.py:369-371,
392-394,407-410; fairseq/models/transformer.py:1046-1048), restated:

  * the table: ``embed_tokens`` called directly on a label -- no embed_scale, no positions, no project_in_dim.  Adaptive input
    (fairseq/modules/adaptive_input.py:63-74): band i with cutoff[i-1] <= y < cutoff[i] gives
    ``emb_i[y - cutoff[i-1]] @ proj_i.T``, band 0 with its own projection; plain embedding: ``weight[y]``;
  * the graph: node order, validity and edges of the code-store graph (``oracle.graph.build_graph``), the ntgt feature of a
    node with datastore row r is ``E[vals[r]]``;
  * the model: ``oracle.hgt.hgt_forward`` on those features.

``slot_rows`` / ``token_gather`` / ``neighbor_labels`` restate the padded-slot view the HIP kernels write (include/gnnlm.h).
"""
import numpy as np
import torch

from oracle import graph as og
from oracle import hgt as ohgt


def embed_table(bands=None, plain=None, dtype=np.float64, skip_band0_proj=False):
    """E [V, d].  bands = [(emb_i [size_i, dim_i], proj_i [d, dim_i]), ...] or plain = weight [V, d].
    skip_band0_proj: the WRONG table a build would get that treats band 0 like the adaptive softmax does (no projection)."""
    if plain is not None:
        return np.asarray(plain, dtype=dtype)
    rows = []
    for i, (e, p) in enumerate(bands):
        e, p = np.asarray(e, dtype=dtype), np.asarray(p, dtype=dtype)
        rows.append(e if (i == 0 and skip_band0_proj) else e @ p.T)
    return np.concatenate(rows, 0)


def fixture_table(g, kind="adaptive", **kw):
    if kind == "plain":
        return embed_table(plain=g["plain_weight"], **kw)
    return embed_table(bands=[(g[f"emb{i}"], g[f"proj{i}"]) for i in range(len(g["cutoff"]))], **kw)


def slot_rows(ids, left, right):
    """[n_groups, 1 + left + right] datastore row of every slot: centre o, then o-left .. o-1, then o+1 .. o+right."""
    delta = np.array([0] + list(range(-left, 0)) + list(range(1, right + 1)), dtype=np.int64)
    return np.asarray(ids, dtype=np.int64).reshape(-1, 1) + delta[None, :]


def token_gather(E, vals, ids, left, right, n_store, n_vocab=None):
    """-> (x [n_slots, d], labels int32 [n_slots] (-1: invalid), valid uint8 [n_slots]).  A slot is valid iff its centre id is
    >= 0, its row lies in [0, n_store) and its label in [0, n_vocab); x is the table row (a copy) or zeros."""
    E = np.asarray(E)
    n_vocab = E.shape[0] if n_vocab is None else n_vocab
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    rows = slot_rows(ids, left, right)
    ok = (ids[:, None] >= 0) & (rows >= 0) & (rows < n_store)
    lab = np.where(ok, np.asarray(vals).astype(np.int64)[np.clip(rows, 0, max(n_store - 1, 0))], -1)
    lab = np.where((lab >= 0) & (lab < n_vocab), lab, -1).reshape(-1)
    x = np.where((lab >= 0)[:, None], E[np.clip(lab, 0, None)], 0).astype(E.dtype)
    return x, lab.astype(np.int32), (lab >= 0).astype(np.uint8)


def neighbor_labels(ids, vals, n_store, n_vocab):
    ids = np.asarray(ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < n_store)
    lab = np.where(ok, np.asarray(vals).astype(np.int64)[np.clip(ids, 0, max(n_store - 1, 0))], -1)
    return np.where((lab >= 0) & (lab < n_vocab), lab, -1).astype(np.int32)


def forward(E, vals, nb, n_store, left, right, sd, n_layers, n_heads, tgt, all_layers=False, dtype=torch.float64,
            tgt_offsets=None, invalid_neighbor_context=0, max_intra_context=0):
    """The reference-order forward of one block in ``dtype``: (outputs of oracle.hgt.hgt_forward, the graph dict)."""
    nb = np.asarray(nb)
    gr = og.build_graph(nb, np.zeros(nb.shape[0], np.int64) if tgt_offsets is None else tgt_offsets, n_store, left, right,
                        invalid_neighbor_context=invalid_neighbor_context, max_intra_context=max_intra_context)
    labels = np.asarray(vals).astype(np.int64)[gr["ntgt_offsets"]]
    feats = {"tgt": torch.as_tensor(np.asarray(tgt)).to(dtype),
             "ntgt": torch.as_tensor(np.asarray(E)[labels].reshape(len(labels), np.asarray(E).shape[1])).to(dtype)}
    sd = {k: torch.as_tensor(np.asarray(v)).to(dtype) if torch.as_tensor(np.asarray(v)).is_floating_point() else torch.as_tensor(np.asarray(v))
          for k, v in sd.items()}
    return ohgt.hgt_forward(sd, n_layers, n_heads, feats, gr, return_all_layers=all_layers), gr


def fixture_cases(g):
    """[(key, tag, left, right, n_layers, n_heads, kind)] of tests/golden/reinit_nfeat.npz."""
    out = []
    for key in sorted({k.split(".tgt_in")[0] for k in g.files if k.endswith(".tgt_in")}):
        tag, cfg = key.split(".")
        kind = "plain" if cfg.endswith("plain") else "adaptive"
        cfg = cfg[:-5] if kind == "plain" else cfg
        out.append((key, tag, int(tag[1]), int(tag[3]), int(cfg[1]), int(cfg[3:]), kind))
    return out


def fixture_sd(g, n_layers, n_heads):
    pre = f"sd.L{n_layers}H{n_heads}."
    return {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}
