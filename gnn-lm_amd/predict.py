"""Next-token distributions in row chunks: top-N, the target's rank and log-probability without the ``[n, V]`` tensor of a batch.

The reference answers "what does GNN + kNN predict here" with two dense tensors, ``get_normalized_probs`` ``[B, T, V]``
(fairseq/models/transformer.py:1064-1085) and ``get_knn_prob(targets=None)`` ``[B*T, V]`` (knn/knn_model.py:192-205), 1 GB per 1024
tokens at the WikiText-103 vocabulary.  ``predict_rows`` walks the rows in chunks of at most ``DENSE_CHUNK_BYTES`` of dense
log-probs: head (csrc/dense_dist.hip) -> optional ``orig_prob_ratio`` mixture (``gnnlm_logp_mix`` over the flattened chunk) ->
optional kNN mix (``gnnlm_knn_mix_dense``) -> ``gnnlm_topk_merge`` with ``ncols = V`` and ``gnnlm_row_rank``.  Only the ``[n, N]``
results outlive a chunk.
"""
import torch

from . import ops

DENSE_CHUNK_BYTES = 256 << 20     # dense log-probs alive per buffer: the size of the Infinity Cache
MAX_TOPK = 2048                   # gnnlm_topk_merge's k


def head_vocab(asm) -> int:
    return int(asm.vocab) if hasattr(asm, "vocab") else int(asm.cutoff[-1])


def chunk_rows(V: int, chunk_bytes=None) -> int:
    """Rows of a chunk (``chunk_bytes`` None: the module's DENSE_CHUNK_BYTES as it is now)."""
    return max(1, int(DENSE_CHUNK_BYTES if chunk_bytes is None else chunk_bytes) // (4 * int(V)))


def check_topk(topk, V=None):
    if not isinstance(topk, int) or isinstance(topk, bool) or topk < 1:
        raise ValueError(f"topk: a positive integer, got {topk!r}")
    if topk > MAX_TOPK:
        raise ValueError(f"topk = {topk}: at most {MAX_TOPK} (the k-selection kernel keeps its state in LDS)")
    if V is not None and topk > V:
        raise ValueError(f"topk = {topk} exceeds the vocabulary ({V})")


def lm_dense_rows(asm, x, h=None, ratio=0.0):
    """Dense log-probs of the rows ``x`` [c, d] under head ``asm``; with ``h`` (the base LM's features of the same rows) and
    ``ratio`` > 0 the ``orig_prob_ratio`` mixture of the two heads (transformer.py:1056-1062,1075-1077) -> [c, V] f32."""
    gnn = asm.log_probs(x)
    if h is None or ratio <= 0:
        return gnn
    if ratio >= 1:
        raise ValueError(f"math domain error: orig_prob_ratio = {ratio} needs log(1 - orig_prob_ratio) (transformer.py:1060)")
    base = asm.log_probs(h)
    return ops.logp_mix(gnn.view(-1), base.view(-1), [float(ratio)])[0].view_as(gnn)


def predict_rows(dense_fn, n, V, targets, topk, knn=None, chunk_bytes=None):
    """-> (ids [n, N] int64, logp [n, N] f32, target_rank [n] int32, target_logp [n] f32), best first, ties by ascending id.

    ``dense_fn(r0, r1)`` -> the language model's dense log-probs of rows [r0, r1), [r1 - r0, V] f32.  ``knn`` (optional): dict
    ``sims`` [n, k], ``ids`` [n, k], ``temperature``, ``lmbda`` and the labels (``vals`` / ``n_store`` / ``row0`` / ``knn_vals``) as
    :func:`ops.knn_mix_dense` takes them; the rows are then the kNN mixture.  ``targets`` [n] int64: a target outside [0, V) has
    rank -1 and log-probability -inf."""
    check_topk(topk, V)
    dev = targets.device
    targets = targets.contiguous()
    ids = torch.empty(n, topk, device=dev, dtype=torch.int64)
    logp = torch.empty(n, topk, device=dev, dtype=torch.float32)
    rank = torch.empty(n, device=dev, dtype=torch.int32)
    tlogp = torch.empty(n, device=dev, dtype=torch.float32)
    step = chunk_rows(V, chunk_bytes)
    mix_buf = None
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        dense = dense_fn(r0, r1)
        if knn is not None:
            if mix_buf is None:
                mix_buf = torch.empty(min(step, n), V, device=dev, dtype=torch.float32)
            kv = knn.get("knn_vals")
            dense = ops.knn_mix_dense(dense, knn["sims"][r0:r1], knn["ids"][r0:r1], knn["temperature"], knn["lmbda"],
                                      vals=knn.get("vals") if kv is None else None, n_store=knn.get("n_store"), row0=knn.get("row0", 0),
                                      knn_vals=None if kv is None else kv[r0:r1], out=mix_buf[:r1 - r0])
        ops.topk_merge(dense, logp[r0:r1], ids[r0:r1], init=True)
        t = targets[r0:r1]
        ops.row_rank(dense, t, out=rank[r0:r1])
        inside = (t >= 0) & (t < V)
        picked = dense.gather(1, t.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
        tlogp[r0:r1] = torch.where(inside, picked, torch.full_like(picked, float("-inf")))
    return ids, logp, rank, tlogp


def topk_stats(rank, topk):
    """-> (top-1 accuracy, top-N accuracy, mean reciprocal rank) of a host array of target ranks (-1: not in the vocabulary)."""
    import numpy as np
    rank = np.asarray(rank, dtype=np.int64)
    if rank.size == 0:
        return 0.0, 0.0, 0.0
    ok = rank >= 0
    return (float((ok & (rank == 0)).mean()), float((ok & (rank < topk)).mean()),
            float(np.where(ok, 1.0 / (np.maximum(rank, 0) + 1.0), 0.0).mean()))
