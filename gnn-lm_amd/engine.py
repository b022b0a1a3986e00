"""The eval hot path as one object: gather -> HGT -> adaptive softmax -> kNN interpolation.

``GnnLmEngine.score`` is what one iteration of the reference's hot loop computes between
``gen_timer.start()`` and ``gen_timer.stop()`` (fairseq_cli/eval_lm.py:214-219) *plus* the graph
construction the reference does in its DataLoader workers (token_block_dataset.py:287-331), for a
batch of independent token blocks:

    TokenGraphTransformerDecoder.forward          fairseq/models/transformer.py:943-1009
    AdaptiveSoftmax.get_log_prob + gather         fairseq/modules/adaptive_softmax.py:170-206
    KNNModel.get_knn_prob                         knn/knn_model.py:87-101 (search: on the device with ``knn_index``), 179-217
    combine_knn_and_vocab_probs                   fairseq/sequence_scorer.py:55-68

Everything runs on the current HIP stream through libgnnlm_hip.so; nothing synchronises.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops
from .adaptive_softmax import AdaptiveSoftmax
from .dense_softmax import DenseSoftmax
from .hgt import HGT, CodeStore, NeighborGraph, TokenStore


@dataclass
class BlockBatch:
    """Inputs of one step: ``n_blocks`` independent blocks of ``T`` tokens (device tensors)."""
    ids: torch.Tensor                       # int64 [n_blocks*T, kg]  rows of neighbors.mmap.{kg}
    tgt_feats: torch.Tensor                 # fp16 / fp32 [n_blocks*T, d]  rows of {split}_dstore/keys.npy
    targets: torch.Tensor                   # int64 [n_blocks*T]
    n_blocks: int
    T: int
    knn_sims: Optional[torch.Tensor] = None  # f32 [n_blocks*T, k]   similarities of the kNN search
    knn_ids: Optional[torch.Tensor] = None   # int64 [n_blocks*T, k] (-1 = padding)
    knn_vals: Optional[torch.Tensor] = None  # int32 [n_blocks*T, k] vals[knn_ids] if already fetched (sharded store)
    fetched_codes: Optional[torch.Tensor] = None
    fetched_valid: Optional[torch.Tensor] = None
    fetched_centres_only: bool = False
    fetched_index: Optional[torch.Tensor] = None
    # blocks of unequal length packed back to back: a ragged.RaggedBatch or offsets [n_blocks + 1]; None = n_blocks x T (T is then read)
    block_off: Optional[object] = None


class GnnLmEngine:
    def __init__(self, hgt: HGT, asm: "AdaptiveSoftmax | DenseSoftmax", store: "CodeStore | TokenStore", left: int, right: int,
                 max_intra_context: int = 0, fetcher=None, fetch_vals: bool = False, precision=None):
        self.hgt, self.asm, self.store = hgt, asm, store
        if precision is not None:                    # None: whatever hgt / asm already carry
            self.precision = precision
        self.left, self.right, self.max_intra_context = left, right, max_intra_context
        # range-sharded store (dist.ShardedFetcher): the code rows -- and, with fetch_vals, the labels of the kNN ids -- are
        # fetched from their owners inside the step (batches that bring their own fetched_* / knn_vals keep them)
        self.fetcher, self.fetch_vals = fetcher, fetch_vals

    @property
    def precision(self) -> str:
        """Arithmetic of the GEMMs of the HGT and of the adaptive softmax, a name of ``ops.PRECISIONS``: "f32" (default), "fp16"
        (what ``eval_lm --fp16`` sets: float16 operands rounded to nearest even, f32 accumulation; everything else stays f32),
        "bf16x3" / "bf16x6".  Setting it sets both modules; cached centre states of another precision are dropped (hgt.py)."""
        return ops.precision_name(self.hgt.gemm_precision, self.asm.gemm_precision)

    @precision.setter
    def precision(self, value):
        self.hgt.gemm_precision = self.asm.gemm_precision = ops.precision_value(value)

    def features(self, batch: BlockBatch) -> torch.Tensor:
        """gcn_feat: HGT output for every token [n_blocks*T, d] (transformer.py:997)."""
        tgt = batch.tgt_feats
        if tgt.dtype == torch.float16:
            tgt = ops.half_to_float(tgt.contiguous())           # token_block_dataset.py:328
        G = NeighborGraph(ids=batch.ids, n_blocks=batch.n_blocks, T=batch.T, left=self.left, right=self.right,
                          store=self.store, fetched_codes=batch.fetched_codes, fetched_valid=batch.fetched_valid,
                          fetched_centres_only=batch.fetched_centres_only, fetched_index=batch.fetched_index,
                          max_intra_context=self.max_intra_context, fetcher=self.fetcher if batch.fetched_codes is None else None,
                          block_off=batch.block_off)
        return self.hgt(G, features={"tgt": tgt})["tgt"]

    def score(self, batch: BlockBatch, lmbda: float = 0.0, temperature: float = 1.0, knn_index=None, k: int = 0, sweep=None,
              knn_keys=None, knn_sim_func: str = "do_not_recomp_ip", orig_prob_ratio: float = 0.0):
        """Per-token log-probabilities.  Returns dict(gcn_feat, lm_logp, logp[, p_knn, recall]).

        ``orig_prob_ratio`` = alpha in (0, 1) (transformer.py:987-1005,1056-1062,1075-1077): ``lm_logp`` is the mixture
        logsumexp(log(alpha) + ``lm_logp_base``, log(1 - alpha) + ``lm_logp_gnn``) of the tied softmax over the batch's precomputed
        features and over the HGT output (both returned), ``logp`` the kNN mix of that.  <= 0: off (``lm_logp`` is ``lm_logp_gnn``);
        >= 1: ValueError, as the reference's math.log(1 - alpha).  A sweep may carry a fourth element ``alphas`` (each in 0 .. 1, at most
        8): ``sweep_logp`` is then [len(alphas) * G, n] with alpha slowest (``ops.grid_points(ks, ts, ls, alphas)``), from one more
        softmax pass whatever the number of alphas; ``(None, None, None, alphas)`` sweeps the ratio alone.

        ``sweep = (ks, temperatures, lmbdas)``: additionally ``sweep_logp`` [G, n], every point of the kNN-LM tuning grid
        (``ops.grid_points`` order) from the step's one forward and one search (which then runs with ``lmbda`` 0 too).

        ``knn_index`` (an ``ivfpq.IVFPQIndex`` with the labels attached): the kNN search of the step's own queries -- the gcn_feat
        rows, L2-normalised for a cosine index only (knn_model.py:100,181-184) -- runs on the device inside the step, as it runs inside the
        reference's timer (fairseq_cli/eval_lm.py:214-219 around sequence_scorer.py:115-120); the batch's ``knn_*`` fields are
        then not read.  The softmax is enqueued between the search and the host's one look at its survivor counts.

        ``knn_keys`` (the key table in HBM, fp16 / f32 [n_store, d]) with ``knn_sim_func`` "ip" / "l2" (``--knn-sim-func``,
        knn_model.py:161-175): the index's distances are replaced by the similarities recomputed from the full-precision keys
        (``ops.knn_recompute_sims``; "ip" divides by |key| as the reference does for a cosine index) before
        the interpolation and the sweep, and come back as ``knn_sims``.  "do_not_recomp_l2" with an L2 index (``metric="l2"``, the
        reference's default ``faiss_store.l2``): the similarities are the negated squared distances of the search (knn_model.py:153-154)."""
        return self.score_finish(self.score_begin(batch, lmbda, temperature, knn_index, k, sweep, knn_keys, knn_sim_func, orig_prob_ratio))

    def predict(self, batch: BlockBatch, lmbda: float = 0.0, temperature: float = 1.0, knn_index=None, k: int = 0, sweep=None,
                knn_keys=None, knn_sim_func: str = "do_not_recomp_ip", orig_prob_ratio: float = 0.0, topk: int = 1):
        """The arguments of ``score`` plus ``topk`` = N <= 2048 -> ``(ids [n, N] int64, logp [n, N], target_rank [n] int32,
        target_logp [n])``: the N most probable next tokens of every position under the distribution ``score`` takes the target's
        column of (GNN head, ``orig_prob_ratio`` mixture, kNN mix), best first with ties by ascending id; the number of tokens in
        front of the target; and the target's own log-probability (``score``'s ``logp`` up to the summation order of p_knn).
        Worked in row chunks of at most 256 MiB of dense log-probs (``predict.predict_rows``): the [n, V] tensor of the batch never
        exists.  A sweep has no single distribution: refused."""
        from .predict import check_topk, head_vocab, lm_dense_rows, predict_rows
        if sweep:
            raise ValueError("predict: a sweep has no single distribution to rank; call it once per setting")
        V = head_vocab(self.asm)
        check_topk(topk, V)
        out = self.score_finish(self.score_begin(batch, lmbda, temperature, knn_index, k, None, knn_keys, knn_sim_func, orig_prob_ratio))
        x = out["gcn_feat"]
        h = None
        if orig_prob_ratio > 0:
            h = batch.tgt_feats
            h = ops.half_to_float(h.contiguous()) if h.dtype == torch.float16 else h.float()
        knn = None
        if lmbda > 0.0:
            if "knn_sims" in out:                                # searched inside the step
                knn = dict(sims=out["knn_sims"], ids=out["knn_ids"], knn_vals=out["knn_vals"], n_store=self.store.n_store)
            else:
                knn_vals = batch.knn_vals
                if knn_vals is None and self.fetcher is not None and self.fetch_vals:
                    knn_vals = self.fetcher.fetch_knn_vals(batch.knn_ids)
                knn = dict(sims=batch.knn_sims.contiguous(), ids=batch.knn_ids.contiguous(), knn_vals=knn_vals, vals=self.store.vals,
                           n_store=self.store.n_store, row0=getattr(self.store, "vals_row0", self.store.row0))
            knn.update(temperature=temperature, lmbda=lmbda)
        dense_fn = lambda r0, r1: lm_dense_rows(self.asm, x[r0:r1], None if h is None else h[r0:r1], orig_prob_ratio)
        return predict_rows(dense_fn, x.shape[0], V, batch.targets, topk, knn)

    def score_begin(self, batch: BlockBatch, lmbda: float = 0.0, temperature: float = 1.0, knn_index=None, k: int = 0, sweep=None,
                    knn_keys=None, knn_sim_func: str = "do_not_recomp_ip", orig_prob_ratio: float = 0.0):
        """Enqueue the step up to the search's host read (features, search, softmax) and return a handle for ``score_finish``:
        several batches can be in flight (one per stream), the host looks at a search's survivor counts only when it comes back
        to that batch."""
        if knn_sim_func not in ("do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2"):
            raise ValueError("knn_sim_func: do_not_recomp_ip, do_not_recomp_l2, ip or l2")
        if not knn_sim_func.startswith("do_not_recomp") and knn_keys is None:
            raise ValueError(f"knn_sim_func={knn_sim_func!r} needs knn_keys (the key table in HBM)")
        index_l2 = getattr(knn_index, "metric", "ip") == "l2"
        if knn_index is not None and knn_sim_func.startswith("do_not_recomp") and (knn_sim_func == "do_not_recomp_l2") != index_l2:
            raise ValueError(f"knn_sim_func={knn_sim_func!r} on an index of metric {'l2' if index_l2 else 'ip'}: the search's own values are "
                             "similarities for do_not_recomp_ip on an inner-product index and for do_not_recomp_l2 on an L2 index only")
        if orig_prob_ratio >= 1:
            raise ValueError(f"math domain error: orig_prob_ratio = {orig_prob_ratio} needs log(1 - orig_prob_ratio) (transformer.py:1060)")
        alpha = float(orig_prob_ratio) if orig_prob_ratio > 0 else 0.0
        alphas = list(sweep[3]) if sweep and len(sweep) > 3 else None
        sweep = tuple(sweep[:3]) if sweep and sweep[0] is not None else None
        x = self.features(batch)
        pending = qn = None
        # knn_model.py:181-184: the queries (and, for "ip", the recomputed keys, :172-173) are normalised for a cosine index only; an index
        # object that does not say (no `cosine` attribute: a search stand-in) is a cosine one, as every index was before L2 ones existed
        cosine = getattr(knn_index, "cosine", True)
        if (lmbda > 0.0 or sweep) and knn_index is not None:
            qn = x / (x ** 2).sum(-1, keepdim=True).sqrt() if cosine else x
            pending = knn_index.search_begin(qn.contiguous(), k, return_vals=True)
        branches = lm_rows = None
        if alpha > 0 or alphas:
            # the base branch: the same softmax over the precomputed features (the "orig_x" of transformer.py:988 under
            # --use-precompute-feat), one more pass whatever the number of alphas.  Two n-row calls, not one over the stacked [2n, d]
            # rows: the GEMMs take the same time either way and the stacked form pays for its two concatenations
            h = batch.tgt_feats
            h = ops.half_to_float(h.contiguous()) if h.dtype == torch.float16 else h.float()
            lm_logp = self.asm.target_log_prob(x, batch.targets)
            branches = (lm_logp, self.asm.target_log_prob(h, batch.targets))
            if alphas:
                lm_rows = ops.logp_mix(*branches, alphas)                  # [A, n]: the grid's language-model rows
            if alpha > 0:
                lm_logp = ops.logp_mix(*branches, [alpha])[0]
        else:
            lm_logp = self.asm.target_log_prob(x, batch.targets)
        resim = (qn, knn_keys, knn_sim_func, cosine) if pending is not None and not knn_sim_func.startswith("do_not_recomp") else None
        if pending is not None and resim is None and index_l2:
            resim = "negate"                                             # knn_model.py:153-154: sims = -dists
        return batch, lmbda, temperature, x, lm_logp, pending, sweep, resim, branches, lm_rows

    def score_finish(self, handle):
        batch, lmbda, temperature, x, lm_logp, pending, sweep, resim, branches, lm_rows = handle
        out = {"gcn_feat": x, "lm_logp": lm_logp, "logp": lm_logp}
        if branches is not None:
            out.update(lm_logp_gnn=branches[0], lm_logp_base=branches[1])
        if lm_rows is not None and not sweep:
            out["sweep_logp"] = lm_rows                                   # the ratio alone: one point per alpha
        grid_lm = lm_rows if lm_rows is not None else lm_logp
        if pending is not None:
            sims, ids, vals = pending.result()
            if resim == "negate":
                sims = -sims
            elif resim is not None:                              # knn_model.py:161-175 on the step's own queries
                qn, keys, fn, cosine = resim
                sims = ops.knn_recompute_sims(qn.contiguous(), ids.contiguous(), keys, fn, normalize_keys=(fn == "ip" and cosine))
            if lmbda > 0.0:
                logp, p_knn, recall = ops.knn_interp(lm_logp, sims, ids, batch.targets, temperature, lmbda,
                                                     n_store=self.store.n_store, knn_vals=vals)
                out.update(logp=logp, p_knn=p_knn, recall=recall)
            out.update(knn_sims=sims, knn_ids=ids, knn_vals=vals)
            if sweep:
                out["sweep_logp"] = ops.knn_interp_grid(grid_lm, sims, ids, batch.targets, *sweep, n_store=self.store.n_store, knn_vals=vals)[0]
        elif lmbda > 0.0 or sweep:                               # sequence_scorer.py:102
            if batch.knn_sims is None or batch.knn_ids is None:
                raise ValueError("lmbda > 0 needs knn_sims / knn_ids (results of the kNN search)")
            knn_vals = batch.knn_vals
            if knn_vals is None and self.fetcher is not None and self.fetch_vals:
                knn_vals = self.fetcher.fetch_knn_vals(batch.knn_ids)
            labels = dict(vals=self.store.vals, n_store=self.store.n_store, row0=getattr(self.store, "vals_row0", self.store.row0), knn_vals=knn_vals)
            if lmbda > 0.0:
                logp, p_knn, recall = ops.knn_interp(lm_logp, batch.knn_sims, batch.knn_ids, batch.targets, temperature, lmbda, **labels)
                out.update(logp=logp, p_knn=p_knn, recall=recall)
            if sweep:
                out["sweep_logp"] = ops.knn_interp_grid(grid_lm, batch.knn_sims, batch.knn_ids, batch.targets, *sweep, **labels)[0]
        return out
