"""``SequenceScorer`` -- mirror of ``fairseq/sequence_scorer.py:17-194`` for the LM eval path.

Same constructor, same ``generate(models, sample, knn_dstore=..., temperature=...)`` call, same
hypothesis dicts (``tokens, score, attention, alignment, positional_scores, dstore_keys, knn_recall``,
:185-193).  (This build) with ``args.sweep = (ks, temperatures, lmbdas[, alphas])`` ``generate_finish`` also leaves
``handle["sweep_logp"]`` [G, scored tokens]: every point of the kNN-LM tuning grid, from the batch's one search (``alphas``: the
``orig_prob_ratio`` axis, slowest, from the model's two softmax branches; ``(None, None, None, alphas)`` sweeps the ratio alone).
(This build) with ``args.output_topk = N > 0`` every hypothesis also carries ``topk_ids`` / ``topk_scores`` [len, N] and ``target_rank`` [len].
What differs is only where the arithmetic runs: the dense ``[B, T, V]`` log-prob tensor and
the host-side kNN gathers are replaced by the HIP kernels behind ``model.target_log_probs`` and
``KNNModel.interpolate``.

Reference behaviours kept on purpose:
  * the kNN queries are ``extra[args.knn_keytype]`` if present else ``inner_states[-1]`` (:105) -- the
    recipe's ``--knn-keytype keytype`` typo therefore selects the base-LM features;
  * queries are flattened in [T, B] order but targets in [B, T] order (``orig_target.permute(0, 1)``
    is a no-op, :117): identical for bsz == 1 (the recipe), reproduced as written otherwise;
  * ``softmax_batch`` is accepted; the precondition B*T < softmax_batch of the kNN branch (:105 todo)
    is asserted instead of silently using the last sub-batch.
"""
import sys

import torch


def strip_pad(tensor, pad):
    return tensor[tensor.ne(pad)]                                   # fairseq/utils.py:190-191


class SequenceScorer(object):
    def __init__(self, tgt_dict, softmax_batch=None, compute_alignment=False, args=None):
        self.pad, self.eos = tgt_dict.pad(), tgt_dict.eos()
        self.softmax_batch = softmax_batch or sys.maxsize
        assert self.softmax_batch > 0
        self.compute_alignment, self.args = compute_alignment, args

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        return self.generate_finish(self.generate_begin(models, sample, **kwargs))

    @torch.no_grad()
    def generate_begin(self, models, sample, **kwargs):
        """(this build) ``generate`` up to the kNN search's one host read: forward, search and softmax are enqueued, the handle goes to
        ``generate_finish``.  A driver with several batches in flight (eval_lm --streams) comes back to a batch when the others are
        enqueued: the host never waits on a search while the device has nothing else to do."""
        if len(models) != 1:
            raise ValueError("Only knn *log* probs are supported.")        # :108-109 (ensembles unused on this path)
        model = models[0]
        net_input = sample["net_input"]
        temperature = kwargs.get("temperature", 1.0)
        orig_target = sample["target"]
        decoder_out = model(**net_input)
        bsz, tsz = orig_target.shape
        lmbda = getattr(self.args, "lmbda", 0.0)
        use_knn = "knn_dstore" in kwargs and lmbda > 0.0
        # (this build) args.sweep = (ks, temperatures, lmbdas): the tuning grid is scored from this batch's one search -- which therefore
        # runs with --lmbda 0 too (the hypotheses then stay the LM's)
        sweep = getattr(self.args, "sweep", None)
        # a fourth element is the orig_prob_ratio axis (alphas): the model's two unmixed branches are mixed at every alpha, and each
        # mixture is one language-model row of the grid -- or, without a kNN term (ks None / no knn_dstore), a point of its own
        alphas = sweep[3] if sweep and len(sweep) > 3 else None
        sweep = tuple(sweep[:3]) if sweep and sweep[0] is not None and "knn_dstore" in kwargs else None
        pending = None
        if use_knn or sweep:
            # (the reference's precondition is about ITS batch: with the driver's --batch-blocks the launch holds several of the recipe's
            # one-block batches, each of which must fit -- the recipe passes --softmax-batch 3072 for 256-token batches)
            assert (tsz if sample.get("blockwise_knn") else bsz * tsz) < self.softmax_batch, "kNN scoring needs B*T < --softmax-batch (sequence_scorer.py:105)"
            knn_model = kwargs["knn_dstore"]
            extra = decoder_out[1]
            kt = getattr(self.args, "knn_keytype", None)
            queries = extra[kt] if kt in extra else extra["inner_states"][-1]          # [T, B, C]  (:105)
            seq_len, b2, hidden = queries.shape
            # the search only needs the features: it is enqueued BEFORE the softmax (which does not need the neighbours), and its
            # one host round trip (survivor counts) is waited for AFTER -- the device works through the softmax meanwhile
            if hasattr(knn_model, "interpolate_begin"):
                pending = knn_model.interpolate_begin(queries.contiguous().view(-1, hidden))
        probs = model.target_log_probs(decoder_out, orig_target.clamp(min=0))
        return dict(sample=sample, decoder_out=decoder_out, probs=probs, use_knn=use_knn, pending=pending, lmbda=lmbda, temperature=temperature, model=model,
                    knn_model=kwargs.get("knn_dstore"), queries=(queries if use_knn or sweep else None), sweep=sweep, alphas=alphas)

    @torch.no_grad()
    def generate_finish(self, h):
        sample, decoder_out, probs, use_knn, pending = h["sample"], h["decoder_out"], h["probs"], h["use_knn"], h["pending"]
        lmbda, temperature, knn_model = h["lmbda"], h["temperature"], h["knn_model"]
        orig_target = sample["target"]
        bsz, tsz = orig_target.shape
        recall = None
        sweep, grid, alphas = h.get("sweep"), None, h.get("alphas")
        # (this build) args.output_topk = N > 0: every hypothesis also carries the N most probable next tokens of each scored position
        # (`topk_ids` / `topk_scores` [len, N], best first) and the number of tokens in front of the target (`target_rank` [len])
        topk, found = int(getattr(self.args, "output_topk", 0) or 0), None
        if topk and (sweep or alphas):
            raise ValueError("output_topk with a sweep: a grid has no single distribution to rank")
        if alphas:
            from . import ops
            if "branch_logp" not in decoder_out[1]:
                raise ValueError("a sweep over orig_prob_ratio needs the model's two branches (GnnLmModel.keep_branches)")
            gnn, base = decoder_out[1]["branch_logp"]                                   # [B, T] each, unmixed
        if sweep:
            # one search result, two consumers: the hypotheses' own setting and the grid (same targets, same pairing)
            queries = h["queries"]
            seq_len, b2, hidden = queries.shape
            tq = (orig_target.transpose(0, 1) if sample.get("blockwise_knn") else orig_target.permute(0, 1)).reshape(seq_len * b2)
            lm_flat = probs.transpose(0, 1).reshape(-1)
            found = knn_model.search_finish(pending if pending is not None else knn_model.interpolate_begin(queries.contiguous().view(-1, hidden)))
            lm_rows = lm_flat if not alphas else \
                ops.logp_mix(gnn.transpose(0, 1).reshape(-1), base.transpose(0, 1).reshape(-1), alphas)   # [A, T*B]: alpha is the grid's slowest axis
            grid = knn_model.interpolate_grid_finish(found, tq.clamp(min=0), lm_rows, *sweep)[0].view(-1, seq_len, b2).transpose(1, 2)   # [G, B, T]
            if use_knn:
                mixed, _, rec = knn_model.interpolate_finish(found, tq.clamp(min=0), lm_flat, temperature, lmbda)
                probs = mixed.view(seq_len, b2).transpose(0, 1)
                recall = rec.view(seq_len, b2).transpose(0, 1)
        elif alphas:                                            # the ratio alone: one point per alpha, no kNN term
            grid = ops.logp_mix(gnn.reshape(-1), base.reshape(-1), alphas).view(-1, bsz, tsz)
        if use_knn and not sweep:
            queries = h["queries"]
            seq_len, b2, hidden = queries.shape
            # as written (:117): targets in [B, T] order against queries in [T, B] order -- only right for B = 1, the recipe.
            # The driver's --batch-blocks (several of the recipe's one-block batches per launch) asks for the pairing those
            # one-block batches have: targets in the queries' order.
            tq = (orig_target.transpose(0, 1) if sample.get("blockwise_knn") else orig_target.permute(0, 1)).reshape(seq_len * b2)
            lm_flat = probs.transpose(0, 1).reshape(-1)                                 # [T*B] like the queries
            if topk:                                            # one search result, two consumers: the target column and the dense rows
                found = knn_model.search_finish(pending if pending is not None else knn_model.interpolate_begin(queries.contiguous().view(-1, hidden)))
                mixed, _, rec = knn_model.interpolate_finish(found, tq.clamp(min=0), lm_flat, temperature, lmbda)
            elif pending is not None:
                mixed, _, rec = knn_model.interpolate_finish(pending, tq.clamp(min=0), lm_flat, temperature, lmbda)
            else:
                mixed, _, rec = knn_model.interpolate(queries.contiguous().view(-1, hidden), tq.clamp(min=0),
                                                      lm_flat, temperature, lmbda)
            probs = mixed.view(seq_len, b2).transpose(0, 1)
            recall = rec.view(seq_len, b2).transpose(0, 1)
        kt = getattr(self.args, "knn_keytype", None)
        feat = decoder_out[1][kt] if kt in decoder_out[1] else decoder_out[1]["inner_states"][-1]
        top = self._dense_topk(h, found, topk) if topk else None
        if sample.get("ragged") is not None:
            return self._finish_ragged(h, probs, recall, grid, feat, top)
        start_idxs = sample["start_indices"] if "start_indices" in sample else [0] * bsz
        # strip_pad / the [mask] selections of the reference (:156-191) are boolean indexings: each one synchronises the
        # stream (nonzero).  LM eval targets carry no padding (--sample-break-mode none), so ask ONCE per batch -- or not
        # at all when the driver already knows (sample["no_pad_in_target"], set by eval_lm from the whole split) -- and
        # take plain views; the general path below is the reference's, line by line.
        no_pad = sample.get("no_pad_in_target")
        if no_pad is None:
            no_pad = not bool(sample["target"].eq(self.pad).any())
        hypos = []
        starts = [int(v) for v in start_idxs]
        if grid is not None:
            # the grid's log-probs of exactly the positions the hypotheses score, in the hypotheses' order: [G, scored tokens]
            if no_pad and len(set(starts)) == 1:
                h["sweep_logp"] = grid[:, :, starts[0]:].reshape(grid.shape[0], -1)
            else:
                keep = torch.zeros(bsz, tsz, dtype=torch.bool, device=grid.device)
                for i in range(bsz):
                    keep[i, starts[i]:] = True
                if not no_pad:
                    keep &= sample["target"].ne(self.pad)
                h["sweep_logp"] = grid[:, keep]
        # one reduction for the whole batch instead of a sum and a division per hypothesis (64 launches per 32-block batch)
        score_all = probs[:, starts[0]:].sum(dim=1) / (tsz - starts[0]) if no_pad and len(set(starts)) == 1 and tsz > starts[0] else None
        for i in range(bsz):
            s = starts[i]
            if no_pad:
                ref = sample["target"][i, s:]
                tgt_len = ref.numel()
                p_i = probs[i][s:]
                keys_i = feat[s:, i, :]
                rec_i = recall[i, s:] if recall is not None else None
                top_i = [t[i, s:] for t in top] if top is not None else None
            else:
                ref = strip_pad(sample["target"][i, s:], self.pad)
                tgt_len = ref.numel()
                p_i = probs[i][s:s + tgt_len]
                mask = sample["target"][i, s:].ne(self.pad)
                keys_i = feat[s:, i, :][mask]
                rec_i = recall[i, s:][mask] if recall is not None else None
                top_i = [t[i, s:][mask] for t in top] if top is not None else None
            hypos.append([{
                "tokens": ref,
                "score": score_all[i] if score_all is not None else p_i.sum() / tgt_len,
                "attention": None,
                "alignment": None,
                "positional_scores": p_i,
                "dstore_keys": keys_i,
                "knn_recall": rec_i,
            }])
            if top_i is not None:
                hypos[-1][0].update(topk_ids=top_i[0], topk_scores=top_i[1], target_rank=top_i[2])
        return hypos

    def _dense_topk(self, h, found, topk):
        """-> (ids [B, T, N] int64, scores [B, T, N], target_rank [B, T] int32) of the batch: the distribution behind ``probs`` (the
        model's head, its ``orig_prob_ratio`` mixture, and the kNN mix when ``found`` holds the batch's search result), consumed in
        row chunks (``predict.predict_rows``).  Rows run in the queries' [T, B] order, and the kNN branch ranks the target it scores:
        the pairing of ``generate_finish`` as written."""
        from .predict import head_vocab, predict_rows
        model, decoder_out, sample = h["model"], h["decoder_out"], h["sample"]
        if not hasattr(model, "dense_log_probs_rows"):
            raise ValueError("output_topk needs a model with dense_log_probs_rows (GnnLmModel)")
        x, extra = decoder_out[0], decoder_out[1]
        bsz, tsz, d = x.shape
        x2 = x.transpose(0, 1).reshape(tsz * bsz, d).contiguous()
        h2 = None
        if getattr(model, "orig_prob_ratio", 0) > 0 and "orig_x" in extra:
            h2 = extra["orig_x"].transpose(0, 1).reshape(tsz * bsz, -1).contiguous()
        tgt = sample["target"]
        tq = (tgt.transpose(0, 1) if found is None or sample.get("blockwise_knn") else tgt.permute(0, 1)).reshape(-1).clamp(min=0).contiguous()
        knn = None
        if found is not None:
            if not hasattr(h["knn_model"], "mix_labels"):
                raise ValueError("output_topk with a kNN store needs KNNModel.mix_labels (the search result with its labels)")
            knn = dict(h["knn_model"].mix_labels(found), temperature=h["temperature"], lmbda=h["lmbda"])
        ids, scores, rank, _ = predict_rows(lambda r0, r1: model.dense_log_probs_rows(x2[r0:r1], None if h2 is None else h2[r0:r1]),
                                            x2.shape[0], head_vocab(model.adaptive_softmax), tq, topk, knn)
        back = lambda t: t.view(tsz, bsz, *t.shape[1:]).transpose(0, 1)
        return back(ids), back(scores), back(rank)

    def _finish_ragged(self, h, probs, recall, grid, feat, top=None):
        """(this build) The hypotheses of a RAGGED batch: ``sample["ragged"]`` (a ragged.RaggedBatch) cuts the batch's one row of
        packed tokens into blocks; one hypothesis per block, ``tokens`` / ``positional_scores`` of the block's own scored length
        (``start_indices`` tokens of context in front are not scored) -- what ``strip_pad`` leaves of the reference's padded rows
        (:156-191).  Everything per hypothesis is a view; the per-hypothesis sums are ONE segmented sum.  Optional device tables of
        the driver (built once per split): ``sample["scored_rows"]`` (int64, the scored rows of the batch in order; None = every
        row) and ``sample["scored_off"]`` (int, [n_blocks + 1] offsets of the hypotheses inside them).  Also left on the handle:
        ``scored_pos`` (the scored positions' scores, flat), ``hyp_sums`` (float32, one per hypothesis), ``sweep_logp``."""
        from .ragged import packed_rows
        sample = h["sample"]
        rb = sample["ragged"]
        no_pad = sample.get("no_pad_in_target")
        if no_pad is None:
            no_pad = not bool(sample["target"].eq(self.pad).any())
        if not no_pad:
            raise NotImplementedError("padding symbols inside the targets of a ragged batch (the blocks are packed, not padded)")
        off = rb.offsets
        starts = [int(v) for v in sample.get("start_indices", [0] * rb.n_blocks)]
        p, tgt = probs[0], sample["target"][0]
        rows, scored_off = sample.get("scored_rows"), sample.get("scored_off")
        if rows is None and any(starts):                      # (a caller without the driver's tables: built from the host lists)
            import numpy as np
            lens = off[1:] - off[:-1] - np.asarray(starts)
            scored_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(p.device)
            rows = packed_rows(scored_off, torch.from_numpy(off[:-1] + np.asarray(starts)).to(p.device), int(lens.sum()))
        if scored_off is None:
            scored_off = rb.block_off
        scored_off = (scored_off - scored_off[0]).to(torch.int64)
        pos = p if rows is None else p[rows]
        if grid is not None:
            h["sweep_logp"] = grid[:, 0] if rows is None else grid[:, 0][:, rows]
        # segmented sum: differences of a float64 running sum at the hypotheses' boundaries (deterministic, one pass)
        cs = torch.cat([torch.zeros(1, dtype=torch.float64, device=p.device), pos.double().cumsum(0)])
        sums = (cs[scored_off[1:]] - cs[scored_off[:-1]]).float()
        score_all = sums / (scored_off[1:] - scored_off[:-1]).float()
        h["scored_pos"], h["hyp_sums"] = pos, sums
        hypos = []
        for b in range(rb.n_blocks):
            a, e = int(off[b]) + starts[b], int(off[b + 1])
            hypos.append([{
                "tokens": tgt[a:e],
                "score": score_all[b],
                "attention": None,
                "alignment": None,
                "positional_scores": p[a:e],
                "dstore_keys": feat[a:e, 0, :],
                "knn_recall": recall[0, a:e] if recall is not None else None,
            }])
            if top is not None:
                hypos[-1][0].update(topk_ids=top[0][0, a:e], topk_scores=top[1][0, a:e], target_rank=top[2][0, a:e])
        return hypos
