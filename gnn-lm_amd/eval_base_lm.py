"""The base transformer LM path of ``eval_lm`` (no ``--graph``): perplexity of a ``--arch transformer_lm*`` checkpoint over
``DATA/{split}.bin/.idx`` and the "save features" loop of the recipe (gnnlm_scripts/wiki103/prepare_wiki103.sh:69-78):

    python -m gnnlm_amd.eval_lm DATA --path base.pt --sample-break-mode complete --tokens-per-sample 3072 --max-tokens 3072 \\
        --context-window 2560 --softmax-batch 1024 --gen-subset S --dstore-mmap DATA --save-knnlm-dstore --dstore-fp16

Mirror of ``fairseq_cli/eval_lm.py:61-336`` with ``SequenceScorer.generate`` (fairseq/sequence_scorer.py) for one model:

  tokens   the split's stream through the ``.bin/.idx`` reader.  Target = the stream, source = the stream shifted right by one
           with ``eos`` in front of token 0 (``TokenBlockDataset.__getitem__`` with ``include_targets``).
  samples  ``--sample-break-mode none | complete | complete_doc | eos`` through ``eval_lm.sample_blocks``, packed back to back up
           to ``--max-tokens`` rows per batch (a sample longer than that is a batch of its own).
  context  ``--context-window w`` = ``LMContextWindowDataset`` (fairseq/data/lm_context_window_dataset.py): the samples are cut
           at ``tokens_per_sample - w`` and each carries the source tokens in front of it -- as many as the collater keeps:
           min(w, what the previous sample left, tokens_per_sample - its own length) -- which are computed but not scored.  The
           context is taken in CORPUS order.
  scoring  the checkpoint's head on the scored rows only, read in place (row views of the feature buffer, no gather), in pieces
           of at most ``--softmax-batch`` rows; score_sum and count in float64; the reference's two final lines.
  dstore   ``--save-knnlm-dstore --dstore-mmap DIR [--dstore-fp16] [--knn-keytype last_ffn_input]``: row i = token i of the split.

  kNN-LM   ``--knnlm --k --lmbda --temperature --probe --dstore-dir --index-file --knn-sim-func --knn-keytype`` (sequence_scorer.py:
           102-136): the queries are the scored rows of ``extra[knn_keytype]`` if the decoder offers that key, else of
           ``inner_states[-1]``, packed (and scaled to unit length for a cosine index) by ``ops.pack_rows``; the search is enqueued before
           the head and finished after it; ``--lmbda 0`` searches nothing.  Only the scored rows are searched (the reference searches
           the context rows too and drops the results), and the queries are those of ALL scored rows whatever ``--softmax-batch`` is
           (sequence_scorer.py:105-106 takes the last softmax piece's: its own "todo").  ``--sweep-lmbda / -temperature / -k``,
           ``--output-topk``, ``--output-knn-recall`` as on the ``--graph`` path.

Not built here (refused): ``--sweep-orig-prob-ratio`` (no second model to mix), more than one process, ``--graph-capture``.
"""
import logging
import os
import time

import numpy as np
import torch

from . import gen_common, ops

logger = logging.getLogger("gnnlm_amd.eval_lm")

EOS = 2


def shifted_source(tokens, eos=EOS):
    """Source stream of a target stream: shifted right by one, ``eos`` in front (token_block_dataset.py:134-144)."""
    tokens = np.asarray(tokens)
    src = np.empty(tokens.shape[0], dtype=np.int64)
    src[0:1] = eos
    src[1:] = tokens[:-1]
    return src


def context_lengths(lengths, tokens_per_sample, context_window):
    """How many context tokens the collater of LMContextWindowDataset puts in front of every sample, samples taken in order
    (lm_context_window_dataset.py:46-56): ``prev_tokens`` is the last ``w`` tokens of the previous row (its own context included),
    cut from the front so that context + sample <= tokens_per_sample + w.  ``tokens_per_sample`` is the value AFTER the driver's
    ``tokens_per_sample -= w``."""
    out, prev = [], 0
    cap = tokens_per_sample + context_window
    for n in lengths:
        n = int(n)
        prev = max(0, prev - max(0, prev + n - cap))
        out.append(prev)
        prev = min(context_window, prev + n)
    return np.asarray(out, dtype=np.int64)


def check_args(args):
    """Host only, before any device work -> ``(sweep, topk)``: the tuning grid ``(ks, temperatures, lmbdas)`` of --sweep-* or None, and
    N of --output-topk (0: off), both as the --graph driver reads them (``eval_lm.parse_sweep`` / ``check_output_topk``)."""
    from .eval_lm import check_output_topk, parse_sweep
    gen_common.check_knn_store(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("the base LM path runs in one process (WORLD_SIZE > 1 is not built)")
    if getattr(args, "graph_capture", False):
        raise ValueError("--graph-capture is not built for the base LM path")
    if args.save_knnlm_dstore and not args.dstore_mmap:
        raise ValueError("--save-knnlm-dstore needs --dstore-mmap")
    if getattr(args, "sweep_orig_prob_ratio", None) is not None:
        raise ValueError("--sweep-orig-prob-ratio belongs to the --graph path (the base LM has no second model to mix)")
    sweep = parse_sweep(args)                                    # (needs --knnlm; not with --save-knnlm-dstore; k' <= --k <= 1024)
    topk = check_output_topk(args)                               # (not with --sweep-*, --save-knnlm-dstore)
    if args.output_knn_recall and not args.knnlm:
        raise ValueError("--output-knn-recall needs --knnlm")
    gen_common.check_knn_sim_func(args)
    if getattr(args, "reinit_nfeat", False):
        raise ValueError("--reinit-nfeat belongs to the --graph path")
    if args.add_bos_token:
        raise ValueError("--add-bos-token is not built for the base LM path")
    if args.knn_keytype not in (None, "", "last_ffn_input"):
        # (sequence_scorer.py:181-182: any other key type is absent from the decoder's extra and falls back to inner_states[-1])
        logger.info("--knn-keytype %s is not a key of the base LM's outputs: inner_states[-1] is saved (as the reference)", args.knn_keytype)
    return sweep, topk


def main(args, model=None):
    """-> the result dict of ``eval_lm.main`` (score_sum, count, ppl, tokens, seconds, ...) plus ``pos_scores`` (float32 numpy, one
    log-probability per scored token in corpus order) when ``args.keep_pos_scores`` is set (tests, tools)."""
    from .eval_lm import (DstoreWriter, budget_batches, check_break_mode, fairseq_token_stream, report_result, report_sweep, report_topk,
                          sample_blocks, word_output_setup, word_outputs, write_result_json)
    from .ragged import BlockTable, packed_rows
    sweep, topk = check_args(args)
    break_mode = check_break_mode(args)
    w = int(args.context_window)
    if w < 0 or w >= args.tokens_per_sample:
        raise ValueError(f"--context-window {w} must lie in [0, --tokens-per-sample {args.tokens_per_sample})")
    if w > 0 and break_mode == "complete_doc":
        raise ValueError("--context-window with --sample-break-mode complete_doc is not built (the dropped separators leave gaps in the context)")
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    stream_np = fairseq_token_stream(args.data, args.gen_subset)
    if stream_np is None:
        raise FileNotFoundError(f"the base LM reads the binarised split {os.path.join(args.data, args.gen_subset)}.bin/.idx (fairseq's mmap "
                                "dataset): not found or not in that format")
    n_tok = int(stream_np.shape[0])
    if n_tok == 0:
        raise ValueError("the split is empty")
    model = gen_common.load_model(args, device, model)
    if args.fp16:
        logger.info("--fp16: float16 matrix-core GEMMs with float32 accumulation (transformer layers and output layer); embedding, "
                    "attention and LayerNorm stay float32")
    tgt_np = np.asarray(stream_np).astype(np.int64)
    tgt = torch.from_numpy(tgt_np).to(device)
    src = torch.from_numpy(shifted_source(tgt_np)).to(device)
    vocab = model.embed.vocab
    # ---- samples (corpus order), their context, the batches
    T = args.tokens_per_sample - w
    blocks = [(s, e) for _, s, e in sample_blocks(args.data, args.gen_subset, break_mode, T, n_tok, 0)]
    if args.first > 0:
        blocks = blocks[:args.first]
    blocks = blocks[args.shard_id::args.num_shards]
    if not blocks:
        raise ValueError("no sample to score")
    barr = np.asarray(blocks, dtype=np.int64).reshape(-1, 2)
    n_s = barr[:, 1] - barr[:, 0]
    abut = bool(np.all(barr[1:, 0] == barr[:-1, 1]))
    if w > 0 and not abut:
        raise ValueError("--context-window needs consecutive samples (no --num-shards > 1): the context is the text in front of a sample")
    ctx = context_lengths(n_s, T, w) if w > 0 else np.zeros(len(blocks), dtype=np.int64)
    ctx = np.minimum(ctx, barr[:, 0])                            # (never before the start of the split; the recurrence already ensures it)
    rows = ctx + n_s
    bounds = budget_batches(rows.tolist(), int(args.max_tokens or 36000), args.max_sentences)
    table = BlockTable(rows, device, batches=bounds)
    first_dev = torch.from_numpy(np.ascontiguousarray(barr[:, 0] - ctx)).to(device)
    start_dev = torch.from_numpy(np.ascontiguousarray(barr[:, 0])).to(device)
    scored_off = torch.from_numpy(np.concatenate([[0], np.cumsum(n_s)])).to(device)
    keytype = args.knn_keytype or None
    # ---- kNN-LM (sequence_scorer.py:102-136): the store, and the split's tables of ops.pack_rows -- how many rows in front of every
    # sample are context, and where its scored rows start among the batch's (offsets relative to the batch: n + 1 entries per batch)
    search, pack = False, None
    knn = gen_common.load_knn(args, model, device,
                              f"are the base LM's {'last_ffn_input' if keytype == 'last_ffn_input' else 'inner_states[-1]'} rows of")
    if knn is not None:
        search = args.lmbda > 0.0 or sweep is not None                  # :102 -- `--lmbda 0` scores the LM alone; a sweep always searches
        if search and args.knn_sim_func in ("ip", "l2") and hasattr(knn, "keys_home"):
            logger.info(knn.keys_home())
    if search or topk:
        rel = np.concatenate([np.concatenate([[0], np.cumsum(n_s[b0:b1])]) for b0, b1 in bounds])
        pack = {"skip": torch.from_numpy(ctx.astype(np.int32)).to(device), "out_off": torch.from_numpy(rel.astype(np.int32)).to(device),
                "n_bad": torch.zeros(1, device=device, dtype=torch.int32)}
    n_grid = len(ops.grid_points(*sweep)) if sweep else 0
    sweep_acc = torch.zeros(n_grid, device=device, dtype=torch.float64) if sweep else None
    top_parts = []                                                      # (first sample, ids, logp, rank) per batch
    vocab_head = None
    if topk:
        from .predict import head_vocab, predict_rows
        vocab_head = head_vocab(model.head)
    # ---- the datastore writer (eval_lm.DstoreWriter): file names and info.json as for the gcn_feat keys
    save = None
    if args.save_knnlm_dstore:
        save = DstoreWriter(args.dstore_mmap, args.gen_subset, keytype, n_tok, model.d, vocab, bool(args.dstore_fp16))
    want_words = args.output_word_probs or args.output_word_stats
    (symbols, bpe_toks, bpe_len), word_stats = word_output_setup(args), dict()
    acc = torch.zeros(1, device=device, dtype=torch.float64)
    keep = [] if getattr(args, "keep_pos_scores", False) else None
    count, ntok, timers = 0, 0, []
    chunk = int(min(args.softmax_batch, 1 << 30))
    torch.cuda.synchronize()
    wall0 = time.perf_counter()
    for bi, (b0, b1) in enumerate(bounds):
        rb = table.batch(bi)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        c_b, n_b = ctx[b0:b1], n_s[b0:b1]
        has_ctx = bool(c_b.any())
        if not has_ctx and (b1 - b0 == 1 or bool(np.all(barr[b0 + 1:b1, 0] == barr[b0:b1 - 1, 1]))):
            tokens = src[int(barr[b0, 0]):int(barr[b1 - 1, 1])]                    # back-to-back samples: a view
        else:
            tokens = src[packed_rows(rb.block_off, first_dev[b0:b1], rb.n_tok)]
        want_keys = save is not None or search
        x, extra = model.extract_features(tokens.contiguous(), rb, want_inner=want_keys and keytype != "last_ffn_input",
                                          want_ffn_input=want_keys and keytype == "last_ffn_input", check=False)
        n_scored = int(n_b.sum())
        pending = None
        if search:
            # the queries (:105): the scored rows of extra[knn_keytype] if the decoder offers that key, else of inner_states[-1] -- the
            # context rows are not searched.  One launch packs them, and scales them for a cosine index; without a context the buffer
            # already is the query matrix.  The search is enqueued BEFORE the head, its one host read is waited for after it.
            feats = extra.get(keytype) if keytype else None
            if feats is None:
                feats = extra["inner_states"][-1]
            cosine = bool(getattr(knn, "cosine", False))
            queries = feats
            if has_ctx or cosine:
                rows_q, unit_q = ops.pack_rows(feats, rb.block_off, pack["skip"][b0:b1] if has_ctx else None, pack["out_off"][b0 + bi:b1 + bi + 1],
                                               model.d, want_rows=not cosine, want_unit=cosine, n_bad=pack["n_bad"],
                                               out=(torch.empty(n_scored, model.d, device=device) if not cosine else None,
                                                    torch.empty(n_scored, model.d, device=device) if cosine else None))
                queries = unit_q if cosine else rows_q
            pending = knn.interpolate_begin(queries, unit=True) if cosine else knn.interpolate_begin(queries)
        if b1 - b0 == 1 or bool(np.all(barr[b0 + 1:b1, 0] == barr[b0:b1 - 1, 1])):
            target = tgt[int(barr[b0, 0]):int(barr[b1 - 1, 1])]
        else:
            target = tgt[packed_rows(scored_off[b0:b1 + 1], start_dev[b0:b1], n_scored)]
        # the scored rows of the batch, as (first row, rows) runs of the feature buffer: everything without a context, else one
        # run per sample -- the head reads them in place
        runs = [(0, rb.n_tok)] if not has_ctx else [(int(rb.offsets[j] + c_b[j]), int(n_b[j])) for j in range(b1 - b0)]
        logp = torch.empty(n_scored, device=device, dtype=torch.float32)
        o = 0
        for r0, n in runs:
            for c0 in range(0, n, chunk):
                c1 = min(n, c0 + chunk)
                logp[o + c0:o + c1] = model.target_logp(x[r0 + c0:r0 + c1], target[o + c0:o + c1])
            o += n
        recall, found = None, None
        if pending is not None:
            # one search result, up to three consumers: the grid, the run's own setting, the dense rows of --output-topk
            found = knn.search_finish(pending) if sweep or topk else pending
            lm_logp = logp
            if sweep:
                ops.rows_sum_f64(knn.interpolate_grid_finish(found, target, lm_logp, *sweep)[0], sweep_acc)
            if args.lmbda > 0.0:                                                  # (a sweep at --lmbda 0: the scores stay the LM's)
                logp, _, recall = knn.interpolate_finish(found, target, lm_logp, args.temperature, args.lmbda)
            else:
                found = None
        if topk:
            xs = x
            if has_ctx:                                                          # the scored rows of the features, contiguous for the chunks
                xs = ops.pack_rows(x, rb.block_off, pack["skip"][b0:b1], pack["out_off"][b0 + bi:b1 + bi + 1], model.d, n_bad=pack["n_bad"],
                                   out=(torch.empty(n_scored, model.d, device=device), None))[0]
            mix = None if found is None else dict(knn.mix_labels(found), temperature=args.temperature, lmbda=args.lmbda)
            t_ids, t_logp, t_rank, _ = predict_rows(lambda r0, r1: model.head.log_probs(xs[r0:r1]), n_scored, vocab_head, target, topk, mix)
            top_parts.append((b0, t_ids.to(torch.int32), t_logp, t_rank))
        ops.masked_sum_f64(logp, None, acc)                                       # score_sum, in float64
        count += n_scored
        ntok += rb.n_tok
        ev1.record()
        timers.append((ev0, ev1))
        if keep is not None:
            keep.append(logp)
        if save is not None:
            keys = extra.get(keytype) if keytype else None
            if keys is None:
                keys = extra["inner_states"][-1]                                 # sequence_scorer.py:181-182
            if has_ctx:
                keys = torch.cat([keys[r0:r0 + n] for r0, n in runs])
            save.append(keys, target, b0)
        if want_words or bpe_toks is not None:
            hypos, o = [], 0
            for j in range(b1 - b0):
                n = int(n_b[j])
                hypos.append([{"tokens": target[o:o + n], "positional_scores": logp[o:o + n],
                               "knn_recall": None if recall is None else recall[o:o + n]}])
                o += n
            count -= word_outputs(args, hypos, list(range(b0, b1)), symbols, bpe_toks, bpe_len, word_stats)
    score_sum = acc.item()                                                        # the only host sync of a plain run
    model.check_tokens()                                                          # ids outside the vocabulary: counted on the device, read here
    if pack is not None and int(pack["n_bad"].item()):
        raise RuntimeError("the scored-row tables handed to gnnlm_pack_rows were refused on the device (a driver bug: they are built here)")
    sweep_sums = sweep_acc.tolist() if sweep else []
    wall = time.perf_counter() - wall0
    if save is not None:
        save.close()
    gen_time = sum(a.elapsed_time(b) for a, b in timers) / 1e3
    ppl = report_result(score_sum, count, ntok, gen_time)
    sweep_rows = report_sweep(sweep, sweep_sums, count) if sweep else None
    if topk:
        report_topk(args, topk, top_parts)
    if args.output_word_stats:
        for ws in sorted(word_stats.values(), key=lambda x: x.count, reverse=True):
            logger.info(ws)
    res = {"score_sum": score_sum, "count": count, "ppl": ppl, "tokens": ntok, "seconds": gen_time,
           "wall_seconds": wall, "word_stats": word_stats if args.output_word_stats else None, "rank": 0, "world": 1,
           "precision": model.precision, "head": "dense" if type(model.head).__name__ == "DenseSoftmax" else "adaptive", "path": "base_lm"}
    if sweep:
        res["sweep"] = sweep_rows
    write_result_json(getattr(args, "result_json", None), res)
    if keep is not None:
        res["pos_scores"] = torch.cat(keep).cpu().numpy()
    return res
