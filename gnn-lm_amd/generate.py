"""Generate from the base transformer LM: K/V-cache decoding, greedy, top-k or nucleus (top-p) sampling, optionally mixed with kNN.

    python -m gnnlm_amd.generate DATA --path base.pt --gen-subset test --n-prompts 8 --prompt-len 32 --max-len-b 64 \\
        [--sampling --sampling-topk 10 | --sampling --sampling-topp 0.9] [--temperature 0.8] [--unkpen X] [--seed 1] [--fp16] \\
        [--knnlm --k 1024 --lmbda 0.25 --knn-temperature 1 --probe 32 --dstore-dir D --index-file F --knn-sim-func do_not_recomp_ip]

Mirror of ``SequenceGenerator`` (fairseq/sequence_generator.py) with ``search.Sampling`` (fairseq/search.py:167-288) at beam 1 for
one decoder-only model.  The loop:

  prefill   ``TransformerLM.prefill`` over the packed prompts fills the K/V cache; the last row of every prompt goes on.
  head      ``head.log_probs`` of the rows divided by the temperature -- sequence_generator.py:572-573 divides ``decoder_out[0]``,
            which is the features under the adaptive softmax and the logits (rows and bias) under the plain output layer.
  kNN       optional: the rows' ``extra[knn_keytype]`` (else ``inner_states[-1]``) searched through the ``KNNModel``'s index, mixed by
            ``ops.knn_mix_dense`` exactly as ``predict.predict_rows`` feeds it.
  rules     ``lprobs[:, pad] = -inf`` and ``lprobs[:, unk] -= unk_penalty`` (sequence_generator.py:279-280).
  pick      ``ops.topk_merge`` with k = ``sampling_topk`` (1 when greedy), then ``ops.sample_topk`` with one uniform number per row from
            a seeded device generator.  With ``--sampling-topp P``: one ``ops.sample_topp`` on the dense rows instead -- the nucleus
            of ``search.Sampling._sample_topp`` (search.py:174-217: the shortest prefix of the sorted row whose probabilities, not
            renormalised, sum to P or more), found without a sort, and one draw from it; no top-k buffers.  P >= 1 samples from
            (essentially) the whole vocabulary: every token with a finite log-probability.
  step      ``TransformerLM.step`` appends the picks; back to head.

Without kNN the loop reads nothing back per token: ``done`` is looked at every 16 steps and at the end.

Refused by name, never approximated: ``--beam`` > 1, ``--sampling`` without ``--sampling-topk`` or ``--sampling-topp``, both of them at
once (the reference lets top-p win silently), ``--sampling-topp`` without ``--sampling`` (fairseq_task.py:243) or NaN,
``--sampling-topk`` > 2048, ``--no-repeat-ngram-size``, ``--min-len`` != 1, ``--graph``, ``--sweep-*``, more than one process.
"""
import argparse
import logging
import os
import sys

import numpy as np
import torch

from . import gen_common, ops
from .gen_common import EOS, PAD, UNK
from .predict import MAX_TOPK, head_vocab

logger = logging.getLogger("gnnlm_amd.generate")

DONE_EVERY = 16                 # steps between two looks at `done`


class Generator:
    def __init__(self, lm, knn=None, knn_keytype=None, k=0, lmbda=0.0, knn_temperature=1.0):
        """lm: a ``TransformerLM`` with a head.  knn: a ``KNNModel`` (or anything with its ``interpolate_dense``) or None;
        ``lmbda`` / ``knn_temperature`` / ``k`` are the mixture's settings (``k`` 0: the model's own)."""
        if lm.head is None:
            raise ValueError("Generator: this TransformerLM was built without an output layer")
        self.lm, self.knn, self.knn_keytype = lm, knn, knn_keytype or None
        self.k, self.lmbda, self.knn_temperature = int(k), float(lmbda), float(knn_temperature)
        self.vocab = head_vocab(lm.head)
        self._cool = {}

    @property
    def head(self):
        """The output layer the picks are made from (``generate_gnn.GnnGenerator``: the GNN-LM's)."""
        return self.lm.head

    def _head(self, temperature):
        """The head that gives log_softmax(decoder_out / temperature) of rows ALREADY divided by it: itself, or -- the plain output
        layer with a bias -- a twin whose bias is divided too."""
        head = self.head
        if temperature == 1.0 or getattr(head, "bias", None) is None:
            return head
        if temperature not in self._cool:
            twin = type(head)(head.weight, head.bias / temperature)
            self._cool = {temperature: twin}
        twin = self._cool[temperature]
        twin.gemm_precision = head.gemm_precision
        return twin

    def next_log_probs(self, x, extra, temperature=1.0, unk_penalty=0.0):
        """Rows ``x`` [B, d] (and the ``extra`` they came with) -> the log-probs the pick is made from, [B, V] f32."""
        rows = x if temperature == 1.0 else x / temperature
        lp = self._head(temperature).log_probs(rows)
        if self.knn is not None and self.lmbda > 0.0:
            q = extra.get(self.knn_keytype) if self.knn_keytype else None
            if q is None:
                q = extra["inner_states"][-1]
            lp = self.knn.interpolate_dense(q.contiguous(), lp, self.knn_temperature, self.lmbda, k=self.k)
        lp[:, PAD] = float("-inf")
        if unk_penalty:
            lp[:, UNK] -= unk_penalty
        return lp

    @staticmethod
    def check(max_new, sampling, sampling_topk, temperature, V, sampling_topp=-1.0):
        """-> the k of the top-k pick (1 when greedy; unused under top-p).  ``sampling_topp`` <= 0 is off (search.py:228)."""
        gen_common.check_decode(max_new, temperature)
        if sampling_topp != sampling_topp:
            raise ValueError("--sampling-topp must be a number (NaN given)")
        if sampling_topp > 0:
            if not sampling:
                raise ValueError("--sampling-topp requires --sampling")
            if sampling_topk > 0:
                raise ValueError("--sampling-topp with --sampling-topk: give one of the two")
            return 1
        if sampling and sampling_topk < 1:
            raise ValueError("--sampling needs --sampling-topk K or --sampling-topp P")
        if sampling and sampling_topk > MAX_TOPK:
            raise ValueError(f"--sampling-topk {sampling_topk}: at most {MAX_TOPK} (gnnlm_topk_merge's k)")
        return min(sampling_topk, V) if sampling else 1

    def prefill(self, prompts, room, beam=None):
        """Pack the prompts and prefill them into a new cache with ``room`` rows behind the longest -> ``(cache, tokens, lens, x, extra,
        last, want_ffn)``: ``x`` / ``extra`` over ALL packed rows, ``last`` the rows the first pick is made from
        (``gen_common.last_rows``).  ``beam``: the cache has ``beam`` slots per prompt, the prompt stored once, in the first."""
        lm = self.lm
        tokens, off, lens, last = gen_common.pack_prompts(prompts, lm.device)
        cache = lm.new_cache(len(prompts) * (beam or 1), int(lens.max()) + room)
        into = cache if beam is None else cache.prompt_view(beam)
        want_ffn = self.knn is not None and self.knn_keytype == "last_ffn_input"
        x, extra = lm.prefill(tokens, off, into, want_ffn_input=want_ffn, check=False)
        if beam is not None:
            cache.spread(into)
        return cache, tokens, lens, x, extra, last, want_ffn

    # the two places where the loop of generate() meets the model: generate_gnn.GnnGenerator puts the graph decoder behind them
    def _start(self, prompts, max_new):
        """Prefill -> ``(cache, x, extra)``: the base LM's cache and the rows the first pick is made from."""
        cache, _, _, x, extra, last, self._want_ffn = self.prefill(prompts, max_new - 1)
        x, extra = gen_common.last_rows(x, extra, last)
        return cache, x, extra

    def _advance(self, nxt, cache):
        """Append the picks -> ``(x, extra)`` of the new rows."""
        return self.lm.step(nxt, cache, want_ffn_input=self._want_ffn)

    def _out_of_range(self, cache):
        """Rows that left a cache's range, over the whole run (one read at the end)."""
        return int(cache.n_bad.item())

    def generate(self, prompts, max_new, sampling=False, sampling_topk=-1, temperature=1.0, unk_penalty=0.0, seed=None, sampling_topp=-1.0):
        """prompts: a list of non-empty lists of token ids, fed as they are -> ``(tokens int64 [B, max_new], logp f32 [B, max_new],
        lengths int64 [B])`` on the device: row b's continuation is ``tokens[b, :lengths[b]]`` (its ``eos`` included when it came), ``pad``
        behind it; ``logp`` the picks' own log-probabilities.  ``sampling_topp`` > 0 (with ``sampling``): nucleus sampling; the mean
        nucleus size over the picks made is left in ``self.mean_nucleus``."""
        lm, dev = self.lm, self.lm.device
        k = self.check(max_new, sampling, sampling_topk, float(temperature), self.vocab, float(sampling_topp))
        topp = float(sampling_topp) if sampling and sampling_topp > 0 else 0.0
        cache, x, extra = self._start(prompts, max_new)
        B = len(prompts)
        out = torch.full((B, max_new), PAD, dtype=torch.int64, device=dev)
        out_lp = torch.zeros(B, max_new, dtype=torch.float32, device=dev)
        best_val = None if topp else torch.empty(B, k, dtype=torch.float32, device=dev)
        best_id = None if topp else torch.empty(B, k, dtype=torch.int64, device=dev)
        nxt = torch.empty(B, dtype=torch.int64, device=dev)
        nxt_lp = torch.zeros(B, dtype=torch.float32, device=dev)
        gen = None
        if sampling:
            gen = torch.Generator(device=dev)
            gen.manual_seed(int(seed) if seed is not None else 1)
        n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if topp:
            n_keep = torch.zeros(B, dtype=torch.int32, device=dev)      # this step's nucleus sizes (0 for a row that made no pick)
            keep_sum = torch.zeros(2, dtype=torch.int64, device=dev)    # nucleus sizes summed, picks made
        self.mean_nucleus = None
        for t in range(max_new):
            lp = self.next_log_probs(x, extra, float(temperature), float(unk_penalty))
            u = torch.rand(B, generator=gen, device=dev, dtype=torch.float32) if sampling else None
            nxt_lp.zero_()
            if topp:
                n_keep.zero_()
                ops.sample_topp(lp, topp, u, pad=PAD, eos=EOS, done=cache.done, n_bad=n_bad, out=nxt, out_logp=nxt_lp, n_keep=n_keep)
                keep_sum[0] += n_keep.sum()
                keep_sum[1] += (n_keep > 0).sum()
            else:
                ops.topk_merge(lp, best_val, best_id, init=True)
                ops.sample_topk(best_val, best_id, u=u, pad=PAD, eos=EOS, done=cache.done, n_bad=n_bad, out=nxt, out_logp=nxt_lp)
            out[:, t] = nxt
            out_lp[:, t] = nxt_lp
            if t == max_new - 1 or ((t + 1) % DONE_EVERY == 0 and bool(cache.done.all())):
                break
            x, extra = self._advance(nxt, cache)
        lm.check_tokens()
        if int(n_bad.item()) or self._out_of_range(cache):
            raise RuntimeError("generate: a row had nothing to pick from (non-finite log-probabilities) or left the cache's range")
        if topp:
            total, picks = (int(v) for v in keep_sum.tolist())
            self.mean_nucleus = total / max(picks, 1)
        is_eos = out == EOS
        first = torch.where(is_eos.any(1), is_eos.int().argmax(1) + 1, torch.full((B,), t + 1, device=dev))
        return out, out_lp, first.to(torch.int64)


# ------------------------------------------------------------------------------------------------ the driver
def get_parser():
    p = argparse.ArgumentParser(prog="python -m gnnlm_amd.generate", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    gen_common.add_common_args(p, beam=1, max_len_help="tokens to generate per prompt (fairseq: max_len = a * src_len + b with a = 0)",
                               out_help="write tokens / logp / lengths / prompts to this .npz")
    p.add_argument("--seed", type=int, default=1)
    return p


def check_args(args):
    """Host only, before any device work: what this build does not compute is refused with the flag's name."""
    if args.beam != 1:
        raise ValueError(f"--beam {args.beam}: this driver decodes at --beam 1 only; beam search is python -m gnnlm_amd.beam_search")
    if args.min_len != 1:
        raise ValueError(f"--min-len {args.min_len} is not built (only --min-len 1)")
    gen_common.check_unbuilt(args)
    Generator.check(args.max_len_b, args.sampling, args.sampling_topk, args.temperature, MAX_TOPK, args.sampling_topp)
    gen_common.check_knn_and_prompts(args)


def read_prompts(args):
    """The prompts as fed: ``eos`` (the sentence start the language-modelling task feeds, token_block_dataset.py:134-144), then the
    tokens of --prompt-ids or of ``--n-prompts`` consecutive pieces of ``--prompt-len`` tokens of the split."""
    if args.prompt_ids is not None:
        try:
            ids = [int(s) for s in args.prompt_ids.split(",") if s.strip()]
        except ValueError:
            raise ValueError(f"--prompt-ids {args.prompt_ids!r}: comma-separated token ids") from None
        return [[EOS] + ids]
    from .eval_lm import fairseq_token_stream
    stream = fairseq_token_stream(args.data, args.gen_subset)
    if stream is None:
        raise FileNotFoundError(f"the prompts are cut from {os.path.join(args.data, args.gen_subset)}.bin/.idx (fairseq's mmap dataset): "
                                "not found or not in that format")
    n = min(args.n_prompts, int(stream.shape[0]) // args.prompt_len)
    if n < 1:
        raise ValueError(f"the split holds fewer than --prompt-len {args.prompt_len} tokens")
    return [[EOS] + [int(t) for t in stream[i * args.prompt_len:(i + 1) * args.prompt_len]] for i in range(n)]


def main(args, model=None, file=None):
    """-> dict(tokens, logp, lengths (numpy), prompts).  Prints fairseq's ``S-i`` / ``H-i`` lines to ``file`` (stdout)."""
    check_args(args)
    file = sys.stdout if file is None else file
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    prompts = read_prompts(args)
    model = gen_common.load_model(args, device, model)
    how = "greedy" if not args.sampling else \
        (f"top-p {args.sampling_topp} (nucleus) sampling" if args.sampling_topp > 0 else f"top-{args.sampling_topk} sampling") + \
        f" at temperature {args.temperature}"
    logger.info("%d prompt(s), up to %d new tokens each, %s, precision %s", len(prompts), args.max_len_b, how, model.precision)
    knn = gen_common.load_knn(args, model, device)
    g = Generator(model, knn, args.knn_keytype, k=args.k if args.knnlm else 0, lmbda=args.lmbda if args.knnlm else 0.0,
                  knn_temperature=args.knn_temperature)
    tokens, logp, lengths = g.generate(prompts, args.max_len_b, sampling=args.sampling, sampling_topk=args.sampling_topk,
                                       temperature=args.temperature, unk_penalty=args.unkpen, seed=args.seed, sampling_topp=args.sampling_topp)
    if g.mean_nucleus is not None:
        logger.info("top-p %s: mean nucleus size %.1f of %d tokens", args.sampling_topp, g.mean_nucleus, g.vocab)
    tokens, logp, lengths = tokens.cpu().numpy(), logp.cpu().numpy(), lengths.cpu().numpy()
    word = gen_common.word_of(args.data)
    for i, p in enumerate(prompts):
        n = int(lengths[i])
        print(f"S-{i}\t" + " ".join(word(t) for t in p[1:]), file=file)
        print(f"H-{i}\t{float(logp[i, :n].astype(np.float64).sum())}\t" + " ".join(word(int(t)) for t in tokens[i, :n]), file=file)
    res = {"tokens": tokens, "logp": logp, "lengths": lengths, "prompts": prompts}
    if args.out:
        pr, pr_len = gen_common.padded_prompts(prompts)
        np.savez(args.out, tokens=tokens, logp=logp, lengths=lengths, prompts=pr, prompt_lengths=pr_len)
    return res


def cli_main(argv=None):
    gen_common.cli_main(main, get_parser, argv)


if __name__ == "__main__":
    cli_main()
