"""Beam search from the base transformer LM: one K/V cache of ``B * beam`` slots read through a table, the selection on the device.

    python -m gnnlm_amd.beam_search DATA --path base.pt --gen-subset test --n-prompts 8 --prompt-len 32 --max-len-b 64 \\
        [--beam 5] [--nbest 1] [--lenpen 1] [--unnormalized] [--min-len 1] [--temperature 1] [--unkpen X] [--fp16] [--score-prompt] \\
        [--diverse-beam-groups G --diverse-beam-strength 0.5 | --diversity-rate R] \\
        [--knnlm --k 1024 --lmbda 0.25 --knn-temperature 1 --probe 32 --dstore-dir D --index-file F --knn-sim-func do_not_recomp_ip]

Mirror of ``SequenceGenerator`` (fairseq/sequence_generator.py) with ``search.BeamSearch`` (fairseq/search.py:49-85) for one
decoder-only model whose prompt is passed as ``prefix_tokens`` (``LanguageModelingTask.inference_step``).  While a prefix is forced
exactly one hypothesis per sentence has a finite score (sequence_generator.py:288-295 with search.py:63-66), so the reference's run
over a prompt of p tokens is: prefill the prompt once per sentence, take the first selection from ONE row per sentence, start that
row at the prompt's cumulative log-probability, count length from p.  That is the loop here, for ``max_new`` = n, steps t = 0 .. n:

  rows      t = 0: the prefill's last row of every prompt (B rows); afterwards the ``B * beam`` rows of the step
  lprobs    ``Generator.next_log_probs`` (temperature, the optional kNN mix, ``pad = -inf``, the unk penalty); NaN counts as absent
  rules     t == n: every column but ``eos`` is -inf (the forced ``eos`` at max_len, sequence_generator.py:283-285); otherwise
            ``len0[b] + t < min_len`` forbids ``eos`` for sentence b (:315-317)
  top       ``ops.topk_merge`` with k = 2 * beam
  select    ``ops.beam_select``: candidates, finalization, survivors, the table of cache slots, ``finished`` / ``done`` -- one launch;
            with ``--diverse-beam-groups`` (``search.DiverseBeamSearch``, search.py:105-164) or ``--diversity-rate``
            (``search.DiverseSiblingsSearch``, :291-353) ``ops.beam_select_diverse``, the same launch with the candidates drawn group
            by group under the Hamming penalty, or with the sibling penalty
  step      ``TransformerLM.step(next, cache, src=table)`` unless t == n

Hypothesis j of sentence b is cache sequence ("slot") ``b * beam + j``; key row u of a hypothesis lives in slot ``table[slot, u]``, so
what the reference does with ``reorder_incremental_state`` -- an index-select of every layer's K and V by parent -- is a permutation of
4-byte table entries, and a sentence's prompt is stored once (slot ``b * beam``).  ``finished`` is looked at every 16 steps and at
the end.  On the host: score = raw / (len0 + length) ** lenpen (raw with ``unnormalized``), ``positional_scores`` the differences of
the cumulative history, a stable sort by score descending, ``nbest`` returned.

Not the reference's: when MORE than ``beam`` of a step's 2 * beam candidates are ``eos`` the reference carries the surplus as
ignored hypotheses; here the slots without a survivor are dead (``pad``, -inf).  Refused by name: ``--sampling``, ``--sampling-topp``,
``--no-repeat-ngram-size``, ``--graph``, ``--sweep-*``, more than one process, ``2 * beam > V - 1``, ``--beam`` > 32, ``--nbest`` > beam,
``--score-prompt`` with ``--knnlm``, a negative ``--diverse-beam-strength`` and a ``--diversity-rate`` in (-1, 0): the selection is made
from each hypothesis's best 2 * beam tokens, which holds every candidate a penalty can leave among the best only if penalties lower.
``--diversity-rate`` -1 (the default) or below is "off" and 0 is plain beam search, as in the reference (fairseq_task.py:257).
"""
import logging
import sys

import numpy as np
import torch

from . import gen_common, ops
from .generate import DONE_EVERY, EOS, PAD, UNK, Generator, read_prompts

logger = logging.getLogger("gnnlm_amd.beam_search")

MAX_BEAM = 32


class BeamState:
    """The device state of ``gnnlm_beam_select`` for B sentences: see :func:`ops.beam_select`.  ``len`` / ``done`` are the cache's."""

    def __init__(self, B, beam, max_new, cache_len, cache_done, device, score0=None):
        self.beam, self.max_new = int(beam), int(max_new)
        S, T1 = B * beam, max_new + 1
        i32 = lambda *s: torch.zeros(*s, device=device, dtype=torch.int32)
        self.score = torch.zeros(B, beam, device=device, dtype=torch.float32)
        if score0 is not None:
            self.score[:, 0] = torch.as_tensor(np.asarray(score0, np.float32), device=device)
        self.t, self.finished, self.fin_n = i32(B), i32(B), i32(B)
        self.len, self.done = cache_len, cache_done
        self.next = torch.full((S,), PAD, device=device, dtype=torch.int64)
        self.parent = i32(S)
        self.hist_tok = torch.full((B, T1, beam), PAD, device=device, dtype=torch.int64)
        self.hist_par = i32(B, T1, beam)
        self.hist_score = torch.zeros(B, T1, beam, device=device, dtype=torch.float32)
        self.fin_tok = torch.full((B, beam, T1), PAD, device=device, dtype=torch.int64)
        self.fin_cum = torch.zeros(B, beam, T1, device=device, dtype=torch.float32)
        self.fin_len = i32(B, beam)
        self.fin_score = torch.zeros(B, beam, device=device, dtype=torch.float32)


def finish(fin_n, fin_tok, fin_cum, fin_len, fin_score, score0, len0, lenpen=1.0, unnormalized=False, nbest=None):
    """Host: the finalized hypotheses as ``gnnlm_beam_select`` left them (numpy) -> per sentence a list of dicts ``tokens`` (int64, the
    ``eos`` included), ``score``, ``raw`` (the cumulative log-probability, float32), ``positional_scores`` (float32), best first."""
    out = []
    for b in range(len(fin_n)):
        hyps = []
        for f in range(int(fin_n[b])):
            n = int(fin_len[b, f])
            cum = fin_cum[b, f, :n].astype(np.float32)
            raw = np.float32(fin_score[b, f])
            pos = cum - np.concatenate([[np.float32(score0[b])], cum[:-1]]).astype(np.float32)
            score = raw if unnormalized else np.float32(raw / np.float32((int(len0[b]) + n) ** lenpen))
            hyps.append({"tokens": fin_tok[b, f, :n].astype(np.int64), "score": float(score), "raw": float(raw), "positional_scores": pos})
        hyps = sorted(hyps, key=lambda h: h["score"], reverse=True)          # stable, as sequence_generator.py:501
        out.append(hyps[:nbest] if nbest else hyps)
    return out


class BeamGenerator(Generator):
    @staticmethod
    def check_beam(max_new, beam, nbest, temperature, V):
        gen_common.check_decode(max_new, temperature)
        if beam < 1 or beam > MAX_BEAM:
            raise ValueError(f"--beam {beam}: between 1 and {MAX_BEAM} (gnnlm_beam_select)")
        if 2 * beam > V - 1:
            raise ValueError(f"--beam {beam}: a step draws 2 * beam candidates and never pad, so 2 * beam <= V - 1 = {V - 1}")
        if nbest is not None and not 1 <= nbest <= beam:
            raise ValueError(f"--nbest {nbest}: between 1 and --beam {beam}")

    @staticmethod
    def check_diverse(beam, groups, strength, diversity_rate):
        if groups < 1 or beam % groups:
            raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
        if not 0 <= strength < float("inf") or not 0 <= diversity_rate < float("inf"):
            raise ValueError("--diverse-beam-strength / --diversity-rate: a penalty is finite and not negative")
        if groups > 1 and diversity_rate != 0:
            raise ValueError("Provided Search parameters are mutually exclusive.")

    def start(self, prompts, max_new, beam, temperature=1.0, unk_penalty=0.0, score0=None, len0=None, score_prompt=False):
        """Prefill the prompts once per sentence into a cache of ``B * beam`` slots -> dict(cache, state, table, x, extra, len0, score0,
        want_ffn): everything :meth:`advance` needs; ``x`` / ``extra`` are the B rows the first selection is made from."""
        dev, B = self.lm.device, len(prompts)
        cache, tokens, lens, x, extra, last, want_ffn = self.prefill(prompts, max_new, beam)
        len0 = np.zeros(B, np.int64) if len0 is None else np.asarray(len0, np.int64)
        score0 = np.zeros(B, np.float32) if score0 is None else np.asarray(score0, np.float32)
        if score_prompt:                                     # log p(prompt[1:] | its own past), as the reference's forced prefix steps score it
            if self.knn is not None and self.lmbda > 0.0:
                raise ValueError("--score-prompt with --knnlm is not built (the prompt's rows are not searched)")
            off = np.concatenate([[0], np.cumsum(lens)])
            rows = np.concatenate([np.arange(off[b], off[b + 1] - 1) for b in range(B)]).astype(np.int64)
            tgt = np.concatenate([np.arange(off[b] + 1, off[b + 1]) for b in range(B)]).astype(np.int64)
            score0, len0 = np.zeros(B, np.float32), lens - 1
            if len(rows):
                xr = x[torch.from_numpy(rows).to(dev)]
                lp = self._head(temperature).target_log_prob(xr if temperature == 1.0 else xr / temperature, tokens[torch.from_numpy(tgt).to(dev)])
                lp = lp.double().cpu().numpy() - unk_penalty * (tokens.cpu().numpy()[tgt] == UNK)
                score0 = np.asarray([lp[off[b] - b:off[b + 1] - b - 1].sum() for b in range(B)], np.float32)
        x, extra = gen_common.last_rows(x, extra, last)
        state = BeamState(B, beam, max_new, cache.len, cache.done, dev, score0)
        table = torch.zeros(B * beam, cache.cap, device=dev, dtype=torch.int32)
        cand = (torch.empty(B * beam, 2 * beam, device=dev, dtype=torch.float32), torch.empty(B * beam, 2 * beam, device=dev, dtype=torch.int64))
        return dict(cache=cache, state=state, table=table, x=x, extra=extra, len0=len0, score0=score0, want_ffn=want_ffn, cand=cand, B=B)

    def candidates(self, run, x, extra, t, min_len=1, temperature=1.0, unk_penalty=0.0):
        """The rows' log-probs under the step's rules -> the sorted top 2 * beam of every row, in ``run['cand']`` (views of its first rows)."""
        state, B = run["state"], run["B"]
        lp = self.next_log_probs(x, extra, float(temperature), float(unk_penalty))
        lp.masked_fill_(lp != lp, float("-inf"))
        per = x.shape[0] // B
        if t == state.max_new:
            keep = lp[:, EOS].clone()
            lp.fill_(float("-inf"))
            lp[:, EOS] = keep
        else:
            short = np.nonzero(run["len0"] + t < min_len)[0]
            if len(short):
                rows = (torch.from_numpy(short).to(lp.device)[:, None] * per + torch.arange(per, device=lp.device)[None, :]).reshape(-1)
                lp[rows, EOS] = float("-inf")
        val, idx = run["cand"][0][:x.shape[0]], run["cand"][1][:x.shape[0]]
        ops.topk_merge(lp, val, idx, init=True)
        return val, idx

    def generate(self, prompts, max_new, beam=5, nbest=None, lenpen=1.0, unnormalized=False, min_len=1, temperature=1.0, unk_penalty=0.0,
                 score0=None, len0=None, score_prompt=False, groups=1, strength=0.5, diversity_rate=0.0):
        """prompts: a list of non-empty lists of token ids, fed as they are -> per prompt the ``nbest`` (default: all finalized, at most
        ``beam``) hypotheses, best first: dicts of ``tokens`` (numpy int64: up to ``max_new`` new tokens and the ``eos``), ``score``, ``raw``,
        ``positional_scores``.  ``score0`` / ``len0`` [B]: the prompts' cumulative log-probability and length as the reference counts them
        (default zeros: a hypothesis is scored over what was generated); ``score_prompt`` computes both from the prefill.  ``groups`` > 1:
        diverse beam search, ``beam / groups`` hypotheses per group, a token costs ``strength`` for every earlier group's candidate that
        chose it at the step; ``diversity_rate`` > 0: the c-th best continuation of a hypothesis loses ``c * diversity_rate``.  The
        penalties stay in the scores.  With ``groups`` 1 and ``diversity_rate`` 0 the plain selection is launched."""
        lm = self.lm
        self.check_beam(max_new, beam, nbest, float(temperature), self.vocab)
        self.check_diverse(beam, groups, strength, diversity_rate)
        diverse = groups > 1 or diversity_rate != 0
        run = self.start(prompts, max_new, beam, float(temperature), float(unk_penalty), score0, len0, score_prompt)
        cache, state, table = run["cache"], run["state"], run["table"]
        x, extra = run["x"], run["extra"]
        for t in range(max_new + 1):
            val, idx = self.candidates(run, x, extra, t, min_len, temperature, unk_penalty)
            if diverse:
                ops.beam_select_diverse(val, idx, state, src=table, eos=EOS, pad=PAD, groups=groups, strength=strength, rate=diversity_rate)
            else:
                ops.beam_select(val, idx, state, src=table, eos=EOS, pad=PAD)
            if t == max_new or ((t + 1) % DONE_EVERY == 0 and bool(state.finished.all())):
                break
            x, extra = lm.step(state.next, cache, want_ffn_input=run["want_ffn"], src=table)
        lm.check_tokens()
        if int(cache.n_bad.item()):
            raise RuntimeError("beam search: a row left the cache's range or followed a table entry outside it")
        fin_n = state.fin_n.cpu().numpy()
        if not bool(state.finished.all()) or (fin_n < 1).any():
            raise RuntimeError("beam search: a sentence ended without a finalized hypothesis (non-finite log-probabilities)")
        self.last_run = run
        return finish(fin_n, state.fin_tok.cpu().numpy(), state.fin_cum.cpu().numpy(), state.fin_len.cpu().numpy(),
                      state.fin_score.cpu().numpy(), run["score0"], run["len0"], lenpen, unnormalized, nbest)


# ------------------------------------------------------------------------------------------------ the driver
def get_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m gnnlm_amd.beam_search", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    gen_common.add_common_args(p, beam=5, max_len_help="new tokens per hypothesis before the forced eos",
                               out_help="write tokens / scores / positional scores / lengths / prompts to this .npz")
    p.add_argument("--nbest", type=int, default=1)
    p.add_argument("--lenpen", type=float, default=1.0)
    p.add_argument("--unnormalized", action="store_true")
    p.add_argument("--score-prompt", action="store_true", help="score and count the prompt as the reference's prefix_tokens run does")
    # the reference's defaults (-1, 0.5, -1.0) are what diverse_args / check_args read when a flag is not given: a flag left out
    # leaves no name in the namespace, so the namespace of a plain run is what it was before these flags
    S = argparse.SUPPRESS
    p.add_argument("--diverse-beam-groups", type=int, default=S, help="diverse beam search with this many groups (default -1: off)")
    p.add_argument("--diverse-beam-strength", type=float, default=S, help="what a token costs a group per earlier group's candidate that chose it (default 0.5)")
    p.add_argument("--diversity-rate", type=float, default=S, help="sibling penalty: the c-th best continuation of a hypothesis loses c * rate (default -1.0: off)")
    return p


def diverse_args(args):
    """-> (groups, strength, diversity_rate) as :meth:`BeamGenerator.generate` takes them.  The flags are read with their defaults when the
    namespace lacks them; groups <= 0 and a rate <= -1 mean "off" (fairseq_task.py:247, :257), a rate of 0 is plain beam search."""
    groups = getattr(args, "diverse_beam_groups", -1)
    rate = getattr(args, "diversity_rate", -1.0)
    return (groups if groups > 0 else 1), getattr(args, "diverse_beam_strength", 0.5), (rate if rate > 0 else 0.0)


def check_args(args):
    """Host only, before any device work: what this build does not compute is refused with the flag's name."""
    if args.sampling or args.sampling_topk > 0:
        raise ValueError("--sampling: beam search does not sample (python -m gnnlm_amd.generate does, at beam 1)")
    if not args.sampling_topp <= 0:                          # (a NaN too)
        raise ValueError("--sampling-topp: beam search does not sample (python -m gnnlm_amd.generate does, at beam 1)")
    gen_common.check_unbuilt(args)
    if args.beam > MAX_BEAM or args.beam < 1:
        raise ValueError(f"--beam {args.beam}: between 1 and {MAX_BEAM}")
    if not 1 <= args.nbest <= args.beam:
        raise ValueError(f"--nbest {args.nbest}: between 1 and --beam {args.beam}")
    groups, strength, rate = getattr(args, "diverse_beam_groups", -1), getattr(args, "diverse_beam_strength", 0.5), getattr(args, "diversity_rate", -1.0)
    if groups > 0 and rate > 0:                              # (fairseq_task.py:229-241; sampling is refused above)
        raise ValueError("Provided Search parameters are mutually exclusive.")
    if groups > 0 and args.beam % groups:
        raise ValueError("DiverseBeamSearch requires --beam to be divisible by the number of groups")
    if not 0 <= strength < float("inf"):
        raise ValueError(f"--diverse-beam-strength {strength}: finite and not negative (a negative penalty can lift a token from outside a hypothesis's best 2 * beam)")
    if -1 < rate < 0 or rate != rate or rate == float("inf"):
        raise ValueError(f"--diversity-rate {rate}: the reference runs DiverseSiblingsSearch with any rate above -1; a rate in (-1, 0) rewards siblings "
                         "and is not built (the candidates are each hypothesis's best 2 * beam tokens); -1 is off, 0 is plain beam search")
    if args.max_len_b < 1:
        raise ValueError("--max-len-b must be at least 1")
    if not args.temperature > 0:
        raise ValueError("--temperature must be greater than 0")
    if args.score_prompt and args.knnlm:
        raise ValueError("--score-prompt with --knnlm is not built (the prompt's rows are not searched)")
    gen_common.check_knn_and_prompts(args)


def main(args, model=None, file=None):
    """-> dict(hypotheses (per prompt, best first), prompts).  Prints fairseq's ``S-i`` / ``H-i`` / ``P-i`` lines to ``file`` (stdout)."""
    check_args(args)
    file = sys.stdout if file is None else file
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    prompts = read_prompts(args)
    model = gen_common.load_model(args, device, model)
    logger.info("%d prompt(s), beam %d, up to %d new tokens each, precision %s", len(prompts), args.beam, args.max_len_b, model.precision)
    knn = gen_common.load_knn(args, model, device)
    g = BeamGenerator(model, knn, args.knn_keytype, k=args.k if args.knnlm else 0, lmbda=args.lmbda if args.knnlm else 0.0,
                      knn_temperature=args.knn_temperature)
    groups, strength, rate = diverse_args(args)
    hyps = g.generate(prompts, args.max_len_b, beam=args.beam, nbest=args.nbest, lenpen=args.lenpen, unnormalized=args.unnormalized,
                      min_len=args.min_len, temperature=args.temperature, unk_penalty=args.unkpen, score_prompt=args.score_prompt,
                      groups=groups, strength=strength, diversity_rate=rate)
    word = gen_common.word_of(args.data)
    for i, p in enumerate(prompts):
        print(f"S-{i}\t" + " ".join(word(t) for t in p[1:]), file=file)
        for h in hyps[i]:
            print(f"H-{i}\t{h['score']}\t" + " ".join(word(int(t)) for t in h["tokens"]), file=file)
            print(f"P-{i}\t" + " ".join(f"{float(v):.4f}" for v in h["positional_scores"]), file=file)
    res = {"hypotheses": hyps, "prompts": prompts, "score0": g.last_run["score0"], "len0": g.last_run["len0"]}
    if args.out:
        n, T1 = args.nbest, args.max_len_b + 1
        tok = np.full((len(prompts), n, T1), PAD, dtype=np.int64)
        pos = np.zeros((len(prompts), n, T1), dtype=np.float32)
        score, raw = np.full((len(prompts), n), -np.inf, dtype=np.float32), np.full((len(prompts), n), -np.inf, dtype=np.float32)
        lengths = np.zeros((len(prompts), n), dtype=np.int64)
        for i, hs in enumerate(hyps):
            for f, h in enumerate(hs):
                m = len(h["tokens"])
                tok[i, f, :m], pos[i, f, :m], score[i, f], raw[i, f], lengths[i, f] = h["tokens"], h["positional_scores"], h["score"], h["raw"], m
        pr, pr_len = gen_common.padded_prompts(prompts)
        np.savez(args.out, tokens=tok, positional_scores=pos, scores=score, raw=raw, lengths=lengths, prompts=pr, prompt_lengths=pr_len)
    return res


def cli_main(argv=None):
    gen_common.cli_main(main, get_parser, argv)


if __name__ == "__main__":
    cli_main()
