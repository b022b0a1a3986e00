"""Restatements for diverse beam search (tests only; imports neither the package under test nor the reference):

  step_list                the step's candidate list of gnnlm_beam_select_diverse (include/gnnlm.h): groups under the Hamming penalty
                           (search.DiverseBeamSearch) or the sibling penalty (search.DiverseSiblingsSearch), 2 * beam places, an empty
                           place None -- in float32 (the descriptor's arithmetic) or float64
  select_diverse_ref       one step on the arrays of the descriptor, float32: step_list, then finalize / survive / table / finish
  diverse_beam_search_ref  the whole loop around a callable that maps a token history to a log-prob row, float64, over the WHOLE
                           vocabulary of every hypothesis -- not its best 2 * beam tokens, so that a run which agrees with the device
                           also shows that 2 * beam columns are enough
"""
import numpy as np

from beam_ref import EOS, PAD, UNK, walk


def _f32(x):
    return np.float32(x)


def step_list(score, rows, beam, groups=1, strength=0.0, rate=0.0, fl=_f32, margins=None):
    """score[j]: the hypotheses' scores; rows[j]: the candidates (log-prob, token, column) of hypothesis j, len(rows) == 1 at the first
    selection; ``fl`` rounds every intermediate (np.float32 or float).  -> 2 * beam places, each (value, j, token) or None.
    ``margins`` (a list) collects the gaps between adjacent values wherever an order decides: a group's best 2 * beam_g + 1; for
    siblings a hypothesis's best k + 1 and the best 2 * beam + 1 of all."""
    G, one = int(groups), len(rows) == 1
    assert beam % G == 0 and (G == 1 or rate == 0)
    places = [None] * (2 * beam)
    fin = lambda x: bool(np.isfinite(x))

    def gaps(vals):
        if margins is not None and len(vals) > 1:
            v = np.asarray(vals, np.float64)
            margins.append(float(np.min(v[:-1] - v[1:])))

    if G == 1 and rate != 0 and not one:
        cands = []
        for j, row in enumerate(rows):
            own = []
            for lp, tok, c in row:
                with np.errstate(invalid="ignore", over="ignore"):
                    v = fl(fl(score[j]) + fl(lp))
                if fin(lp) and fin(v):
                    own.append((-float(v), tok, c, v))
            own.sort(key=lambda x: x[:3])
            gaps([x[3] for x in own[:2 * beam + 1]])
            for rank, (_, tok, c, v) in enumerate(own[:2 * beam], 1):
                with np.errstate(invalid="ignore", over="ignore"):
                    s = fl(v - fl(fl(rank) * fl(rate)))
                if fin(s):
                    cands.append((-float(s), j, tok, c, s))
        cands.sort(key=lambda x: x[:4])
        gaps([x[4] for x in cands[:2 * beam + 1]])
        for r, (_, j, tok, _, s) in enumerate(cands[:2 * beam]):
            places[r] = (s, j, tok)
        return places
    counts, bg = {}, beam // G
    for g in range(G):
        cands = []
        for j in ([0] if one else range(g, beam, G)):
            for lp, tok, c in rows[j]:
                n = counts.get(tok, 0)
                with np.errstate(invalid="ignore", over="ignore"):
                    x = fl(fl(lp) + fl(fl(-strength) * fl(n))) if n else fl(lp)
                    v = fl(fl(score[j]) + x)
                if fin(lp) and fin(v):
                    cands.append((-float(v), j, tok, c, v))
        cands.sort(key=lambda x: x[:4])
        gaps([x[4] for x in cands[:2 * bg + 1]])
        for c, (_, j, tok, _, v) in enumerate(cands[:2 * bg]):
            places[c * G + g] = (v, j, tok)
            counts[tok] = counts.get(tok, 0) + 1
    return places


def select_diverse_ref(cand_val, cand_id, st, beam, beam_in, groups=1, strength=0.0, rate=0.0, eos=EOS, pad=PAD, src=None):
    """gnnlm_beam_select_diverse on arrays -> (state after the step, table after the step or None); the inputs are left as they are."""
    st = {k: np.array(v) for k, v in st.items()}
    src = None if src is None else np.array(src)
    old = None if src is None else src.copy()
    B, T1, N = len(st["t"]), st["hist_tok"].shape[1], cand_val.shape[1]
    for b in range(B):
        t, s0 = int(st["t"][b]), b * beam
        if st["finished"][b] or not 0 <= t <= T1 - 1:
            continue
        rows = [[(np.float32(cand_val[b * beam_in + j, c]), int(cand_id[b * beam_in + j, c]), c) for c in range(N)] for j in range(beam_in)]
        places = step_list(st["score"][b], rows, beam, groups, strength, rate)
        history = lambda j: ([], []) if t == 0 else walk(st, b, t - 1, j)
        for p in places[:beam]:
            if p is not None and p[2] == eos and st["fin_n"][b] < beam:
                s, j, _ = p
                f = int(st["fin_n"][b])
                toks, cum = history(j)
                st["fin_tok"][b, f, :t + 1] = toks + [eos]
                st["fin_cum"][b, f, :t + 1] = cum + [s]
                st["fin_len"][b, f], st["fin_score"][b, f] = t + 1, s
                st["fin_n"][b] += 1
        alive = [p for p in places if p is not None and p[2] != eos][:beam]
        par = []
        for j in range(beam):
            s, jp, tok = alive[j] if j < len(alive) else (np.float32(-np.inf), j, pad)
            par.append(jp)
            st["next"][s0 + j], st["parent"][s0 + j], st["score"][b, j] = tok, s0 + jp, s
            st["hist_tok"][b, t, j], st["hist_par"][b, t, j], st["hist_score"][b, t, j] = tok, jp, s
        if src is not None:
            n, cap = int(st["len"][s0]), src.shape[1]
            rows_n = min(max(n, 0), cap)
            for j in range(beam):
                src[s0 + j, :rows_n] = s0 if beam_in == 1 else old[s0 + par[j], :rows_n]
                if 0 <= n < cap:
                    src[s0 + j, n] = s0 + j
        if st["fin_n"][b] == beam or t == T1 - 1:
            st["finished"][b] = 1
            st["done"][s0:s0 + beam] = 1
        st["t"][b] = t + 1
    return st, src


def diverse_beam_search_ref(lprobs_fn, prompts, beam, max_new, groups=1, strength=0.0, rate=0.0, min_len=1, lenpen=1.0, unnormalized=False,
                            unk_penalty=0.0, score0=None, len0=None, nbest=None, pad=PAD, eos=EOS, unk=UNK):
    """prompts as fed (lists of token ids); ``lprobs_fn(history)`` -> the next token's log-probs [V] before the pad / unk rules.
    -> (per prompt the hypotheses best first: dicts tokens / score / raw / positional_scores, info) with info['step_margin'] the
    smallest gap step_list reports at any step, info['final_margin'] the smallest gap between two final scores of a sentence,
    info['shift'] how often a survivor left its group's place (an eos in front of it was finalized or an earlier place was empty)."""
    out, info, margins = [], dict(final_margin=np.inf, shift=0), []
    for b, prompt in enumerate(prompts):
        s0 = 0.0 if score0 is None else float(score0[b])
        l0 = 0 if len0 is None else int(len0[b])
        hyps, finalized = [(list(prompt), s0, [], [])], []
        for t in range(max_new + 1):
            rows, score = [], []
            for h in hyps:
                if h is None:
                    rows.append([])
                    score.append(-np.inf)
                    continue
                lp = np.array(lprobs_fn(h[0]), np.float64)
                lp[np.isnan(lp)] = -np.inf
                lp[pad] = -np.inf
                lp[unk] -= unk_penalty
                if t == max_new:
                    keep = lp[eos]
                    lp[:] = -np.inf
                    lp[eos] = keep
                elif l0 + t < min_len:
                    lp[eos] = -np.inf
                rows.append([(float(lp[tok]), int(tok), int(tok)) for tok in np.nonzero(np.isfinite(lp))[0]])
                score.append(h[1])
            places = step_list(score, rows, beam, groups, strength, rate, fl=float, margins=margins)
            for p in places[:beam]:
                if p is not None and p[2] == eos and len(finalized) < beam:
                    finalized.append((hyps[p[1]][2] + [eos], hyps[p[1]][3] + [p[0]], t + 1))
            if len(finalized) == beam or t == max_new:
                break
            alive = [(r, p) for r, p in enumerate(places) if p is not None and p[2] != eos][:beam]
            info["shift"] += sum(r % groups != j % groups for j, (r, _) in enumerate(alive)) if groups > 1 else 0
            hyps = [(hyps[j][0] + [tok], v, hyps[j][2] + [tok], hyps[j][3] + [v]) for _, (v, j, tok) in alive] + [None] * (beam - len(alive))
        res = []
        for toks, cum, n in finalized:
            cum = np.asarray(cum, np.float64)
            raw = cum[-1]
            res.append({"tokens": np.asarray(toks, np.int64), "raw": float(raw), "score": float(raw if unnormalized else raw / (l0 + n) ** lenpen),
                        "positional_scores": cum - np.concatenate([[s0], cum[:-1]])})
        res = sorted(res, key=lambda h: h["score"], reverse=True)
        sc = np.asarray([h["score"] for h in res])
        if len(sc) > 1:
            info["final_margin"] = min(info["final_margin"], float(np.min(sc[:-1] - sc[1:])))
        out.append(res[:nbest] if nbest else res)
    info["step_margin"] = min(margins) if margins else np.inf
    return out, info
