"""Restatements for beam search (tests only; imports neither the package under test nor the reference), numpy float64:

  select_ref       the rules of gnnlm_beam_select (include/gnnlm.h) on given arrays, the one float32 add included
  beam_search_ref  the whole loop of gnnlm_amd/beam_search.py around a callable that maps a token history to a log-prob row
  ToyLM            the table model of tests/golden/beam_search.npz: logits = A[last] + B[last but one] + len * w, log_softmax in float32
  IncLprobs        decode_ref.Incremental (float64) behind that callable, one model step per new hypothesis
"""
import copy

import numpy as np

PAD, EOS, UNK = 1, 2, 3
STATE_KEYS = ("score", "t", "finished", "fin_n", "len", "done", "next", "parent", "hist_tok", "hist_par", "hist_score", "fin_tok", "fin_cum",
              "fin_len", "fin_score")


def new_state(B, beam, max_new, lens, score0=None, pad=PAD):
    """The arrays of gnnlm_beam_select's state, empty: dtypes as the descriptor's."""
    T1 = max_new + 1
    st = dict(score=np.zeros((B, beam), np.float32), t=np.zeros(B, np.int32), finished=np.zeros(B, np.int32), fin_n=np.zeros(B, np.int32),
              len=np.repeat(np.asarray(lens, np.int32), beam), done=np.zeros(B * beam, np.int32), next=np.full(B * beam, pad, np.int64),
              parent=np.zeros(B * beam, np.int32), hist_tok=np.full((B, T1, beam), pad, np.int64), hist_par=np.zeros((B, T1, beam), np.int32),
              hist_score=np.zeros((B, T1, beam), np.float32), fin_tok=np.full((B, beam, T1), pad, np.int64),
              fin_cum=np.zeros((B, beam, T1), np.float32), fin_len=np.zeros((B, beam), np.int32), fin_score=np.zeros((B, beam), np.float32))
    if score0 is not None:
        st["score"][:, 0] = score0
    return st


def select_ref(cand_val, cand_id, st, beam, beam_in, eos=EOS, pad=PAD, src=None):
    """-> (state after the step, table after the step or None); the inputs are left as they are."""
    st = {k: np.array(v) for k, v in st.items()}
    src = None if src is None else np.array(src)
    old = None if src is None else src.copy()
    B, T1, N = len(st["t"]), st["hist_tok"].shape[1], cand_val.shape[1]
    for b in range(B):
        t, s0 = int(st["t"][b]), b * beam
        if st["finished"][b] or not 0 <= t <= T1 - 1:
            continue
        cands = []
        for j in range(beam_in):
            for c in range(N):
                v = np.float32(cand_val[b * beam_in + j, c])
                with np.errstate(invalid="ignore", over="ignore"):
                    s = np.float32(np.float32(st["score"][b, j]) + v)
                if np.isfinite(v) and np.isfinite(s):
                    cands.append((-float(s), j, int(cand_id[b * beam_in + j, c]), c, s))
        cands.sort(key=lambda x: x[:4])
        top = cands[:2 * beam]
        history = lambda j: ([], []) if t == 0 else walk(st, b, t - 1, j)
        for _, j, tok, _, s in top[:beam]:
            if tok == eos and st["fin_n"][b] < beam:
                f = int(st["fin_n"][b])
                toks, cum = history(j)
                st["fin_tok"][b, f, :t + 1] = toks + [eos]
                st["fin_cum"][b, f, :t + 1] = cum + [s]
                st["fin_len"][b, f], st["fin_score"][b, f] = t + 1, s
                st["fin_n"][b] += 1
        alive = [c for c in top if c[2] != eos][:beam]
        par = []
        for j in range(beam):
            if j < len(alive):
                _, jp, tok, _, s = alive[j]
            else:
                jp, tok, s = j, pad, np.float32(-np.inf)
            par.append(jp)
            st["next"][s0 + j], st["parent"][s0 + j], st["score"][b, j] = tok, s0 + jp, s
            st["hist_tok"][b, t, j], st["hist_par"][b, t, j], st["hist_score"][b, t, j] = tok, jp, s
        if src is not None:
            n, cap = int(st["len"][s0]), src.shape[1]
            rows = min(max(n, 0), cap)
            for j in range(beam):
                src[s0 + j, :rows] = s0 if beam_in == 1 else old[s0 + par[j], :rows]
                if 0 <= n < cap:
                    src[s0 + j, n] = s0 + j
        if st["fin_n"][b] == beam or t == T1 - 1:
            st["finished"][b] = 1
            st["done"][s0:s0 + beam] = 1
        st["t"][b] = t + 1
    return st, src


def walk(st, b, t, j):
    """The tokens and cumulative scores of steps 0 .. t of the hypothesis that is number j after step t, along the backpointers."""
    toks, cum = [], []
    for s in range(t, -1, -1):
        toks.append(int(st["hist_tok"][b, s, j]))
        cum.append(st["hist_score"][b, s, j])
        j = int(st["hist_par"][b, s, j])
    return toks[::-1], cum[::-1]


def beam_search_ref(lprobs_fn, prompts, beam, max_new, min_len=1, lenpen=1.0, unnormalized=False, unk_penalty=0.0, score0=None, len0=None,
                    nbest=None, pad=PAD, eos=EOS, unk=UNK):
    """prompts as fed (lists of token ids); ``lprobs_fn(history)`` -> the next token's log-probs [V] before the pad / unk rules.
    -> (per prompt the hypotheses best first: dicts tokens / score / raw / positional_scores, info) with info['step_margin'] the
    smallest gap between adjacent values among the best 2 * beam + 1 candidates of any step, info['final_margin'] the smallest gap
    between two final scores of a sentence, info['surplus'] whether a step ever had fewer than ``beam`` survivors."""
    out, info = [], dict(step_margin=np.inf, final_margin=np.inf, surplus=False)
    for b, prompt in enumerate(prompts):
        s0 = 0.0 if score0 is None else float(score0[b])
        l0 = 0 if len0 is None else int(len0[b])
        hyps, finalized = [(list(prompt), s0, [], [])], []
        for t in range(max_new + 1):
            cands = []
            for j, h in enumerate(hyps):
                if h is None:
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
                cands += [(-(h[1] + lp[tok]), j, int(tok)) for tok in np.nonzero(np.isfinite(lp))[0]]
            cands.sort()
            vals = np.asarray([-c[0] for c in cands[:2 * beam + 1]])
            if len(vals) > 1:
                info["step_margin"] = min(info["step_margin"], float(np.min(vals[:-1] - vals[1:])))
            top = cands[:2 * beam]
            for nv, j, tok in top[:beam]:
                if tok == eos and len(finalized) < beam:
                    finalized.append((hyps[j][2] + [eos], hyps[j][3] + [-nv], t + 1))
            if len(finalized) == beam or t == max_new:
                break
            alive = [c for c in top if c[2] != eos][:beam]
            info["surplus"] |= len(alive) < beam
            hyps = [(hyps[j][0] + [tok], -nv, hyps[j][2] + [tok], hyps[j][3] + [-nv]) for nv, j, tok in alive] + [None] * (beam - len(alive))
        res = []
        for toks, cum, n in finalized:
            cum = np.asarray(cum)
            raw = cum[-1]
            res.append({"tokens": np.asarray(toks, np.int64), "raw": float(raw), "score": float(raw if unnormalized else raw / (l0 + n) ** lenpen),
                        "positional_scores": cum - np.concatenate([[s0], cum[:-1]])})
        res = sorted(res, key=lambda h: h["score"], reverse=True)
        sc = np.asarray([h["score"] for h in res])
        if len(sc) > 1:
            info["final_margin"] = min(info["final_margin"], float(np.min(sc[:-1] - sc[1:])))
        out.append(res[:nbest] if nbest else res)
    return out, info


class ToyLM:
    """The fixture's model: the next token's logits are A[last] + B[last but one] (the last token again while there is only one)
    + len(history) * w, then log_softmax -- in float32, as the fixture's generator computes it with torch."""

    def __init__(self, A, B, w):
        self.A, self.B, self.w = np.asarray(A, np.float32), np.asarray(B, np.float32), np.asarray(w, np.float32)

    def __call__(self, hist):
        a, b = hist[-1], hist[-2] if len(hist) > 1 else hist[-1]
        z = (self.A[a] + self.B[b] + np.float32(len(hist)) * self.w).astype(np.float64)
        z = z - z.max()
        return z - np.log(np.exp(z).sum())


class IncLprobs:
    """``decode_ref.Incremental`` (float64) as ``lprobs_fn``: the model state of every history seen is kept, so a new hypothesis costs
    one model step.  ``temperature`` divides the decoder output (the rows under the adaptive softmax, the logits under the plain layer)."""

    def __init__(self, m, hw=None, temperature=1.0):
        import decode_ref as dr
        self.dr, self.m, self.hw, self.T, self.memo = dr, m, hw, float(temperature), {}

    def _state(self, hist):
        key = tuple(hist)
        if key not in self.memo:
            if len(hist) == 1:
                inc = self.dr.Incremental(self.m)
            else:
                prev = self._state(hist[:-1])[0]
                inc = copy.copy(prev)
                inc.K, inc.V = [list(k) for k in prev.K], [list(v) for v in prev.V]
            self.memo[key] = (inc, inc.step(hist[-1]))
        return self.memo[key]

    def __call__(self, hist):
        row = self._state(list(hist))[1]["out"]
        if self.hw is None:
            z = np.asarray(row, np.float64) @ np.asarray(self.m["E"], np.float64).T / self.T
            z = z - z.max()
            return z - np.log(np.exp(z).sum())
        return self.dr.adaptive_dense_logp(row / self.T, **self.hw)


# ---------------------------------------------------------------------------------------------------- the end-to-end cases
# (head, beam) -> the seed of decode_ref.gen_model / gen_prompts (its prompts of 5 and 33 tokens); seeds for which the float64 run keeps
# every adjacent pair among a step's best 2 * beam + 1 candidates and every pair of a sentence's final scores E2E_MARGIN apart
# (tests/test_beam_ref_cpu.py checks it), so a flipped candidate on the device can only be a defect
E2E = dict(max_new=12, min_len=3, lenpen=0.7, unk_penalty=0.5)
E2E_MARGIN = 1e-3
E2E_SEEDS = {("dense", 1): 301, ("dense", 2): 301, ("dense", 5): 305, ("adaptive", 1): 301, ("adaptive", 2): 301, ("adaptive", 5): 332}
_E2E = {}


def e2e_case(head, beam):
    """-> (model, head weights, prompts, hypotheses, info) of the float64 run (computed once, shared)."""
    if (head, beam) not in _E2E:
        import decode_ref as dr
        seed = E2E_SEEDS[head, beam]
        m, hw = dr.gen_model(seed, head)
        prompts = dr.gen_prompts(seed)[1:]
        res, info = beam_search_ref(IncLprobs(m, hw), prompts, beam, **E2E)
        _E2E[head, beam] = (m, hw, prompts, res, info)
    return _E2E[head, beam]
