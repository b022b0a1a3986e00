"""Restatements for incremental decoding (tests only; imports neither the package under test nor the reference):

  Incremental      the model of tests/transformer_lm_ref.py taking ONE token at a time, with per-layer K / V lists (float64 by default)
  decode_attn_ref  one new row per sequence against a K/V cache, float64
  sample_ref       the pick of gnnlm_sample_topk from a sorted top-N, float64 prefix sums
  greedy_chain     the greedy continuation of a prompt under the tied plain output layer (logits = x . E^T), with every step's top-1 /
                   top-2 gap
"""
import math

import numpy as np
import torch

import transformer_lm_ref as tr

PAD, EOS, UNK = 1, 2, 3


class Incremental:
    """One sequence.  ``step(token)`` -> dict(out, last_inner, last_ffn_input) of the new row, numpy float64 [d]."""

    def __init__(self, m, dtype=torch.float64, half_gemm=False):
        self.m, self.dtype, self.half = m, dtype, half_gemm
        self.W = [{k: tr._t(v, dtype) for k, v in w.items()} for w in m["layers"]]
        self.K = [[] for _ in m["layers"]]
        self.V = [[] for _ in m["layers"]]
        self.n = 0

    def step(self, token):
        m, dtype, half = self.m, self.dtype, self.half
        x = torch.as_tensor(np.asarray(m["E"]))[int(token)].to(dtype) * torch.tensor(m["scale"], dtype=dtype)
        if m["P"] is not None:
            x = x + torch.as_tensor(np.asarray(m["P"]))[m["pad_idx"] + 1 + self.n].to(dtype)
        x = x.unsqueeze(0)
        if m["ln_emb"] is not None:
            x = tr._ln(x, tr._t(m["ln_emb"][0], dtype), tr._t(m["ln_emb"][1], dtype))
        H, d = m["H"], x.shape[1]
        dk = d // H
        ffn_in = None
        for l, W in enumerate(self.W):
            h = tr._ln(x, W["ln1_g"], W["ln1_b"])
            if half:
                q = tr._mm(h, W["wq"] * dk ** -0.5, True) + W["bq"] * dk ** -0.5
            else:
                q = (tr._mm(h, W["wq"], False) + W["bq"]) * dk ** -0.5
            self.K[l].append(tr._mm(h, W["wk"], half) + W["bk"])
            self.V[l].append(tr._mm(h, W["wv"], half) + W["bv"])
            K, V = torch.cat(self.K[l], 0), torch.cat(self.V[l], 0)
            a = torch.zeros_like(x)
            for hh in range(H):
                c = slice(hh * dk, (hh + 1) * dk)
                a[:, c] = torch.softmax(q[:, c] @ K[:, c].t(), dim=-1) @ V[:, c]
            x = x + tr._mm(a, W["wo"], half) + W["bo"]
            h = tr._ln(x, W["ln2_g"], W["ln2_b"])
            ffn_in = h
            f = tr._mm(h, W["w1"], half) + W["b1"]
            f = torch.relu(f) if m["act"] == "relu" else 0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0)))
            x = x + tr._mm(f, W["w2"], half) + W["b2"]
        inner = x
        if m["ln_out"] is not None:
            x = tr._ln(x, tr._t(m["ln_out"][0], dtype), tr._t(m["ln_out"][1], dtype))
        self.n += 1
        f64 = lambda t: t.to(torch.float64).numpy()[0]
        return {"out": f64(x), "last_inner": f64(inner), "last_ffn_input": f64(ffn_in)}


def incremental_rows(m, tokens, half_gemm=False):
    """Every row of one sequence fed token by token -> dict of [n, d] float64 arrays."""
    inc = Incremental(m, half_gemm=half_gemm)
    rows = [inc.step(t) for t in tokens]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def decode_attn_ref(q, k_new, v_new, K, V, lens, H, done=None):
    """q / k_new / v_new [B, d]; K / V [B, cap, d] (the rows below lens[b] are read, nothing else); lens [B] -> out [B, d] float64.
    A done row and a row with lens[b] outside [0, cap) are zero.  -> (out, rows appended [list of b], n_bad)."""
    B, d = q.shape
    cap, dk = K.shape[1], d // H
    out, appended, n_bad = np.zeros((B, d)), [], 0
    for b in range(B):
        if done is not None and done[b]:
            continue
        n = int(lens[b])
        if n < 0 or n >= cap:
            n_bad += 1
            continue
        appended.append(b)
        k = np.concatenate([np.asarray(K[b, :n], np.float64), np.asarray(k_new[b:b + 1], np.float64)], 0)
        v = np.concatenate([np.asarray(V[b, :n], np.float64), np.asarray(v_new[b:b + 1], np.float64)], 0)
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            s = k[:, c] @ np.asarray(q[b, c], np.float64)
            p = np.exp(s - s.max())
            out[b, c] = (p / p.sum()) @ v[:, c]
    return out, appended, n_bad


def sample_cdf(logp_row):
    """float64 inclusive prefix sums of exp(logp_j - logp_0); a -inf entry contributes 0."""
    lp = np.asarray(logp_row, np.float64)
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(lp), np.exp(lp - lp[0]), 0.0)
    return np.cumsum(e)


def sample_ref(logp, ids, u, pad=PAD, eos=EOS, done=None):
    """-> (next [B] int64, picked column [B] (-1: none), done [B], n_bad).  u None: greedy."""
    B, N = logp.shape
    nxt, col = np.full(B, pad, np.int64), np.full(B, -1, np.int64)
    done = np.zeros(B, np.int32) if done is None else np.array(done, np.int32)
    n_bad = 0
    for b in range(B):
        if done[b]:
            continue
        if not np.isfinite(logp[b, 0]):
            done[b], n_bad = 1, n_bad + 1
            continue
        j = 0
        if u is not None:
            c = sample_cdf(logp[b])
            j = int(np.argmax(c > np.float64(u[b]) * c[-1]))
        col[b], nxt[b] = j, ids[b, j]
        if nxt[b] == eos:
            done[b] = 1
    return nxt, col, done, n_bad


# ---------------------------------------------------------------------------------------------------- the generation cases
GEN_SEEDS = [301, 302]
GEN_PROMPT_LENS = [1, 5, 33]
GEN_NEW = 40
GEN_MODEL = dict(V=50, d=64, H=4, L=2, ffn=96, final_norm=False)
GEN_CUT = [16, 32]               # the adaptive variant: bands [0, 16) [16, 32) [32, V), widths d, d / 2, d / 4
GEN_HEADS = ["dense", "adaptive"]
_CACHE = {}


def gen_model(seed, head="dense"):
    """-> (model, head weights): "dense" the plain output layer tied to E; "adaptive" an adaptive input (E = emb_i @ proj_i^T per band)
    with its tied adaptive softmax (dict cutoff, emb, proj, class_proj as transformer_lm_ref.adaptive_logp takes them)."""
    if ("model", seed, head) not in _CACHE:
        m, hw = tr.make_model(seed, **GEN_MODEL), None
        if head == "adaptive":
            rs = np.random.RandomState(seed + 5)
            V, d = GEN_MODEL["V"], GEN_MODEL["d"]
            bands, lo = [], 0
            for i, hi in enumerate(GEN_CUT + [V]):
                dim = d // 2 ** i
                bands.append(((rs.randn(hi - lo, dim) * dim ** -0.5).astype(np.float32), (rs.randn(d, dim) * d ** -0.5).astype(np.float32)))
                lo = hi
            class_proj = (rs.randn(len(GEN_CUT), d) * d ** -0.5).astype(np.float32)
            m["E"] = tr.adaptive_table(bands)
            hw = dict(cutoff=GEN_CUT + [V], emb=[b[0] for b in bands], proj=[b[1] for b in bands], class_proj=class_proj)
        _CACHE["model", seed, head] = (m, hw)
    return _CACHE["model", seed, head]


def gen_prompts(seed):
    """Seeded prompts of GEN_PROMPT_LENS tokens, none of them a special symbol (ids 0 .. 3)."""
    rs = np.random.RandomState(seed + 17)
    return [[int(t) for t in rs.randint(4, GEN_MODEL["V"], size=n)] for n in GEN_PROMPT_LENS]


def dense_logp(m, x):
    """The tied plain output layer: log_softmax(x . E^T), float64 [.., V]."""
    z = np.asarray(x, np.float64) @ np.asarray(m["E"], np.float64).T
    z = z - z.max(-1, keepdims=True)
    return z - np.log(np.exp(z).sum(-1, keepdims=True))


def adaptive_dense_logp(x, cutoff, emb, proj, class_proj):
    """The tied adaptive softmax over the whole vocabulary, float64: x [d] -> [V] (transformer_lm_ref.adaptive_logp for every target)."""
    x = np.asarray(x, np.float64)
    lsm = lambda z: z - z.max() - np.log(np.exp(z - z.max()).sum())
    head = lsm(np.concatenate([np.asarray(emb[0], np.float64), np.asarray(class_proj, np.float64)], 0) @ x)
    out = np.empty(cutoff[-1])
    out[:cutoff[0]] = head[:cutoff[0]]
    for b in range(1, len(cutoff)):
        tail = lsm(np.asarray(emb[b], np.float64) @ (np.asarray(proj[b], np.float64).T @ x))
        out[cutoff[b - 1]:cutoff[b]] = head[cutoff[0] + b - 1] + tail
    return out


def greedy_chain(m, prompt, n_new, pad=PAD, eos=EOS, hw=None):
    """-> (tokens [<= n_new] (ends with eos if it came), their log-probs, the top-1 / top-2 gap of every step, the dense log-probs of
    every step [steps, V] after the pad rule)."""
    inc = Incremental(m)
    for t in prompt:
        row = inc.step(t)
    toks, lps, gaps, dist = [], [], [], []
    for _ in range(n_new):
        lp = dense_logp(m, row["out"]) if hw is None else adaptive_dense_logp(row["out"], **hw)
        lp[pad] = -np.inf
        order = np.argsort(-lp, kind="stable")
        toks.append(int(order[0]))
        lps.append(float(lp[order[0]]))
        gaps.append(float(lp[order[0]] - lp[order[1]]))
        dist.append(lp)
        if toks[-1] == eos:
            break
        row = inc.step(toks[-1])
    return toks, np.asarray(lps), np.asarray(gaps), np.stack(dist)


def gen_chain(seed, i, head="dense"):
    """The reference greedy chain of prompt i of seed under ``head`` (computed once, shared)."""
    if ("chain", seed, i, head) not in _CACHE:
        m, hw = gen_model(seed, head)
        _CACHE["chain", seed, i, head] = greedy_chain(m, gen_prompts(seed)[i], GEN_NEW, hw=hw)
    return _CACHE["chain", seed, i, head]
