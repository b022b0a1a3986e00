"""Restatement of the base transformer LM (decoder-only, pre-norm, eval mode) for the tests: embed, positions, layers, key types,
the shifted source and the context-window slicing.  float64 by default; ``dtype=torch.float32`` gives the float32 evaluation of the
same formulas and ``half_gemm=True`` rounds both operands of every matrix product to float16 first (what ``--fp16`` means in this
project: tests/fp16_inputs.py).  Imports neither the package under test nor the reference.

A model is a plain dict (``make_model``):
  E [V, d]            the token-embedding table (already materialised: adaptive input = per band emb_i @ proj_i^T)
  P [rows, d] | None  position table; row pad_idx + 1 + t serves position t of a block
  scale, pad_idx, H, act ("relu" | "gelu"), ln_emb (g, b) | None, ln_out (g, b) | None
  layers: list of dicts ln1_g ln1_b wq bq wk bk wv bv wo bo ln2_g ln2_b w1 b1 w2 b2
"""
import math

import numpy as np
import torch

EOS, PAD = 2, 1


def sinusoidal_table(rows, d, pad_idx=PAD):
    """float32, the order of operations of the published tensor2tensor-style table: exp(arange(half) * -(log(1e4) / (half - 1))),
    outer product with the positions, [sin | cos], the pad row zeroed."""
    half = d // 2
    step = math.log(10000) / (half - 1)
    freq = torch.exp(torch.arange(half, dtype=torch.float32) * -step)
    ang = torch.arange(rows, dtype=torch.float32).unsqueeze(1) * freq.unsqueeze(0)
    tab = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    if d % 2:
        tab = torch.cat([tab, torch.zeros(rows, 1)], dim=1)
    if pad_idx < rows:
        tab[pad_idx] = 0
    return tab.numpy()


def adaptive_table(bands):
    """[(emb_i [size_i, dim_i], proj_i [d, dim_i])] -> E [V, d] in float64."""
    return np.concatenate([np.asarray(e, np.float64) @ np.asarray(p, np.float64).T for e, p in bands], 0)


def make_model(seed, V, d, H, L, ffn, act="relu", final_norm=True, emb_norm=False, positions="sinusoidal", pos_rows=128, scale=None):
    """Seeded float32 weights (numpy) of a small model; Linear weights ~ 1 / sqrt(fan in), LayerNorm gains around 1."""
    rs = np.random.RandomState(seed)
    r = lambda *s: rs.randn(*s).astype(np.float32)
    lin = lambda o, i: (r(o, i) / np.float32(math.sqrt(i)), 0.1 * r(o))
    ln = lambda: ((1.0 + 0.1 * r(d)).astype(np.float32), 0.1 * r(d))
    m = {"E": (r(V, d) / np.float32(math.sqrt(d))), "H": H, "act": act, "pad_idx": PAD, "scale": math.sqrt(d) if scale is None else scale,
         "P": None, "ln_emb": ln() if emb_norm else None, "layers": []}
    if positions == "sinusoidal":
        m["P"] = sinusoidal_table(pos_rows, d)
    elif positions == "learned":
        m["P"] = (0.5 * r(pos_rows, d)).astype(np.float32)
        m["P"][PAD] = 0
    for _ in range(L):
        w = {}
        w["ln1_g"], w["ln1_b"] = ln()
        for n in "qkvo":
            w["w" + n], w["b" + n] = lin(d, d)
        w["ln2_g"], w["ln2_b"] = ln()
        w["w1"], w["b1"] = lin(ffn, d)
        w["w2"], w["b2"] = lin(d, ffn)
        m["layers"].append(w)
    m["ln_out"] = ln() if final_norm else None
    return m


def _t(a, dtype):
    return None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)


def _mm(a, w, half):
    """a @ w^T; ``half``: both operands rounded to float16 first (products are then exact in the working precision)."""
    if half:
        a, w = a.to(torch.float16).to(a.dtype), w.to(torch.float16).to(w.dtype)
    return a @ w.t()


def _ln(x, g, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def embed(m, tokens, block_off, dtype=torch.float64):
    """x[r] = scale * E[tok[r]] + P[pad + 1 + position of r in its block] -- each step rounded to ``dtype``."""
    tokens = np.asarray(tokens, np.int64)
    off = np.asarray(block_off, np.int64) - int(block_off[0])
    x = torch.as_tensor(np.asarray(m["E"]))[torch.as_tensor(tokens)].to(dtype) * torch.tensor(m["scale"], dtype=dtype)
    if m["P"] is not None:
        pos = np.concatenate([m["pad_idx"] + 1 + np.arange(off[b + 1] - off[b]) for b in range(len(off) - 1)])
        x = x + torch.as_tensor(np.asarray(m["P"]))[torch.as_tensor(pos)].to(dtype)
    return x


def embed_f32(E, tokens, block_off, P, pad_idx, scale):
    """The embed kernel's contract in numpy float32, two roundings: fl32(fl32(scale * E[tok]) + P[...]); a token outside [0, V) gives
    a zero row.  -> (x, number of bad ids)."""
    E = np.asarray(E, np.float32)
    tokens = np.asarray(tokens, np.int64)
    off = np.asarray(block_off, np.int64) - int(block_off[0])
    ok = (tokens >= 0) & (tokens < E.shape[0])
    x = (np.float32(scale) * E[np.where(ok, tokens, 0)]).astype(np.float32)
    if P is not None:
        pos = np.concatenate([pad_idx + 1 + np.arange(off[b + 1] - off[b]) for b in range(len(off) - 1)])
        x = (x + np.asarray(P, np.float32)[pos]).astype(np.float32)
    x[~ok] = 0
    return x, int((~ok).sum())


def forward(m, tokens, block_off, dtype=torch.float64, half_gemm=False):
    """-> dict(out, last_inner, last_ffn_input) as numpy float64 arrays [n_tok, d].  Attention is causal inside each block of the
    packed rows, softmax over the keys at or before the query, q scaled by d_k^-0.5 after its bias."""
    off = np.asarray(block_off, np.int64) - int(block_off[0])
    x = embed(m, tokens, off, dtype)
    if m["ln_emb"] is not None:
        x = _ln(x, _t(m["ln_emb"][0], dtype), _t(m["ln_emb"][1], dtype))
    H, d = m["H"], x.shape[1]
    dk = d // H
    ffn_in = None
    for w in m["layers"]:
        W = {k: _t(v, dtype) for k, v in w.items()}
        h = _ln(x, W["ln1_g"], W["ln1_b"])
        if half_gemm:
            # the library folds d_k^-0.5 into the q weights before they are rounded; for d_k a power of 4 the two orders agree exactly
            q = _mm(h, W["wq"] * dk ** -0.5, True) + W["bq"] * dk ** -0.5
        else:
            q = (_mm(h, W["wq"], False) + W["bq"]) * dk ** -0.5
        k = _mm(h, W["wk"], half_gemm) + W["bk"]
        v = _mm(h, W["wv"], half_gemm) + W["bv"]
        a = torch.zeros_like(x)
        for b in range(len(off) - 1):
            s, e = int(off[b]), int(off[b + 1])
            n = e - s
            mask = torch.triu(torch.full((n, n), float("-inf"), dtype=dtype), 1)
            for hh in range(H):
                c = slice(hh * dk, (hh + 1) * dk)
                p = torch.softmax(q[s:e, c] @ k[s:e, c].t() + mask, dim=-1)
                a[s:e, c] = p @ v[s:e, c]
        x = x + _mm(a, W["wo"], half_gemm) + W["bo"]
        h = _ln(x, W["ln2_g"], W["ln2_b"])
        ffn_in = h
        f = _mm(h, W["w1"], half_gemm) + W["b1"]
        f = torch.relu(f) if m["act"] == "relu" else 0.5 * f * (1.0 + torch.erf(f / math.sqrt(2.0)))
        x = x + _mm(f, W["w2"], half_gemm) + W["b2"]
    inner = x
    if m["ln_out"] is not None:
        x = _ln(x, _t(m["ln_out"][0], dtype), _t(m["ln_out"][1], dtype))
    f64 = lambda t: t.to(torch.float64).numpy()
    return {"out": f64(x), "last_inner": f64(inner), "last_ffn_input": f64(ffn_in)}


# ---------------------------------------------------------------------------------------------------- the GPU test's cases
# packed blocks that cross the attention kernel's 32-row tiles; the CPU test evaluates the same cases in float32
GPU_BLOCKS = [1, 31, 32, 33, 70]
GPU_CASES = {
    1: dict(seed=301, V=50, d=64, H=4, L=2, ffn=96, act="relu", final_norm=False, emb_norm=False, positions="sinusoidal"),
    2: dict(seed=302, V=50, d=64, H=2, L=1, ffn=256, act="gelu", final_norm=True, emb_norm=True, positions="learned"),
    3: dict(seed=303, V=50, d=256, H=2, L=1, ffn=512, act="relu", final_norm=False, emb_norm=False, positions=None),
}
FEATURE_BAR = 5e-5              # max|dev - ref64| / max|ref64| (README "Parity")
_CACHE = {}


def gpu_case(i):
    """-> (model, tokens [n_tok], block_off [n_blocks + 1]) of case i (built once; read-only by convention)."""
    if i not in _CACHE:
        c = GPU_CASES[i]
        m = make_model(pos_rows=PAD + 1 + max(GPU_BLOCKS), **c)
        off = np.concatenate([[0], np.cumsum(GPU_BLOCKS)]).astype(np.int64)
        rs = np.random.RandomState(c["seed"] + 1)
        tokens = rs.randint(0, c["V"], size=int(off[-1])).astype(np.int64)
        tokens[:2] = [0, c["V"] - 1]
        _CACHE[i] = (m, tokens, off)
    return _CACHE[i]


def gpu_case_ref(i, half_gemm=False):
    """The float64 restatement of case i (computed once per variant and shared by the tests)."""
    key = (i, "ref", half_gemm)
    if key not in _CACHE:
        m, tokens, off = gpu_case(i)
        _CACHE[key] = forward(m, tokens, off, torch.float64, half_gemm)
    return _CACHE[key]


FP16_SHARE = 0.5                # precision 3: rms(dev - rounded ref64) <= this share of rms(ref64 - rounded ref64) (test_transformer_lm_ref_cpu.py)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def golden_model(g, name, H, act, scale):
    """The model dict of a case of tests/golden/transformer_lm.npz (the fixture stores its own weights)."""
    layers, i = [], 0
    while f"{name}.layer{i}.wq" in g:
        layers.append({k: g[f"{name}.layer{i}.{k}"] for k in ("ln1_g", "ln1_b", "wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln2_g", "ln2_b",
                                                               "w1", "b1", "w2", "b2")})
        i += 1
    pair = lambda k: (g[f"{name}.{k}.g"], g[f"{name}.{k}.b"]) if f"{name}.{k}.g" in g else None
    if f"{name}.E" in g:
        E = g[f"{name}.E"]
    else:
        bands, b = [], 0
        while f"{name}.band{b}.emb" in g:
            bands.append((g[f"{name}.band{b}.emb"], g[f"{name}.band{b}.proj"]))
            b += 1
        E = adaptive_table(bands)
    return {"E": E, "P": g[f"{name}.P"] if f"{name}.P" in g else None, "H": H, "act": act, "pad_idx": PAD, "scale": scale,
            "ln_emb": pair("ln_emb"), "ln_out": pair("ln_out"), "layers": layers}


# ---------------------------------------------------------------------------------------------------- data side
def shifted_source(tokens, eos=EOS):
    """The source of a target stream: the stream shifted right by one, eos in front of token 0."""
    tokens = np.asarray(tokens, np.int64)
    return np.concatenate([[eos], tokens[:-1]]).astype(np.int64)


def context_windows(lengths, tokens_per_sample, w):
    """Context tokens in front of every sample when samples are taken in corpus order: the carry is the last ``w`` tokens of the
    previous row (its own context included), cut from the front so that context + sample <= tokens_per_sample + w, where
    ``tokens_per_sample`` is the sample size AFTER w was taken off it."""
    out, carry = [], 0
    for n in lengths:
        extra = carry + int(n) - (tokens_per_sample + w)
        if extra > 0:
            carry = max(0, carry - extra)
        out.append(carry)
        carry = min(w, carry + int(n))
    return out


def adaptive_logp(x, target, cutoff, emb, proj, class_proj):
    """Tied adaptive softmax, target log-probability, float64.  cutoff: band upper bounds (last = V); emb[i] [size_i, dim_i],
    proj[i] [d, dim_i] (band 0's is not used by the head); class_proj [n_bands - 1, d]."""
    x = np.asarray(x, np.float64)
    head_w = np.concatenate([np.asarray(emb[0], np.float64), np.asarray(class_proj, np.float64)], 0)
    lse = lambda z: z.max(-1) + np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1))
    head = x @ head_w.T
    head_lse = lse(head)
    out = np.empty(len(target))
    lo = [0] + list(cutoff[:-1])
    for r, t in enumerate(np.asarray(target)):
        b = next(i for i, c in enumerate(cutoff) if t < c)
        if b == 0:
            out[r] = head[r, t] - head_lse[r]
        else:
            tail = (x[r] @ np.asarray(proj[b], np.float64)) @ np.asarray(emb[b], np.float64).T
            out[r] = head[r, cutoff[0] + b - 1] - head_lse[r] + tail[t - lo[b]] - lse(tail)
    return out


def score_split(m, head, tokens, samples, ctx, key="last_inner", dtype=torch.float64):
    """The whole base-LM evaluation of a token stream: ``samples`` [(start, end)] in corpus order, ``ctx`` context tokens in front of
    each.  -> (log p of every scored token [sum of sample lengths], the key of every scored token [.., d])."""
    tokens = np.asarray(tokens, np.int64)
    src = shifted_source(tokens)
    logp, keys = [], []
    for (s, e), c in zip(samples, ctx):
        f = forward(m, src[s - c:e], [0, e - s + c], dtype)
        logp.append(adaptive_logp(f["out"][c:], tokens[s:e], **head))
        keys.append(f[key][c:])
    return np.concatenate(logp), np.concatenate(keys)
