"""Restatement of kNN-LM on the base transformer LM in float64, for the tests: the features of tests/transformer_lm_ref.py, an exact
search over the datastore, the softmax over the neighbours' similarities, and the log-space mix of fairseq/sequence_scorer.py:55-68,
121 (epsilon 1e-10).  Imports neither the package under test nor the reference.

The language model of tests/golden/base_knnlm.npz has a plain output layer tied to its token embedding: log p = log_softmax(x E^T).
"""
import numpy as np

import transformer_lm_ref as tr

EPS = 1e-10
SIZES = [5, 9, 3, 20, 3]                                         # sentence lengths of the fixture's stream; the 20 is longer than a block
CONFIGS = {                                                      # name: (break mode, tokens per sample, context window, max tokens)
    "none": ("none", 16, 0, 16),
    "none+ctx": ("none", 16, 8, 40),
    "complete": ("complete", 16, 0, 40),
}
MODEL = dict(seed=311, V=48, d=32, H=2, L=2, ffn=64, act="relu", final_norm=True, emb_norm=False, positions="sinusoidal")
N_KEYS = 40
MARGIN = 1e-3                                                    # the fixture's condition on the 8th and 9th similarity of a k = 8 query


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def features(m, tokens, samples, ctx):
    """-> dict(out, last_inner, last_ffn_input): float64 [n scored, d] of every scored token, samples in corpus order with ``ctx``
    context tokens in front of each."""
    tokens = np.asarray(tokens, np.int64)
    src = tr.shifted_source(tokens)
    parts = {"out": [], "last_inner": [], "last_ffn_input": []}
    for (s, e), c in zip(samples, ctx):
        f = tr.forward(m, src[s - c:e], [0, e - s + c])
        for k in parts:
            parts[k].append(f[k][c:])
    return {k: np.concatenate(v) for k, v in parts.items()}


def similarities(queries, keys, cosine):
    """float64 [n, N]: inner products; ``cosine``: of the unit queries with the unit keys (knn_model.py:181-184, index_builder.py:90-95)."""
    q, k = np.asarray(queries, np.float64), np.asarray(keys, np.float64)
    if cosine:
        q = q / np.sqrt((q ** 2).sum(-1, keepdims=True))
        k = k / np.sqrt((k ** 2).sum(-1, keepdims=True))
    return q @ k.T


def knn_term(sims, vals, targets, k, t):
    """-> (p_knn [n], recall [n] int64, ids [n, k], the neighbours' similarities [n, k]): the k largest similarities (ties by
    ascending id), softmax of sims / t over them, the mass on the neighbours whose label is the target (knn_model.py:196-217)."""
    ids = np.argsort(-sims, axis=1, kind="stable")[:, :k]
    s = np.take_along_axis(sims, ids, 1)
    p = np.exp(log_softmax(s / t))
    hit = np.asarray(vals, np.int64)[ids] == np.asarray(targets, np.int64)[:, None]
    return (p * hit).sum(-1), hit.sum(-1).astype(np.int64), ids, s


def mix(lm_logp, p_knn, lmbda):
    """sequence_scorer.py:55-68,121: logsumexp(log(1 - lmbda) + lm_logp, log(lmbda) + log(p_knn + 1e-10))."""
    return np.logaddexp(np.log(1.0 - lmbda) + np.asarray(lm_logp, np.float64), np.log(lmbda) + np.log(np.asarray(p_knn, np.float64) + EPS))


def dense_mix(lm_dense, sims, vals, k, t, lmbda):
    """The whole mixed distribution [n, V] (what --output-topk ranks): kNN mass scattered over the labels, then the same mix."""
    ids = np.argsort(-sims, axis=1, kind="stable")[:, :k]
    p = np.exp(log_softmax(np.take_along_axis(sims, ids, 1) / t))
    pk = np.zeros_like(lm_dense)
    np.add.at(pk, (np.arange(len(ids))[:, None], np.asarray(vals, np.int64)[ids]), p)
    return mix(lm_dense, pk, lmbda)


def margin(sims, k):
    """The gap between the k-th and the (k + 1)-th largest similarity of every query."""
    s = -np.sort(-sims, axis=1)
    return s[:, k - 1] - s[:, k]


def score(m, tokens, samples, ctx, keys, vals, keytype, cosine, k, t, lmbda):
    """-> dict(lm [n], mixed [n], recall [n], sims [n, N], ids [n, k], nsims [n, k], dense_lm [n, V]) in float64."""
    f = features(m, tokens, samples, ctx)
    tokens = np.asarray(tokens, np.int64)
    targets = np.concatenate([tokens[s:e] for s, e in samples])
    dense = log_softmax(f["out"] @ np.asarray(m["E"], np.float64).T)
    lm = dense[np.arange(len(targets)), targets]
    sims = similarities(f["last_ffn_input" if keytype == "last_ffn_input" else "last_inner"], keys, cosine)
    p_knn, recall, ids, nsims = knn_term(sims, vals, targets, k, t)
    return dict(lm=lm, mixed=mix(lm, p_knn, lmbda) if lmbda > 0 else lm, recall=recall, sims=sims, ids=ids, nsims=nsims, dense_lm=dense,
                targets=targets)
