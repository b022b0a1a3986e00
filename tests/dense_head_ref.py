"""Float64 restatement of the plain (non-adaptive) output layer, shared by test_dense_head_cpu.py and test_dense_head_gpu.py:
``F.linear(features, weight) [+ xl_bias]`` (fairseq/models/transformer.py:843-852), ``log_softmax`` (:1081-1085), the target
column (fairseq/sequence_scorer.py:48-53,89), and the probability-space mixture of the two softmaxes (:990-991,1002).  numpy only."""
import math

import numpy as np

CASES = [("shared", False), ("shared", True), ("unshared", False), ("unshared", True)]


def dense_logp64(x, w, bias, target):
    """x [n, d], w [V, d], bias [V] or None, target [n] -> float64 [n]; -inf where the target is outside [0, V)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    logits = x @ w.T
    if bias is not None:
        logits = logits + np.asarray(bias, dtype=np.float64)[None, :]
    m = logits.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(logits - m).sum(axis=1, keepdims=True)))[:, 0]
    t = np.asarray(target, dtype=np.int64)
    ok = (t >= 0) & (t < w.shape[0])
    out = np.full(t.shape, -np.inf)
    out[ok] = logits[np.nonzero(ok)[0], t[ok]] - lse[ok]
    return out


def mix64(base, gnn, alpha):
    """log(alpha * exp(base) + (1 - alpha) * exp(gnn)); alpha = 0 is the GNN branch, alpha = 1 the base LM."""
    if alpha <= 0:
        return gnn
    if alpha >= 1:
        return base
    return np.logaddexp(math.log(alpha) + base, math.log(1 - alpha) + gnn)


def case_name(kind, with_bias):
    return f"{kind}.{'bias' if with_bias else 'nobias'}"


def case_weights(g, kind, with_bias):
    """(weight, bias) of a case of dense_head.npz."""
    return g["embed_tokens" if kind == "shared" else "embed_out"], (g["xl_bias"] if with_bias else None)


def half_round(a):
    """float32 array rounded to IEEE half (nearest even, overflow to inf) and widened again: what gemm_precision 3 makes of an operand."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)
