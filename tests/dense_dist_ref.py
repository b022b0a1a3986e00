"""The dense next-token outputs (include/gnnlm.h: gnnlm_adaptive_log_probs, gnnlm_dense_log_probs, gnnlm_knn_mix_dense,
gnnlm_row_rank, and gnnlm_topk_merge with ncols = V) restated in float64 numpy.

    adaptive_log_probs   AdaptiveSoftmax.get_log_prob(input, None)        fairseq/modules/adaptive_softmax.py:170-206
    plain_log_probs      log_softmax(x . w^T + bias)                      fairseq/models/transformer.py:843-852,1081-1085
    knn_probs            softmax over the neighbours, summed per label    knn/knn_model.py:192-205 (`weighted_probs`)
    mix                  logaddexp(lm + log(1 - l), log(p_knn + 1e-10) + log l)   fairseq/sequence_scorer.py:55-68,121
    topn / rank          (value descending, id ascending): the order of gnnlm_topk_merge

The float32 inputs are widened exactly; every sum, exponential and logarithm is float64.  ``round_fp16`` rounds operands as
``gemm_precision 3`` does (tests/fp16_inputs.py draws inputs that need no rounding instead)."""
import numpy as np

F64 = np.float64
MASK_VALUE = -1e10          # knn_model.py:193
KNN_EPSILON = 1e-10         # sequence_scorer.py:110


def _lse(a, axis=-1):
    a = np.asarray(a, dtype=F64)
    m = a.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(a - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def log_softmax(a):
    """(a - max) - log sum exp(a - max): the maximum is taken off first, so a row of -1e12 (padding at t = 0.01) loses nothing."""
    a = np.asarray(a, dtype=F64)
    z = a - a.max(axis=-1, keepdims=True)
    return z - np.log(np.exp(z).sum(axis=-1, keepdims=True))


def round_fp16(a):
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(F64)


def adaptive_log_probs(x, w, rounder=None):
    """x [n, d]; w = dict(cutoff, emb, proj, class_proj) as oracle.adaptive_softmax takes it (proj[i] [d, dim_i], None for band 0)
    -> [n, V] float64.  ``rounder`` (e.g. round_fp16) is applied to every GEMM operand; the projection is a float32 tensor in
    memory before it is an operand again (include/gnnlm.h: gnnlm_adaptive_target_logp)."""
    r = rounder or (lambda a: np.asarray(a, dtype=F64))
    cut = [int(c) for c in w["cutoff"]]
    x = np.asarray(x)
    head_w = np.concatenate([np.asarray(w["emb"][0]), np.asarray(w["class_proj"])], 0)
    head = log_softmax(r(x) @ r(head_w).T)
    parts = [head[:, :cut[0]]]
    for i in range(1, len(cut)):
        xi = r(x) @ r(np.asarray(w["proj"][i]))
        if rounder is not None:
            xi = xi.astype(np.float32)
        tail = log_softmax(r(xi) @ r(np.asarray(w["emb"][i])).T)
        parts.append(tail + head[:, cut[0] + i - 1, None])
    return np.concatenate(parts, 1)


def plain_log_probs(x, weight, bias=None, rounder=None):
    r = rounder or (lambda a: np.asarray(a, dtype=F64))
    logits = r(x) @ r(weight).T
    if bias is not None:
        logits = logits + np.asarray(bias, dtype=F64)          # added unrounded under every precision
    return log_softmax(logits)


def neighbour_labels(ids, vals, n_store=None, row0=0):
    """[n, k] int64 labels as gnnlm_knn_interp reads them: an id < 0 wraps to id + n_store (numpy's vals[-1]); a row outside
    the shard [row0, row0 + len(vals)) has no label (-1)."""
    ids = np.asarray(ids, dtype=np.int64)
    vals = np.asarray(vals)
    n_store = len(vals) if n_store is None else n_store
    row = np.where(ids < 0, ids + n_store, ids) - row0
    ok = (row >= 0) & (row < len(vals))
    return np.where(ok, vals[np.clip(row, 0, len(vals) - 1)].astype(np.int64), -1)


def neighbour_probs(sims, ids, temperature):
    """softmax_j((ids == -1 ? -1e10 : sims) / t) with the division carried out in float32, as the kernels and the reference do."""
    s = np.where(np.asarray(ids) == -1, np.float32(MASK_VALUE), np.asarray(sims, dtype=np.float32)) / np.float32(temperature)
    assert s.dtype == np.float32
    return np.exp(log_softmax(s))


def knn_probs(sims, ids, labels, temperature, V):
    """-> p_knn [n, V] float64: the neighbours' probabilities summed per label; labels outside [0, V) contribute nothing."""
    p = neighbour_probs(sims, ids, temperature)
    labels = np.asarray(labels, dtype=np.int64)
    out = np.zeros((p.shape[0], V), dtype=F64)
    for r in range(p.shape[0]):
        ok = (labels[r] >= 0) & (labels[r] < V)
        np.add.at(out[r], labels[r][ok], p[r][ok])
    return out


def mix(lm_logp, p_knn, lmbda):
    """Everything in float64 (the reference adds the 1e-10 to a float32 tensor: a relative 6e-8 at most, far inside the bars)."""
    a = np.asarray(lm_logp, dtype=F64) + np.log(1.0 - lmbda)
    b = np.log(np.asarray(p_knn, dtype=F64) + KNN_EPSILON) + np.log(lmbda)
    return np.logaddexp(a, b)


def mix_f32(lm_logp, p_knn, lmbda):
    """The same formula evaluated in plain float32 numpy, step by step as gnnlm_knn_mix_dense states it."""
    f = np.float32
    a = np.asarray(lm_logp, dtype=f) + f(np.log(1.0 - lmbda))
    b = np.log(np.asarray(p_knn, dtype=f) + f(KNN_EPSILON)) + f(np.log(lmbda))
    m = np.maximum(a, b)
    out = m + np.log(np.exp(a - m) + np.exp(b - m))
    assert out.dtype == f
    return out


def present(v):
    v = np.asarray(v)
    return ~np.isnan(v) & (v != -np.inf)


def topn(values, n):
    """(ids [rows, n] int64, vals [rows, n]) of the n best columns by (value descending, id ascending); NaN and -inf are absent;
    missing entries are id -1 with -inf.  ``values`` is compared in the dtype it comes in (float32 for bit-for-bit checks)."""
    values = np.asarray(values)
    rows, V = values.shape
    ids = np.full((rows, n), -1, dtype=np.int64)
    vals = np.full((rows, n), -np.inf, dtype=values.dtype)
    for r in range(rows):
        ok = np.nonzero(present(values[r]))[0]
        v = values[r][ok] + values.dtype.type(0)                       # -0 -> +0
        order = np.lexsort((ok, -v))[:n]
        ids[r, :len(order)], vals[r, :len(order)] = ok[order], v[order]
    return ids, vals


def rank(values, target):
    """[rows] int32: present columns in front of the target; -1 for a target outside [0, V); a target whose own value is absent
    comes behind every present column."""
    values = np.asarray(values)
    rows, V = values.shape
    out = np.empty(rows, dtype=np.int32)
    cols = np.arange(V)
    for r in range(rows):
        t = int(target[r])
        if t < 0 or t >= V:
            out[r] = -1
            continue
        ok, tv = present(values[r]), values[r, t]
        if not present(tv):
            out[r] = ok.sum()
        else:
            with np.errstate(invalid="ignore"):
                out[r] = (ok & ((values[r] > tv) | ((values[r] == tv) & (cols < t)))).sum()
    return out


# ------------------------------------------------------------------------------------------------------ inputs of the tests
# (shared by tests/test_dense_dist_ref_cpu.py, which checks that plain float32 arithmetic stays within 1e-5 of the restatement on
# them, and tests/test_dense_dist_abi_gpu.py, which holds the kernels to 2e-5 on the same arrays)
HEAD_CUTOFF, HEAD_DIMS, HEAD_D = (100, 300, 603), (64, 16, 4), 64
PLAIN_V = 205
HEAD_ROWS = (1, 33, 130)
BIG = dict(cutoff=(20000, 60000, 267744), dims=(16, 8, 4), d=16, n=8192)          # 8192 x 267744 x 4 B = 8.8 GB of output
MIX_V, MIX_STORE, MIX_ROWS = 1500, 5000, 6
MIX_KS, MIX_TS, MIX_LMBDAS = (1, 8, 100, 1024), (1.0, 0.01), (0.1, 0.25)
MIX_PATTERNS = ("equal", "distinct", "padded", "outside")


def adaptive_weights(cutoff, dims, d, seed):
    """oracle-style weights (float32): emb[i] [size_i, dim_i] / sqrt(dim_i), proj[i] [d, dim_i] / sqrt(d), class_proj [n_tail, d]."""
    rs = np.random.RandomState(seed)
    emb, proj, prev = [], [], 0
    for i, (c, dim) in enumerate(zip(cutoff, dims)):
        emb.append((rs.randn(c - prev, dim) * dim ** -0.5).astype(np.float32))
        proj.append(None if i == 0 else (rs.randn(d, dim) * d ** -0.5).astype(np.float32))
        prev = c
    return {"cutoff": list(cutoff), "emb": emb, "proj": proj, "class_proj": (rs.randn(len(cutoff) - 1, d) * d ** -0.5).astype(np.float32)}


def head_inputs(n, seed=11):
    """-> (x [n, 64] f32, adaptive weights of HEAD_CUTOFF, plain weight [205, 64], bias [205])"""
    rs = np.random.RandomState(seed + n)
    x = (1.5 * rs.randn(n, HEAD_D)).astype(np.float32)
    return x, adaptive_weights(HEAD_CUTOFF, HEAD_DIMS, HEAD_D, seed), (rs.randn(PLAIN_V, HEAD_D) * HEAD_D ** -0.5).astype(np.float32), \
        rs.randn(PLAIN_V).astype(np.float32)


def mix_case(k, pattern, seed, n=MIX_ROWS, V=MIX_V, n_store=MIX_STORE):
    """-> dict(sims [n, k] f32 with |sims| <= 2, ids [n, k] i64, vals [n_store] i32, labels [n, k] (= vals[ids], numpy's wrap for
    -1), lm_logp [n, V] f32 (a normalised row), V, n_store).  Patterns: every label equal / all labels of a row distinct / ids padded
    with -1 (the last row entirely) / labels at V, V + 100 and -3 among the valid ones."""
    rs = np.random.RandomState(seed)
    sims = -np.sort(-rs.uniform(-2.0, 2.0, size=(n, k)).astype(np.float32), axis=1)       # best first, as a search returns them
    ids = rs.randint(0, n_store, size=(n, k)).astype(np.int64)
    vals = rs.randint(0, V, size=n_store).astype(np.int32)
    if pattern == "equal":
        vals[:] = 7
    elif pattern == "distinct":
        assert k <= V <= n_store
        vals[:V] = rs.permutation(V)
        ids = np.stack([rs.permutation(V)[:k] for _ in range(n)]).astype(np.int64)
    elif pattern == "padded":
        ids[:, k - k // 3:] = -1
        ids[n - 1, :] = -1                                              # a row without any neighbour: uniform over vals[-1]
        ids[0, 0] = -1
    elif pattern == "outside":
        which = rs.rand(n_store)
        vals[which < 0.1] = V
        vals[(which >= 0.1) & (which < 0.2)] = -3
        vals[(which >= 0.2) & (which < 0.25)] = V + 100
        ids[1, :] = np.nonzero(which < 0.25)[0][rs.randint(0, (which < 0.25).sum(), k)]    # a row whose every label is outside
    else:
        raise ValueError(pattern)
    lm = log_softmax(2.0 * rs.randn(n, V)).astype(np.float32)
    return dict(sims=sims, ids=ids, vals=vals, labels=neighbour_labels(ids, vals, n_store), lm_logp=lm, V=V, n_store=n_store, k=k)


def mix_expected(case, temperature, lmbda):
    """-> (p_knn [n, V], out [n, V]) float64"""
    p = knn_probs(case["sims"], case["ids"], case["labels"], temperature, case["V"])
    return p, mix(case["lm_logp"], p, lmbda)


def mix_float32(case, temperature, lmbda):
    """The same in plain float32 numpy: softmax, per-label sums in neighbour order, the mix formula."""
    f = np.float32
    s = np.where(case["ids"] == -1, f(MASK_VALUE), case["sims"]) / f(temperature)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True, dtype=f)
    assert p.dtype == f
    out = np.zeros((p.shape[0], case["V"]), dtype=f)
    for r in range(p.shape[0]):
        ok = (case["labels"][r] >= 0) & (case["labels"][r] < case["V"])
        np.add.at(out[r], case["labels"][r][ok], p[r][ok])
    return out, mix_f32(case["lm_logp"], out, lmbda)


def rank_case(seed=5, n=9, V=777):
    """Rows with ties: values from a 12-entry grid (equal values at many ids), one constant row, one row with NaN / +-inf / +-0
    entries; targets inside ties, at both ends, outside [0, V), and on an absent value."""
    rs = np.random.RandomState(seed)
    grid = np.array([-9.5, -7.25, -7.0, -5.5, -4.0, -3.75, -2.5, -2.0, -1.5, -0.75, -0.5, -0.25], dtype=np.float32)
    v = grid[rs.randint(0, len(grid), size=(n, V))]
    v[2] = np.float32(-3.0)
    sp = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 1e-45, -1e-45], dtype=np.float32)
    v[3, :70] = np.resize(sp, 70)
    t = rs.randint(0, V, size=n).astype(np.int64)
    t[0], t[1], t[2] = 0, V - 1, V // 2
    t[3] = 1                                                            # the target's own value is -inf: absent
    t[4], t[5] = -1, V
    t[6] = 2 ** 32 + 3
    v[7, 5] = v[7, 600] = np.float32(0.5)
    t[7] = 600                                                          # tied for the lead with a smaller id in front
    return v, t
