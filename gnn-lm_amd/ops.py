"""torch-tensor wrappers over the kernel-level C ABI (include/gnnlm.h).

torch is plumbing here (device memory + the current HIP stream); every function below launches a
hand-written gfx950 kernel through libgnnlm_hip.so and raises if that library is missing.
"""
import ctypes

import torch

from . import _lib
from ._lib import call, call_desc, ptr, stream


def _dev(*ts):
    """Refuse host tensors explicitly: the product path has no CPU fallback."""
    for t in ts:
        if t is not None and not (t.is_cuda and t.is_contiguous() or (t.is_cuda and t.dim() == 2 and t.stride(1) == 1)):
            raise _lib.GnnlmError("gnnlm_amd kernels need contiguous device (HIP) tensors; there is no CPU fallback")


def _f32(*ts):
    for t in ts:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f"expected float32, got {t.dtype}")
    return ts[0]


def _dtype(t, dt, what):
    """The C ABI reinterprets raw pointers: a wrong dtype must fail here, not be silently re-read."""
    if t is not None and t.dtype != dt:
        raise TypeError(f"{what}: expected {dt}, got {t.dtype}")


# "fp16" (`eval_lm --fp16`): both GEMM operands rounded to IEEE float16 (nearest even; beyond +-65504 -> +-inf as Tensor.half()),
# exact products, f32 accumulation, f32 epilogues and f32 tensors -- never narrower than the reference's model.half()
PRECISIONS = {"f32": 0, "bf16x3": 1, "bf16x6": 2, "fp16": 3}


def precision_value(p):
    """A name of PRECISIONS or its value -> the value of the C ABI's ``precision`` fields."""
    v = PRECISIONS.get(p, p)
    if v not in PRECISIONS.values() or isinstance(v, bool):
        raise ValueError(f"precision: one of {sorted(PRECISIONS)} (or its value), got {p!r}")
    return int(v)


def precision_name(*values):
    """The name of the precision the given ``gemm_precision`` values share ("mixed" if they differ)."""
    names = {v: k for k, v in PRECISIONS.items()}
    return names[values[0]] if len(set(values)) == 1 else "mixed"


def gemm_nt(A, W, bias=None, residual=None, alpha=1.0, out=None, bias_mode=1, gate=None,
            a_rows=None, m_dev=None, precision=0, c_rows=None):
    """C = alpha * A @ W.T (+ gate*bias) (+ residual).  A [M,K] (row stride may exceed K), W [N,K].
    a_rows: logical row r reads A[a_rows[r]] (< 0: zero row); c_rows: row r is stored to (and its residual
    read from) row c_rows[r] of ``out`` (which must then be given)."""
    _f32(A, W, bias, residual, gate, out)
    _dtype(a_rows, torch.int32, "a_rows"), _dtype(m_dev, torch.int32, "m_dev")
    _dev(A, W, bias, residual, gate, a_rows, m_dev, out, c_rows)
    M, K = A.shape
    N = W.shape[0]
    if a_rows is not None:
        M = a_rows.shape[0]
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    g = _lib.gnnlm_gemm_t()
    g.A, g.lda = A.data_ptr(), A.stride(0)
    g.W, g.ldw = W.data_ptr(), W.stride(0)
    g.C, g.ldc = out.data_ptr(), out.stride(0)
    if a_rows is not None:
        g.a_rows = a_rows.data_ptr()
        g.a_rows_bound = A.shape[0]                    # every gathered row lies inside A
    if c_rows is not None:
        assert c_rows.dtype == torch.int32 and c_rows.shape[0] == M
        g.c_rows = c_rows.data_ptr()
    if bias is not None:
        g.bias, g.bias_mode = bias.data_ptr(), bias_mode
    if gate is not None:
        g.gate = gate.data_ptr()
    if residual is not None:
        g.R, g.ldr = residual.data_ptr(), residual.stride(0)
    if m_dev is not None:
        g.m_dev = m_dev.data_ptr()
    g.alpha = alpha
    g.M, g.N, g.K = M, N, K
    g.precision = PRECISIONS.get(precision, precision)
    call_desc("gnnlm_gemm_nt", g)
    return out


def gemm_lse(A, W, pick=None, alpha=1.0, m_dev=None, precision=0):
    """lse[r] = logsumexp_n(alpha * A[r] . W[n]) and picked[r] = alpha * A[r] . W[pick[r]], without
    materialising the [M, N] logits (LSE epilogue of the GEMM + gnnlm_lse_reduce)."""
    _f32(A, W)
    _dtype(m_dev, torch.int32, "m_dev")
    _dev(A, W, pick, m_dev)
    M, K = A.shape
    N = W.shape[0]
    n_parts = 2 * ((N + 127) // 128)
    part = torch.empty(M, n_parts, 2, device=A.device, dtype=torch.float32)
    lse = torch.empty(M, device=A.device, dtype=torch.float32)
    picked = torch.zeros(M, device=A.device, dtype=torch.float32)
    g = _lib.gnnlm_gemm_t()
    g.A, g.lda, g.W, g.ldw = A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0)
    g.lse_part = part.data_ptr()
    if pick is not None:
        assert pick.dtype == torch.int32
        g.lse_pick, g.lse_picked = pick.data_ptr(), picked.data_ptr()
    if m_dev is not None:
        g.m_dev = m_dev.data_ptr()
    g.alpha = alpha
    g.M, g.N, g.K = M, N, K
    g.precision = PRECISIONS.get(precision, precision)
    call_desc("gnnlm_gemm_nt", g)
    call("gnnlm_lse_reduce", ptr(part), n_parts, M, ptr(m_dev), ptr(lse), stream())
    return lse, picked


def pq_gather_decode(codes, centroids, ids, left=0, right=0, n_store=None, row0=0, vals=None,
                     want_x=True, want_codes=False, want_labels=False, want_valid=True):
    """Gather + decode the slots of each centre row in ``ids`` (flattened).  Returns a dict."""
    _dev(codes, centroids, ids, vals)
    M, ksub, dsub = centroids.shape
    assert ksub == 256 and codes.dtype == torch.uint8 and ids.dtype == torch.int64
    n_g = 1 + left + right
    G = ids.numel()
    S = G * n_g
    dev = codes.device
    d = _lib.gnnlm_gather_t()
    d.codes = codes.data_ptr()
    d.n_local = codes.shape[0]
    d.n_store = n_store if n_store is not None else codes.shape[0]
    d.row0 = row0
    d.M, d.dsub = M, dsub
    d.centroids = centroids.data_ptr()
    d.ids, d.n_groups = ids.data_ptr(), G
    d.left, d.right = left, right
    d.vals_itemsize = 4
    out = {}
    if vals is not None:
        d.vals, d.vals_itemsize = vals.data_ptr(), vals.element_size()
    if want_x:
        out["x"] = torch.empty(S, M * dsub, device=dev, dtype=torch.float32)
        d.out_x, d.ld_x = out["x"].data_ptr(), M * dsub
    if want_codes:
        out["codes"] = torch.empty(S, M, device=dev, dtype=torch.uint8)
        d.out_codes = out["codes"].data_ptr()
    if want_labels:
        out["labels"] = torch.empty(S, device=dev, dtype=torch.int32)
        d.out_labels = out["labels"].data_ptr()
    if want_valid:
        out["valid"] = torch.empty(S, device=dev, dtype=torch.uint8)
        d.out_valid = out["valid"].data_ptr()
    call_desc("gnnlm_pq_gather_decode", d)
    return out


def token_gather(embed, vals, ids, left=0, right=0, n_store=None, n_vocab=None, want_x=True, want_labels=False, want_valid=True,
                 n_groups_dev=None, out_x=None):
    """``--reinit-nfeat``: the token-embedding rows of the slots of each centre row in ``ids`` (flattened) -- the counterpart of
    :func:`pq_gather_decode` for a label-only store (transformer.py:1046-1048).  embed [V, d] f32 (row stride may exceed d), vals
    [n_store] int16 / int32 (the whole label table).  Returns a dict (x [n_slots, d] with zero rows for invalid slots, labels
    int32 with -1, valid uint8).  ``out_x``: write the rows into this [n_slots, >= d] buffer instead (its row stride is used)."""
    _dev(embed, vals, ids, n_groups_dev, out_x)
    _f32(embed, out_x)
    _dtype(ids, torch.int64, "ids"), _dtype(n_groups_dev, torch.int32, "n_groups_dev")
    if vals.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"vals: expected int16 or int32, got {vals.dtype}")
    n_g = 1 + left + right
    G = ids.numel()
    S = G * n_g
    dev = embed.device
    t = _lib.gnnlm_token_gather_t()
    t.ids, t.n_groups, t.left, t.right = ids.data_ptr(), G, left, right
    t.n_store = n_store if n_store is not None else vals.shape[0]
    if t.n_store > vals.shape[0]:
        raise ValueError(f"token_gather: n_store = {t.n_store} but the label table has {vals.shape[0]} rows (it is never sharded)")
    t.vals, t.vals_itemsize = vals.data_ptr(), vals.element_size()
    t.n_vocab, t.d = (n_vocab if n_vocab is not None else embed.shape[0]), embed.shape[1]
    if t.n_vocab > embed.shape[0]:
        raise ValueError(f"token_gather: n_vocab = {t.n_vocab} but the table has {embed.shape[0]} rows")
    t.embed, t.ld_embed = embed.data_ptr(), embed.stride(0)
    out = {}
    if want_x or out_x is not None:
        if out_x is None:
            out_x = torch.empty(S, embed.shape[1], device=dev, dtype=torch.float32)
        assert out_x.shape[0] >= S and out_x.shape[1] >= embed.shape[1]
        out["x"] = out_x
        t.out_x, t.ld_x = out_x.data_ptr(), out_x.stride(0)
    if want_labels:
        out["labels"] = torch.empty(S, device=dev, dtype=torch.int32)
        t.out_labels = out["labels"].data_ptr()
    if want_valid:
        out["valid"] = torch.empty(S, device=dev, dtype=torch.uint8)
        t.out_valid = out["valid"].data_ptr()
    if n_groups_dev is not None:
        t.n_groups_dev = n_groups_dev.data_ptr()
    call_desc("gnnlm_token_gather", t)
    return out


def neighbor_labels(ids, vals, n_store=None, n_vocab=None):
    """int32, shaped like ``ids``: the label of every neighbour, -1 where ``ids`` names no row of the store (or the label lies
    outside [0, n_vocab)) -- the index through which layer 0's star edges read the embedding table (``gnnlm_star_attn_t.x_index``)."""
    _dev(ids, vals)
    _dtype(ids, torch.int64, "ids")
    if vals.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"vals: expected int16 or int32, got {vals.dtype}")
    n_store = n_store if n_store is not None else vals.shape[0]
    if n_store > vals.shape[0]:
        raise ValueError(f"neighbor_labels: n_store = {n_store} but the label table has {vals.shape[0]} rows")
    out = torch.empty(ids.shape, device=ids.device, dtype=torch.int32)
    call("gnnlm_neighbor_labels", ptr(ids), ids.numel(), n_store, ptr(vals), vals.element_size(),
         n_vocab if n_vocab is not None else 2 ** 31 - 1, ptr(out), stream())
    return out


def pq_lookup_direct(codes, centroids):
    """x[n, m*dsub:(m+1)*dsub] = centroids[m, codes[n, m]] for an explicit code matrix (no store)."""
    _dev(codes, centroids)
    n, M = codes.shape
    dsub = centroids.shape[2]
    x = torch.empty(n, M * dsub, device=codes.device, dtype=torch.float32)
    valid = torch.ones(n, device=codes.device, dtype=torch.uint8)
    d = _lib.gnnlm_gather_t()
    d.codes, d.direct, d.in_valid = codes.data_ptr(), 1, valid.data_ptr()
    d.M, d.dsub, d.centroids = M, dsub, centroids.data_ptr()
    d.n_groups, d.vals_itemsize = n, 4
    d.out_x, d.ld_x = x.data_ptr(), M * dsub
    call_desc("gnnlm_pq_gather_decode", d)
    return x


def star_attn(U, ids, codes=None, centroids=None, row0=0, X=None, x_group_stride=1, codes_direct=0, n_store=None,
              nb_valid=None, nb_valid_stride=1, shards=None, rows_per_rank=0, x_index=None):
    """n_store: rows of the whole store (ids >= n_store are not neighbours; default: the rows of ``codes``);
    nb_valid (uint8): validity byte of neighbour (i, j) at [(i*kg + j) * nb_valid_stride];
    shards = [(codes_g [rows_g, M], first global row), ...] + rows_per_rank: a range-sharded table whose shards are all
    mapped into this process (instead of ``codes``; needs ``n_store``)."""
    _dev(U, ids, codes, centroids, X, nb_valid)
    _f32(U, centroids, X)
    _dtype(ids, torch.int64, "ids"), _dtype(codes, torch.uint8, "codes"), _dtype(nb_valid, torch.uint8, "nb_valid")
    _dtype(x_index, torch.int32, "x_index"), _dev(x_index)
    T, H, D = U.shape
    kg = ids.shape[1]
    Z = torch.empty_like(U)
    has_nb = torch.empty(T, device=U.device, dtype=torch.float32)
    a = _lib.gnnlm_star_attn_t()
    a.U, a.ids = U.data_ptr(), ids.data_ptr()
    a.T, a.H, a.D, a.kg = T, H, D, kg
    if shards:
        from .hgt import CodeStore, shards_device_ptr
        keep = CodeStore(codes=None, centroids=centroids, n_store=n_store, shards=shards, rows_per_rank=rows_per_rank)
        a.shards = shards_device_ptr(keep)
        a.M, a.dsub = centroids.shape[0], centroids.shape[2]
        a.centroids = centroids.data_ptr()
    elif codes is not None:
        a.codes, a.row0, a.n_local = codes.data_ptr(), row0, codes.shape[0]
        a.M, a.dsub = centroids.shape[0], centroids.shape[2]
        a.centroids = centroids.data_ptr()
        a.codes_direct = codes_direct
        if n_store is None and not codes_direct:
            n_store = row0 + codes.shape[0]
    else:
        a.X, a.ldx, a.x_group_stride = X.data_ptr(), X.stride(0), x_group_stride
    a.Z, a.has_nb = Z.data_ptr(), has_nb.data_ptr()
    a.n_store = n_store or 0
    if nb_valid is not None:
        a.nb_valid, a.nb_valid_stride = nb_valid.data_ptr(), nb_valid_stride
    if x_index is not None:                                     # [T, kg] int32: dense row / validity byte of (i, j) (-1: not a neighbour)
        a.x_index = x_index.data_ptr()
    call_desc("gnnlm_star_attn", a)
    if shards:
        Z._gnnlm_keep = keep                                    # the device copy of the shard table outlives the queued launch
    return Z, has_nb


def chain_attn(Q, K, V, valid, left, right, H, scale=None):
    _dev(Q, K, V, valid, scale)
    S, d = Q.shape
    n_g = 1 + left + right
    out = torch.empty_like(Q)
    c = _lib.gnnlm_chain_attn_t()
    c.Q, c.K, c.V, c.ld = Q.data_ptr(), K.data_ptr(), V.data_ptr(), Q.stride(0)
    c.valid = valid.data_ptr()
    c.n_groups, c.left, c.right, c.H, c.dk = S // n_g, left, right, H, d // H
    if scale is not None:
        c.scale = scale.data_ptr()
    c.out, c.ldo = out.data_ptr(), out.stride(0)
    call_desc("gnnlm_chain_attn", c)
    return out


def causal_attn(Q, K, V, n_blocks, T, H, max_ctx=0):
    """Fused causal attention (T = 256, d_k = 128): Q, K', V' [n_blocks*T, H*dk] -> [n_blocks*T, H*dk]."""
    _f32(Q), _f32(K), _f32(V)
    _dev(Q, K, V)
    d = Q.shape[1]
    out = torch.empty_like(Q)
    call("gnnlm_causal_attn", ptr(Q), ptr(K), ptr(V), Q.stride(0), ptr(out), out.stride(0), n_blocks, T, H, d // H,
         max_ctx, stream())
    return out


def causal_attn_varlen(Q, K, V, block_off, H, max_ctx=0, out=None):
    """Causal attention over packed blocks of unequal length in one launch: Q, K', V' [n_tok, H*dk] (row stride may exceed it),
    ``block_off`` a :class:`ragged.RaggedBatch` or offsets [n_blocks + 1] -> [n_tok, H*dk].  d_k in {16, 32, 64, 128}."""
    from .ragged import as_ragged
    _f32(Q), _f32(K), _f32(V), _f32(out)
    _dev(Q, K, V, out)
    rg = as_ragged(block_off, Q.device)
    if rg.n_tok != Q.shape[0] or K.shape != Q.shape or V.shape != Q.shape or K.stride(0) != Q.stride(0) or V.stride(0) != Q.stride(0):
        raise ValueError("causal_attn_varlen: Q, K, V must share shape and row stride, with block_off[-1] - block_off[0] rows")
    d = Q.shape[1]
    if out is None:
        out = torch.empty(Q.shape, device=Q.device, dtype=torch.float32)
    desc = rg.desc()
    call("gnnlm_causal_attn_varlen", ptr_strided(Q), ptr_strided(K), ptr_strided(V), Q.stride(0), ptr_strided(out), out.stride(0),
         ctypes.byref(desc), H, d // H, max_ctx, stream())
    return out


def kv_cache_desc(k, v, lens, done=None, n_bad=None):
    """A filled ``gnnlm_kv_cache_t`` over ``k`` / ``v`` f32 [L, B, cap, d] (views with wider strides welcome: unit element stride, the
    rest multiples of 4), ``lens`` int32 [B], optional ``done`` int32 [B] and ``n_bad`` int32 [1] -- all on the device."""
    _f32(k, v)
    _dtype(lens, torch.int32, "lens"), _dtype(done, torch.int32, "done"), _dtype(n_bad, torch.int32, "n_bad")
    for t in (k, v, lens, done, n_bad):
        if t is not None and not t.is_cuda:
            raise _lib.GnnlmError("gnnlm_amd kernels need device (HIP) tensors; there is no CPU fallback")
    if k.dim() != 4 or v.shape != k.shape or v.stride() != k.stride() or (k.stride(3) != 1 and k.shape[3] > 1):
        raise ValueError("kv_cache: k and v must be [L, B, cap, d] with the same strides and unit element stride")
    L, B, cap, d = k.shape
    if lens.shape != (B,) or not lens.is_contiguous() or (done is not None and (done.shape != (B,) or not done.is_contiguous())):
        raise ValueError("kv_cache: lens / done must be contiguous [B]")
    c = _lib.gnnlm_kv_cache_t()
    c.k, c.v = k.data_ptr(), v.data_ptr()
    c.ld_row = k.stride(2) if cap > 1 else max(k.stride(2), d)
    c.ld_seq = k.stride(1) if B > 1 else max(k.stride(1), cap * c.ld_row)
    c.ld_layer = k.stride(0) if L > 1 else max(k.stride(0), B * c.ld_seq)
    c.L, c.B, c.cap, c.d = L, B, cap, d
    c.len = lens.data_ptr()
    c.done = done.data_ptr() if done is not None else None
    c.n_bad = n_bad.data_ptr() if n_bad is not None else None
    return c


def _decode_attn_desc(a, what, q, k_new, v_new, k, v, lens, layer, H, done, n_bad, max_len, out, workspace):
    """Fill the ``gnnlm_decode_attn_t`` ``a`` (checks, the output and the workspace included) -> (out, workspace, the cache descriptor)."""
    _f32(q, k_new, v_new, out)
    _dev(q, k_new, v_new, out)
    c = kv_cache_desc(k, v, lens, done, n_bad)
    if q.dim() != 2 or q.shape != (c.B, c.d) or k_new.shape != q.shape or v_new.shape != q.shape or \
            k_new.stride(0) != q.stride(0) or v_new.stride(0) != q.stride(0):
        raise ValueError(f"{what}: q, k_new, v_new must be [B, d] with one row stride")
    if out is None:
        out = torch.empty(c.B, c.d, device=q.device, dtype=torch.float32)
    dk = c.d // H
    need = _lib.lib().gnnlm_decode_attn_workspace_bytes(c.B, H, dk, max_len or c.cap)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(max(need, 16), device=q.device, dtype=torch.uint8)
    a.q, a.k_new, a.v_new, a.ld = q.data_ptr(), k_new.data_ptr(), v_new.data_ptr(), max(q.stride(0), c.d)
    a.out, a.ldo = out.data_ptr(), max(out.stride(0), c.d)
    a.cache, a.layer, a.H, a.dk, a.max_len = c, int(layer), int(H), dk, int(max_len)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return out, workspace, c


def decode_attn(q, k_new, v_new, k, v, lens, layer, H, done=None, n_bad=None, max_len=0, out=None, workspace=None):
    """One new row per sequence against the K/V cache (``gnnlm_decode_attn``): ``q`` / ``k_new`` / ``v_new`` [B, H*dk] f32 sharing one row
    stride (q already scaled), the cache as in :func:`kv_cache_desc` -> ``out`` [B, H*dk].  Row b with ``done[b] == 0`` and
    ``0 <= lens[b] < cap`` gets ``k_new[b]`` / ``v_new[b]`` written to cache row ``lens[b]`` of ``layer`` and attends keys
    ``0 .. lens[b]``; any other row gets zeros (one outside the range is counted in ``n_bad``).  ``lens`` is not changed.
    ``max_len``: host bound on ``lens[b] + 1`` (0: cap).  d_k in {16, 32, 64, 128}; the result of a row is bit-reproducible and depends
    on that row alone."""
    a = _lib.gnnlm_decode_attn_t()
    out, workspace, _ = _decode_attn_desc(a, "decode_attn", q, k_new, v_new, k, v, lens, layer, H, done, n_bad, max_len, out, workspace)
    call_desc("gnnlm_decode_attn", a)
    return out


def sample_topk(logp, ids, u=None, pad=1, eos=2, done=None, n_bad=None, out=None, out_logp=None, want_logp=True):
    """The next token of every row from its sorted top-N (``gnnlm_sample_topk``): ``logp`` f32 / ``ids`` i64 [B, N] best first, as
    :func:`topk_merge` leaves them.  ``u`` None: greedy (column 0); ``u`` f32 [B] in [0, 1): the smallest j whose inclusive prefix sum of
    ``exp(logp_j - logp_0)`` exceeds ``u * total`` (search.py:231-247 with the caller's random numbers).  -> ``(next i64 [B], next_logp f32
    [B] or None)``; ``done`` int32 [B] (optional, updated in place): a done row gets ``pad``, a pick of ``eos`` sets it."""
    _dev(logp, ids, u, done, n_bad, out, out_logp)
    _f32(logp, u, out_logp)
    _dtype(ids, torch.int64, "ids"), _dtype(out, torch.int64, "out"), _dtype(done, torch.int32, "done"), _dtype(n_bad, torch.int32, "n_bad")
    if logp.dim() != 2 or ids.shape != logp.shape:
        raise ValueError("sample_topk: logp / ids [B, N]")
    B, N = logp.shape
    for t in (u, done, out, out_logp):
        if t is not None and (t.shape != (B,) or not t.is_contiguous()):
            raise ValueError("sample_topk: u / done / out / out_logp must be contiguous [B]")
    if out is None:
        out = torch.empty(B, device=logp.device, dtype=torch.int64)
    if out_logp is None and want_logp:
        out_logp = torch.empty(B, device=logp.device, dtype=torch.float32)
    s = _lib.gnnlm_sample_topk_t()
    s.logp, s.ld_logp = logp.data_ptr(), _row_stride(logp)
    s.ids, s.ld_ids = ids.data_ptr(), _row_stride(ids)
    s.B, s.N = B, N
    s.u = u.data_ptr() if u is not None else None
    s.pad, s.eos = int(pad), int(eos)
    s.next = out.data_ptr()
    s.next_logp = out_logp.data_ptr() if out_logp is not None else None
    s.done = done.data_ptr() if done is not None else None
    s.n_bad = n_bad.data_ptr() if n_bad is not None else None
    call_desc("gnnlm_sample_topk", s)
    return out, out_logp


def sample_topp(logp, topp, u, pad=1, eos=2, done=None, n_bad=None, out=None, out_logp=None, want_logp=True, n_keep=None, keep_mass=None):
    """Nucleus sampling over dense rows (``gnnlm_sample_topp``): ``logp`` f32 [B, V] (rows contiguous, any row stride), ``topp`` > 0
    (``inf``: the whole vocabulary), ``u`` f32 [B] in [0, 1).  The nucleus is the shortest prefix of the row's order (larger value
    first, then smaller id) whose unnormalised mass ``sum exp(logp)`` reaches ``topp`` (search.py:174-217); the pick is the smallest id
    whose prefix sum of nucleus masses, in ascending id, exceeds ``u * S``.  -> ``(next i64 [B], next_logp f32 [B] or None)``;
    ``done`` / ``n_bad`` as in :func:`sample_topk`; ``n_keep`` int32 [B] / ``keep_mass`` f32 [B] (optional outputs): the nucleus size and
    mass.  No workspace, nothing read back."""
    _dev(logp, u, done, n_bad, out, out_logp, n_keep, keep_mass)
    _f32(logp, u, out_logp, keep_mass)
    _dtype(out, torch.int64, "out"), _dtype(done, torch.int32, "done"), _dtype(n_bad, torch.int32, "n_bad"), _dtype(n_keep, torch.int32, "n_keep")
    if logp.dim() != 2 or (logp.shape[1] > 1 and logp.stride(1) != 1):
        raise ValueError("sample_topp: logp [B, V] with contiguous rows")
    if u is None:
        raise ValueError("sample_topp: u is required")
    B, V = logp.shape
    for t in (u, done, out, out_logp, n_keep, keep_mass):
        if t is not None and (t.shape != (B,) or not t.is_contiguous()):
            raise ValueError("sample_topp: u / done / out / out_logp / n_keep / keep_mass must be contiguous [B]")
    if out is None:
        out = torch.empty(B, device=logp.device, dtype=torch.int64)
    if out_logp is None and want_logp:
        out_logp = torch.empty(B, device=logp.device, dtype=torch.float32)
    s = _lib.gnnlm_sample_topp_t()
    s.logp, s.ld = logp.data_ptr(), _row_stride(logp)
    s.B, s.V, s.topp = B, V, float(topp)
    s.u = u.data_ptr()
    s.pad, s.eos = int(pad), int(eos)
    s.next = out.data_ptr()
    for name, t in (("next_logp", out_logp), ("done", done), ("n_bad", n_bad), ("n_keep", n_keep), ("keep_mass", keep_mass)):
        setattr(s, name, t.data_ptr() if t is not None else None)
    call_desc("gnnlm_sample_topp", s)
    return out, out_logp


def _src_table(src, B, cap, what):
    _dtype(src, torch.int32, "src")
    if not src.is_cuda or src.dim() != 2 or src.shape[0] != B or src.shape[1] < cap or (src.stride(1) != 1 and src.shape[1] > 1) or \
            (B > 1 and src.stride(0) < src.shape[1]):
        raise ValueError(f"{what}: src must be a device int32 [{B}, >= {cap}] table with contiguous rows")
    return max(src.stride(0), src.shape[1])


def beam_attn(q, k_new, v_new, k, v, lens, src, layer, H, done=None, n_bad=None, max_len=0, out=None, workspace=None):
    """:func:`decode_attn` through a table of cache slots (``gnnlm_beam_attn``): ``src`` int32 [B, >= cap], key row ``u < lens[s]`` of
    hypothesis s is row u of cache sequence ``src[s, u]``; the new row goes to row ``lens[s]`` of sequence s itself.  Given the same
    rows in the same order the output is the bits of :func:`decode_attn` on a contiguous cache.  An entry outside [0, B) below
    ``lens[s]`` is never followed: the row gets zeros and is counted in ``n_bad``."""
    b = _lib.gnnlm_beam_attn_t()
    out, workspace, c = _decode_attn_desc(b.a, "beam_attn", q, k_new, v_new, k, v, lens, layer, H, done, n_bad, max_len, out, workspace)
    b.src, b.ld_src = src.data_ptr(), _src_table(src, c.B, c.cap, "beam_attn")
    call_desc("gnnlm_beam_attn", b)
    return out


def beam_select(cand_val, cand_id, state, src=None, src_out=None, eos=2, pad=1):
    """One beam-search step of every sentence (``gnnlm_beam_select``): ``cand_val`` f32 / ``cand_id`` i64 [B * beam_in, N], the sorted
    top-N of every hypothesis row as :func:`topk_merge` leaves it (``beam_in`` 1 at the first step, ``beam`` afterwards; N >= 2 * beam).
    ``state``: anything with the attributes ``beam``, ``max_new`` and the device tensors ``score`` f32 [B, beam] (updated in place), ``t`` /
    ``finished`` / ``fin_n`` int32 [B], ``len`` / ``done`` int32 [B * beam] (the cache's), ``next`` i64 / ``parent`` int32 [B * beam],
    ``hist_tok`` i64 / ``hist_par`` int32 / ``hist_score`` f32 [B, max_new + 1, beam], ``fin_tok`` i64 / ``fin_cum`` f32 [B, beam, max_new + 1],
    ``fin_len`` int32 / ``fin_score`` f32 [B, beam] (``beam_search.BeamState`` is one).  ``src`` int32 [B * beam, cap]: the table of cache
    slots, updated in place (or into ``src_out``).  The rules are the header's; nothing is read back."""
    d = _lib.gnnlm_beam_select_t()
    _beam_select_desc(d, cand_val, cand_id, state, src, src_out, eos, pad)
    call_desc("gnnlm_beam_select", d)
    return state.next, state.parent


def beam_select_diverse(cand_val, cand_id, state, src=None, src_out=None, eos=2, pad=1, groups=1, strength=0.5, rate=0.0):
    """:func:`beam_select` with the step's candidates drawn by diverse groups or with the sibling penalty (``gnnlm_beam_select_diverse``):
    ``groups`` G divides ``state.beam``; group g owns the hypotheses g, g + G, .. and a candidate's value is lowered by ``strength`` for every
    time the groups before its own chose its token at this step; the groups' lists are interleaved, not sorted again.  ``rate`` (with
    ``groups`` 1): the c-th best candidate of a hypothesis loses ``c * rate``.  ``groups=1, rate=0`` gives :func:`beam_select`'s results."""
    d = _lib.gnnlm_beam_select_diverse_t()
    _beam_select_desc(d.sel, cand_val, cand_id, state, src, src_out, eos, pad)
    d.groups, d.strength, d.rate = int(groups), float(strength), float(rate)
    call_desc("gnnlm_beam_select_diverse", d)
    return state.next, state.parent


def _beam_select_desc(d, cand_val, cand_id, state, src, src_out, eos, pad):
    """Fill a ``gnnlm_beam_select_t`` from the arguments of :func:`beam_select`."""
    _dev(cand_val, cand_id)
    _f32(cand_val, state.score, state.hist_score, state.fin_cum, state.fin_score)
    _dtype(cand_id, torch.int64, "cand_id")
    for name in ("next", "hist_tok", "fin_tok"):
        _dtype(getattr(state, name), torch.int64, name)
    for name in ("t", "finished", "fin_n", "len", "done", "parent", "hist_par", "fin_len"):
        _dtype(getattr(state, name), torch.int32, name)
    B, beam, T1 = state.t.shape[0], int(state.beam), int(state.max_new) + 1
    if cand_val.dim() != 2 or cand_id.shape != cand_val.shape or (B and cand_val.shape[0] % B):
        raise ValueError("beam_select: cand_val / cand_id [B * beam_in, N]")
    shapes = {"score": (B, beam), "t": (B,), "finished": (B,), "fin_n": (B,), "len": (B * beam,), "done": (B * beam,), "next": (B * beam,),
              "parent": (B * beam,), "hist_tok": (B, T1, beam), "hist_par": (B, T1, beam), "hist_score": (B, T1, beam),
              "fin_tok": (B, beam, T1), "fin_cum": (B, beam, T1), "fin_len": (B, beam), "fin_score": (B, beam)}
    for name, shp in shapes.items():
        x = getattr(state, name)
        if tuple(x.shape) != shp or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"beam_select: state.{name} must be a contiguous device tensor {shp}")
    d.cand_val, d.ld_val = cand_val.data_ptr(), _row_stride(cand_val)
    d.cand_id, d.ld_id = cand_id.data_ptr(), _row_stride(cand_id)
    d.B, d.beam, d.beam_in, d.N = B, beam, cand_val.shape[0] // B if B else 1, cand_val.shape[1]
    d.eos, d.pad, d.max_new = int(eos), int(pad), int(state.max_new)
    d.score_in = d.score_out = state.score.data_ptr()
    d.t, d.finished, d.fin_n = state.t.data_ptr(), state.finished.data_ptr(), state.fin_n.data_ptr()
    d.len, d.done = state.len.data_ptr(), state.done.data_ptr()
    d.next, d.parent = state.next.data_ptr(), state.parent.data_ptr()
    d.hist_tok, d.hist_par, d.hist_score = state.hist_tok.data_ptr(), state.hist_par.data_ptr(), state.hist_score.data_ptr()
    d.fin_tok, d.fin_cum = state.fin_tok.data_ptr(), state.fin_cum.data_ptr()
    d.fin_len, d.fin_score = state.fin_len.data_ptr(), state.fin_score.data_ptr()
    if src is not None:
        dst = src if src_out is None else src_out
        d.cap = src.shape[1]
        d.ld_src = _src_table(src, B * beam, d.cap, "beam_select")
        if _src_table(dst, B * beam, d.cap, "beam_select") != d.ld_src or dst.shape != src.shape:
            raise ValueError("beam_select: src and src_out must share shape and row stride")
        d.src_in, d.src_out = src.data_ptr(), dst.data_ptr()


def ptr_strided(t):
    """Device pointer of a 2-D tensor whose rows are contiguous (row stride >= width)."""
    if t.dim() != 2 or t.stride(1) != 1:
        raise _lib.GnnlmError("expected a 2-D tensor with contiguous rows")
    return ctypes.c_void_p(t.data_ptr())


def causal_softmax_(S, T, max_ctx=0):
    """In place over S [n_mats, T, ld]."""
    n_mats, T_, ld = S.shape
    assert T_ == T
    call("gnnlm_causal_softmax", ptr(S), n_mats, T, ld, max_ctx, stream())
    return S


def layernorm(x, gamma, beta, eps=1e-5, valid=None):
    rows, d = x.shape
    out = torch.empty_like(x)
    call("gnnlm_layernorm", ptr(x), x.stride(0), ptr(gamma), ptr(beta), ptr(out), out.stride(0), rows, d, eps,
         ptr(valid), stream())
    return out


def gelu_(x):
    """In place, exact (erf) GELU == torch.nn.functional.gelu's default."""
    _dev(x)
    _f32(x)
    assert x.is_contiguous()
    call("gnnlm_gelu", ptr(x), x.numel(), stream())
    return x


def relu_(x):
    """In place max(x, 0) (a NaN stays a NaN, as torch.relu): the feed-forward activation of the base transformer LM."""
    _dev(x)
    _f32(x)
    assert x.is_contiguous()
    call("gnnlm_relu", ptr(x), x.numel(), stream())
    return x


def lm_embed(tokens, E, block_off, P=None, pad_idx=1, scale=1.0, out=None, n_bad=None):
    """x[r] = fl32(fl32(scale * E[tokens[r]]) + P[pad_idx + 1 + position of r in its block]) for the packed rows of ``block_off`` (a
    :class:`ragged.RaggedBatch` or offsets [n_blocks + 1]): the input of the base transformer LM (transformer.py:753-759).  ``P`` None:
    no positional embedding.  A token id outside [0, V) gives a zero row and is counted in ``n_bad`` (device int32 [1], added to).  A
    block longer than ``P`` holds is refused before anything is launched."""
    from .ragged import as_ragged
    _f32(E, P, out)
    _dtype(tokens, torch.int64, "tokens"), _dtype(n_bad, torch.int32, "n_bad")
    _dev(tokens, E, P, out, n_bad)
    rg = as_ragged(block_off, tokens.device)
    if tokens.dim() != 1 or rg.n_tok != tokens.shape[0]:
        raise ValueError("lm_embed: tokens must be [n_tok] with n_tok = block_off[-1] - block_off[0]")
    d = E.shape[1]
    if out is None:
        out = torch.empty(rg.n_tok, d, device=tokens.device, dtype=torch.float32)
    e = _lib.gnnlm_lm_embed_t()
    e.tokens = tokens.data_ptr()
    e.E, e.ld_e, e.n_vocab, e.d = E.data_ptr(), E.stride(0), E.shape[0], d
    if P is not None:
        e.P, e.ld_p, e.p_rows = P.data_ptr(), P.stride(0), P.shape[0]
    e.pad_idx, e.scale, e.max_len = int(pad_idx), float(scale), int(rg.lengths.max()) if rg.n_blocks else 0
    e.out, e.ldo = out.data_ptr(), out.stride(0)
    e.n_bad = n_bad.data_ptr() if n_bad is not None else None
    desc = rg.desc()
    call("gnnlm_lm_embed", ctypes.byref(e), ctypes.byref(desc), stream())
    return out


def pack_rows(src, block_off, skip, out_off, d, want_rows=True, want_unit=False, out=None, n_bad=None):
    """The taken rows of packed blocks as contiguous matrices (``gnnlm_pack_rows``): block b of ``src`` [n_tok, >= d] (f32, row stride
    free) is the rows ``block_off[b] - block_off[0] .. block_off[b + 1] - block_off[0]``, its first ``skip[b]`` rows (the context) are
    left out, and the rest lands at output rows ``out_off[b] ..``.  ``block_off`` / ``out_off`` int32 [n_blocks + 1] and ``skip`` int32
    [n_blocks] or None are DEVICE tensors (a driver keeps one table per split and hands views).  -> ``(rows, unit)``: the rows bit for
    bit (``want_rows``) and ``row / sqrt(sum(row ** 2))`` in float32 (``want_unit``: the query of a cosine index, knn_model.py:181-184),
    None for what is not wanted.  ``out``: a pair of [n_out, d] f32 tensors (row stride free) to write into, either may be None.
    The tables are checked on the device: ``n_bad`` None -- the call waits for the count of violations (4 bytes) and raises before it
    packs anything; ``n_bad`` (device int32 [1], added to) -- nothing is read back, the caller looks at it with its results (rows the
    tables do not describe are never read or written)."""
    _f32(src)
    for t, what in ((block_off, "block_off"), (skip, "skip"), (out_off, "out_off"), (n_bad, "n_bad")):
        _dtype(t, torch.int32, what)
    _dev(src, block_off, skip, out_off, n_bad)
    if src.dim() != 2 or block_off.dim() != 1 or out_off.shape != block_off.shape or (skip is not None and skip.shape[0] != block_off.shape[0] - 1):
        raise ValueError("pack_rows: src [n_tok, ld], block_off / out_off [n_blocks + 1], skip [n_blocks]")
    if not (want_rows or want_unit):
        raise ValueError("pack_rows: nothing is wanted (want_rows and want_unit are both False)")
    n_blocks = block_off.shape[0] - 1
    d = int(d)
    if d > src.shape[1]:
        raise ValueError(f"pack_rows: d = {d}, src has {src.shape[1]} columns")
    rows_out, unit_out = out if out is not None else (None, None)
    if rows_out is None and unit_out is None:
        n_out = int(out_off[-1].item())                      # (a convenience: a driver hands its output buffers and reads nothing back)
    else:
        n_out = int((rows_out if rows_out is not None else unit_out).shape[0])
    if want_rows and rows_out is None:
        rows_out = torch.empty(n_out, d, device=src.device, dtype=torch.float32)
    if want_unit and unit_out is None:
        unit_out = torch.empty(n_out, d, device=src.device, dtype=torch.float32)
    rows_out, unit_out = rows_out if want_rows else None, unit_out if want_unit else None
    _f32(rows_out, unit_out)
    _dev(rows_out, unit_out)
    for t in (rows_out, unit_out):
        if t is not None and (t.dim() != 2 or t.shape[0] != n_out or t.shape[1] < d):
            raise ValueError(f"pack_rows: an output must be [n_out = {n_out}, >= {d}]")
    q = _lib.gnnlm_pack_rows_t()
    q.src, q.ld_src = src.data_ptr(), src.stride(0)
    q.block_off, q.out_off = block_off.data_ptr(), out_off.data_ptr()
    q.skip = skip.data_ptr() if skip is not None else None
    if rows_out is not None:
        q.dst, q.ld_dst = rows_out.data_ptr(), rows_out.stride(0)
    if unit_out is not None:
        q.dst_unit, q.ld_unit = unit_out.data_ptr(), unit_out.stride(0)
    q.n_blocks, q.d, q.n_tok, q.n_out = n_blocks, d, src.shape[0], n_out
    count = n_bad if n_bad is not None else torch.zeros(1, device=src.device, dtype=torch.int32)
    q.n_bad, q.wait = count.data_ptr(), int(n_bad is None)
    call_desc("gnnlm_pack_rows", q)
    return rows_out, unit_out


def half_to_float(x):
    out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    call("gnnlm_half_to_float", ptr(x), ptr(out), x.numel(), stream())
    return out


def filter_neighbors(ids, tok_pos, invalid_ctx, out=None):
    """``--invalid-neighbor-context`` (token_block_dataset.py:360-362): ids [n, kg] i64, tok_pos [n] i64 -> ids with the
    neighbours inside their own token's context replaced by -1 (the graph consumers skip -1 ids)."""
    _dev(ids, tok_pos)
    _dtype(ids, torch.int64, "ids"), _dtype(tok_pos, torch.int64, "tok_pos")
    n, kg = ids.shape
    assert tok_pos.shape == (n,) and ids.is_contiguous() and tok_pos.is_contiguous()
    out = torch.empty_like(ids) if out is None else out
    call("gnnlm_filter_neighbors", ptr(ids), ptr(tok_pos), n, kg, int(invalid_ctx), ptr(out), stream())
    return out


def row_lse_pick(logits, pick=None):
    rows, n = logits.shape
    lse = torch.empty(rows, device=logits.device, dtype=torch.float32)
    picked = torch.empty(rows, device=logits.device, dtype=torch.float32)
    call("gnnlm_row_lse_pick", ptr(logits), logits.stride(0), rows, None, n, ptr(pick), ptr(lse), ptr(picked), stream())
    return lse, picked


_TAG_TABLES = {}                     # id(vals) -> (weakref to vals, version, tag table)
TAG_TABLE_MIN_ROWS = 1 << 20         # below this the label table sits in the L2 anyway


def label_tags(vals, build=True):
    """The one-byte tag table of a label table (``gnnlm_label_tags``; see ``gnnlm_knn_interp_t.vals_tag``), built once per
    table and kept while the table lives (keyed on the tensor object and its in-place version counter).  ``build=False``:
    only what is cached (inside a stream capture nothing may be allocated or launched on the side)."""
    import weakref
    for k_ in [k_ for k_, (ref, _, _) in _TAG_TABLES.items() if ref() is None]:
        del _TAG_TABLES[k_]
    hit = _TAG_TABLES.get(id(vals))
    if hit is not None and hit[0]() is vals and hit[1] == vals._version:
        return hit[2]
    if not build:
        return None
    assert vals.dim() == 1 and vals.is_contiguous() and vals.dtype in (torch.int16, torch.int32)
    tag = torch.empty(vals.shape[0], dtype=torch.uint8, device=vals.device)
    call("gnnlm_label_tags", ptr(vals), vals.element_size(), vals.shape[0], ptr(tag), stream())
    _TAG_TABLES[id(vals)] = (weakref.ref(vals), vals._version, tag)
    return tag


_KNN_SCRATCH = {}                    # (device, stream) -> scratch of the routed look-ups (knn_bucket.hip)
_KNN_SCRATCH_CAPTURED = []           # scratch buffers whose addresses live in captured HIP graphs: kept for good
KNN_BUCKET_MIN_LOOKUPS = 1 << 20     # below this the one-pass kernel is as fast (three launches against one)


def knn_interp(lm_logp, sims, ids, targets, temperature, lmbda, vals=None, n_store=None, row0=0, knn_vals=None, vals_tag="auto",
               bucketed="auto"):
    """``vals_tag``: "auto" = gather through the one-byte tag table (built on first use) when the label table is large and
    k fits the register kernel; True / False force it on / off (tests, A/B).  ``bucketed``: "auto" = with the tag table and at
    least 2^20 look-ups, route the look-ups region by region through the L2 (gnnlm_knn_interp_t.scratch); True / False force."""
    _dev(lm_logp, sims, ids, targets, vals, knn_vals)
    _f32(lm_logp, sims)
    _dtype(ids, torch.int64, "ids"), _dtype(targets, torch.int64, "targets")
    if vals is not None and vals.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"vals: expected int16 / int32, got {vals.dtype}")
    n, k = sims.shape
    dev = sims.device
    out = torch.empty(n, device=dev, dtype=torch.float32)
    pk = torch.empty(n, device=dev, dtype=torch.float32)
    rec = torch.empty(n, device=dev, dtype=torch.int64)
    d = _lib.gnnlm_knn_interp_t()
    d.lm_logp, d.sims, d.ids, d.targets = lm_logp.data_ptr(), sims.data_ptr(), ids.data_ptr(), targets.data_ptr()
    d.vals_itemsize = 4
    if vals is not None:
        d.vals, d.vals_itemsize = vals.data_ptr(), vals.element_size()
        d.n_local = vals.shape[0]
        d.n_store = n_store if n_store is not None else vals.shape[0]
        d.row0 = row0
    if knn_vals is not None:
        assert knn_vals.dtype == torch.int32
        d.knn_vals = knn_vals.data_ptr()
    elif vals is not None and vals.dim() == 1 and vals.is_contiguous() and k <= 1024 and \
            (vals_tag is True or (vals_tag == "auto" and vals.shape[0] >= TAG_TABLE_MIN_ROWS)):
        capturing = torch.cuda.is_current_stream_capturing()
        tag = label_tags(vals, build=not capturing)
        if tag is not None:
            d.vals_tag = tag.data_ptr()
            if bucketed is True or (bucketed == "auto" and n * k >= KNN_BUCKET_MIN_LOOKUPS):
                need = _lib.lib().gnnlm_knn_interp_scratch_bytes(n, k, vals.shape[0])
                key = (str(dev), _lib.raw_stream(dev))
                sc = _KNN_SCRATCH.get(key)
                if (sc is None or sc.numel() < need) and not capturing and n <= (1 << 16) and vals.shape[0] <= (1 << 27):
                    sc = _KNN_SCRATCH[key] = torch.empty(need, dtype=torch.uint8, device=dev)
                if sc is not None and sc.numel() >= need:
                    d.scratch, d.scratch_bytes = sc.data_ptr(), sc.numel()
                    if capturing and not any(t is sc for t in _KNN_SCRATCH_CAPTURED):
                        # its address is baked into a HIP graph: a later, larger request replaces the dictionary entry, but this
                        # buffer must outlive every replay (never freed)
                        _KNN_SCRATCH_CAPTURED.append(sc)
    d.n, d.k = n, k
    d.temperature, d.lmbda = temperature, lmbda
    d.out_logp, d.out_pknn, d.out_recall = out.data_ptr(), pk.data_ptr(), rec.data_ptr()
    call_desc("gnnlm_knn_interp", d)
    return out, pk, rec


def grid_points(ks, temperatures, lmbdas, alphas=None):
    """The points of a sweep in the one order every layer uses: k slowest, then temperature, lmbda fastest
    (row g of ``knn_interp_grid``'s result, ``gnnlm_knn_interp_grid_t``).  With ``alphas`` (the ``orig_prob_ratio`` axis) the points
    are ``(alpha, k, temperature, lmbda)`` and alpha is slowest of all (``gnnlm_knn_interp_grid_lm``); a sweep of alphas alone
    (``ks`` None: no kNN term) has the points ``(alpha,)``."""
    if alphas is None:
        return [(int(k), float(t), float(l)) for k in ks for t in temperatures for l in lmbdas]
    if ks is None:
        return [(float(a),) for a in alphas]
    return [(float(a), int(k), float(t), float(l)) for a in alphas for k in ks for t in temperatures for l in lmbdas]


def logp_mix(gnn_logp, base_logp, alphas, out=None):
    """The ``orig_prob_ratio`` mixture of two target log-probabilities (``gnnlm_logp_mix``; transformer.py:1056-1062,1075-1077):
    ``out[a] = logsumexp(log(alphas[a]) + base_logp, log(1 - alphas[a]) + gnn_logp)`` -> [len(alphas), n] f32 from one read of the
    two inputs.  1 .. 8 ratios, each in 0 .. 1; 0 gives ``gnn_logp`` back bit for bit and 1 ``base_logp``."""
    _dev(gnn_logp, base_logp, out)
    _f32(gnn_logp, base_logp, out)
    alphas = [float(a) for a in alphas]
    if gnn_logp.dim() != 1 or gnn_logp.shape != base_logp.shape or not (gnn_logp.is_contiguous() and base_logp.is_contiguous()):
        raise ValueError("logp_mix: gnn_logp, base_logp [n] contiguous")
    n = gnn_logp.shape[0]
    if out is None:
        out = torch.empty(len(alphas), n, device=gnn_logp.device, dtype=torch.float32)
    elif out.shape != (len(alphas), n) or not out.is_contiguous():
        raise ValueError("logp_mix: out [len(alphas), n] contiguous")
    # the count goes in as given: more ratios than the kernel takes are refused by the library, never cut short
    call("gnnlm_logp_mix", ptr(gnn_logp), ptr(base_logp), n, (ctypes.c_double * max(1, len(alphas)))(*alphas), len(alphas), ptr(out), stream())
    return out


def knn_interp_grid(lm_logp, sims, ids, targets, ks, temperatures, lmbdas, vals=None, n_store=None, row0=0, knn_vals=None):
    """Every point of ``ks x temperatures x lmbdas`` from one read of the search result (``gnnlm_knn_interp_grid``):
    -> (logp [G, n] f32 in :func:`grid_points` order, p_knn [len(ks) * len(temperatures), n] f32, recall [len(ks), n] i64).
    A point with 0 < lmbda < 1 equals ``knn_interp`` on the first k' columns bit for bit; lmbda 0 / 1 are allowed.  The label
    table is read by the plain gather (no tag table, no routed look-ups); k <= 1024.

    A 2-D ``lm_logp`` [A, n] (1 <= A <= 8 language-model rows: the ``orig_prob_ratio`` axis) goes through
    ``gnnlm_knn_interp_grid_lm``: logp is then [A * G, n] with the lm row slowest, and row block a equals the 1-D call with
    ``lm_logp[a]`` bit for bit; p_knn and recall do not depend on the lm row."""
    _dev(lm_logp, sims, ids, targets, vals, knn_vals)
    _f32(lm_logp, sims)
    _dtype(ids, torch.int64, "ids"), _dtype(targets, torch.int64, "targets"), _dtype(knn_vals, torch.int32, "knn_vals")
    if vals is not None and vals.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"vals: expected int16 / int32, got {vals.dtype}")
    for t in (lm_logp, sims, ids, targets, vals, knn_vals):
        if t is not None and not t.is_contiguous():
            raise _lib.GnnlmError("knn_interp_grid needs contiguous tensors")
    ks, temperatures, lmbdas = [int(v) for v in ks], [float(v) for v in temperatures], [float(v) for v in lmbdas]
    n, k = sims.shape
    if lm_logp.dim() not in (1, 2) or lm_logp.shape[-1] != n:
        raise ValueError("knn_interp_grid: lm_logp [n] or [A, n]")
    n_lm = lm_logp.shape[0] if lm_logp.dim() == 2 else None
    dev = sims.device
    d = _lib.gnnlm_knn_interp_grid_t()
    d.lm_logp, d.sims, d.ids, d.targets = lm_logp.data_ptr(), sims.data_ptr(), ids.data_ptr(), targets.data_ptr()
    d.vals_itemsize = 4
    if vals is not None:
        d.vals, d.vals_itemsize = vals.data_ptr(), vals.element_size()
        d.n_local = vals.shape[0]
        d.n_store = n_store if n_store is not None else vals.shape[0]
        d.row0 = row0
    if knn_vals is not None:
        d.knn_vals = knn_vals.data_ptr()
    d.n, d.k = n, k
    # the counts go in as given: a list longer than the descriptor's array is refused by the library, never cut short
    d.n_ks, d.n_temperatures, d.n_lmbdas = len(ks), len(temperatures), len(lmbdas)
    for dst, src in ((d.ks, ks), (d.temperatures, temperatures), (d.lmbdas, lmbdas)):
        for j, v in enumerate(src[:len(dst)]):
            dst[j] = v
    G = len(ks) * len(temperatures) * len(lmbdas)
    out = torch.empty((n_lm or 1) * G, n, device=dev, dtype=torch.float32)
    pk = torch.empty(len(ks) * len(temperatures), n, device=dev, dtype=torch.float32)
    rec = torch.empty(len(ks), n, device=dev, dtype=torch.int64)
    d.out_logp, d.out_pknn, d.out_recall = out.data_ptr(), pk.data_ptr(), rec.data_ptr()
    if n_lm is None:
        call_desc("gnnlm_knn_interp_grid", d)
    else:
        call("gnnlm_knn_interp_grid_lm", ctypes.byref(d), n_lm, n, stream())
    return out, pk, rec


def _rows_out(out, n, V, dev, what):
    """The [n, V] float32 result of a dense call: ``out`` as given (rows may be wider than V: its pad columns are left alone) or new."""
    if out is None:
        return torch.empty(n, V, device=dev, dtype=torch.float32)
    _f32(out)
    if not out.is_cuda or out.dim() != 2 or out.shape != (n, V) or (out.stride(1) != 1 and V > 1) or (n > 1 and out.stride(0) < V):
        raise ValueError(f"{what}: out must be a device tensor [n, V] with unit column stride and row stride >= V")
    return out


def _row_stride(t):
    """Row stride in elements of a [n, V] tensor with contiguous rows (a single row may carry any stride: V then)."""
    if t.dim() != 2 or (t.stride(1) != 1 and t.shape[1] > 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError("expected a 2-D tensor with contiguous rows and row stride >= its width")
    return max(t.stride(0), t.shape[1])


def _head_log_probs(entry, w, V, x, out, workspace, least_workspace):
    _f32(x)
    if not x.is_cuda:
        raise _lib.GnnlmError("gnnlm_amd kernels need device (HIP) tensors; there is no CPU fallback")
    if x.dim() != 2 or x.shape[1] != w.d:
        raise ValueError(f"{entry}: x [n, {w.d}]")
    if x.stride(-1) != 1 or x.stride(0) % 4 or x.stride(0) < w.d or x.data_ptr() % 16:
        x = x.contiguous()
    n = x.shape[0]
    out = _rows_out(out, n, V, x.device, entry)
    if n == 0:
        return out
    L = _lib.lib()
    need = getattr(L, f"gnnlm_{entry}_workspace_bytes" + ("_min" if least_workspace else ""))(ctypes.byref(w), n)
    if workspace is None or workspace.numel() < need:
        workspace = torch.empty(need, device=x.device, dtype=torch.uint8)
    _lib.check(getattr(L, "gnnlm_" + entry)(ctypes.byref(w), ctypes.c_void_p(x.data_ptr()), x.stride(0), n, ctypes.c_void_p(out.data_ptr()),
                                            _row_stride(out), ptr(workspace), need if least_workspace else workspace.numel(), stream()),
               "gnnlm_" + entry)
    return out


def adaptive_log_probs(w, x, out=None, workspace=None, least_workspace=False):
    """Full log-probabilities of the tied adaptive softmax (``gnnlm_adaptive_log_probs``; AdaptiveSoftmax.get_log_prob without a
    target, adaptive_softmax.py:170-206): ``w`` a filled ``gnnlm_adaptive_softmax_t``, ``x`` [n, d] f32 -> [n, V] f32.  ``out`` may be
    a view with a wider row stride (its pad columns stay untouched); ``workspace`` a uint8 device buffer that is used if it is
    large enough; ``least_workspace`` hands the library the least it accepts (128-row chunks: tests)."""
    return _head_log_probs("adaptive_log_probs", w, w.cutoff[w.n_bands - 1], x, out, workspace, least_workspace)


def dense_log_probs(w, x, out=None, workspace=None, least_workspace=False):
    """The same for the plain head (``gnnlm_dense_log_probs``): ``w`` a filled ``gnnlm_dense_softmax_t`` -> [n, vocab] f32."""
    return _head_log_probs("dense_log_probs", w, w.vocab, x, out, workspace, least_workspace)


def knn_mix_dense(lm_logp, sims, ids, temperature, lmbda, vals=None, n_store=None, row0=0, knn_vals=None, out=None, want_pknn=False):
    """The kNN distribution of every row interpolated with a whole row of language-model log-probabilities
    (``gnnlm_knn_mix_dense``): ``lm_logp`` [n, V] f32 (row stride >= V), ``sims`` [n, k] f32, ``ids`` [n, k] i64, labels as in
    :func:`knn_interp` -> ``out`` [n, V] f32, or ``(out, p_knn [n, V])`` with ``want_pknn``.  ``out[r, t]`` is what ``knn_interp`` gives
    for target ``t``.  Deterministic (no atomics); k <= 1024; ``out`` must not overlap ``lm_logp``."""
    _dev(lm_logp, sims, ids, vals, knn_vals)
    _f32(lm_logp, sims)
    _dtype(ids, torch.int64, "ids"), _dtype(knn_vals, torch.int32, "knn_vals")
    if vals is not None and vals.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"vals: expected int16 / int32, got {vals.dtype}")
    for t in (sims, ids, vals, knn_vals):
        if t is not None and not t.is_contiguous():
            raise _lib.GnnlmError("knn_mix_dense needs contiguous sims / ids / labels")
    if lm_logp.dim() != 2 or sims.dim() != 2 or sims.shape != ids.shape or sims.shape[0] != lm_logp.shape[0]:
        raise ValueError("knn_mix_dense: lm_logp [n, V], sims / ids [n, k]")
    n, V = lm_logp.shape
    k = sims.shape[1]
    out = _rows_out(out, n, V, lm_logp.device, "knn_mix_dense")
    pk = torch.empty(n, V, device=lm_logp.device, dtype=torch.float32) if want_pknn else None
    d = _lib.gnnlm_knn_mix_dense_t()
    d.lm_logp, d.ld_lm = lm_logp.data_ptr(), _row_stride(lm_logp)
    d.sims, d.ids = sims.data_ptr(), ids.data_ptr()
    d.vals_itemsize = 4
    if vals is not None:
        d.vals, d.vals_itemsize = vals.data_ptr(), vals.element_size()
        d.n_local = vals.shape[0]
        d.n_store = n_store if n_store is not None else vals.shape[0]
        d.row0 = row0
    if knn_vals is not None:
        d.knn_vals = knn_vals.data_ptr()
    d.n, d.k, d.V = n, k, V
    d.temperature, d.lmbda = temperature, lmbda
    d.out, d.ldo = out.data_ptr(), _row_stride(out)
    if pk is not None:
        d.out_pknn, d.ld_pknn = pk.data_ptr(), V
    call_desc("gnnlm_knn_mix_dense", d)
    return (out, pk) if want_pknn else out


def row_rank(logp, target, out=None):
    """``rank[r]`` = the number of columns of ``logp[r]`` in front of column ``target[r]`` in ``topk_merge``'s order (larger value
    first, then smaller id); -1 for a target outside [0, V) (``gnnlm_row_rank``).  logp [n, V] f32, target [n] i64 -> int32 [n]."""
    _dev(logp, target, out)
    _f32(logp)
    _dtype(target, torch.int64, "target"), _dtype(out, torch.int32, "out")
    if logp.dim() != 2 or target.shape != (logp.shape[0],) or not target.is_contiguous():
        raise ValueError("row_rank: logp [n, V], target [n] contiguous")
    n, V = logp.shape
    if out is None:
        out = torch.empty(n, device=logp.device, dtype=torch.int32)
    elif out.shape != (n,) or not out.is_contiguous():
        raise ValueError("row_rank: out [n] contiguous")
    call("gnnlm_row_rank", ptr_strided(logp), _row_stride(logp), n, V, ptr(target), ptr(out), stream())
    return out


def knn_recompute_sims(queries, ids, keys, metric, normalize_keys=False, out=None):
    """Similarities recomputed from the stored keys (``gnnlm_knn_recompute_sims``; knn_model.py:161-175) -> ``out`` [n, k] f32.

    ``queries`` [n, d] f32 (already normalised for a cosine index); ``keys`` [n_rows, d] fp16 / f32; ``ids`` [n, k] int64, or
    None for direct mode, where neighbour (i, j) is row ``i * k + j`` of ``keys`` (``keys`` is then [n * k, d] or [n, k, d]).
    ``metric``: "ip" / 0 = key . q, "l2" / 1 = -|q - key|^2; ``normalize_keys`` divides an ip result by |key|.  Row strides
    wider than the rows are taken as they are (no copy).  An id < 0 reads row id + n_rows, an id out of range gives -FLT_MAX.
    A result depends on its query row and its key row only."""
    _dev(queries, ids, out)
    if not keys.is_cuda:
        raise _lib.GnnlmError("gnnlm_amd kernels need contiguous device (HIP) tensors; there is no CPU fallback")
    _f32(queries, out)
    _dtype(ids, torch.int64, "ids")
    if keys.dtype not in (torch.float16, torch.float32):
        raise TypeError(f"keys: expected float16 / float32, got {keys.dtype}")
    metric = {"ip": 0, "l2": 1}.get(metric, metric)
    if queries.dim() != 2:
        raise ValueError("knn_recompute_sims: queries [n, d]")
    n, d = queries.shape
    if ids is None:
        if keys.dim() == 3:
            if keys.shape[0] != n or not keys.is_contiguous():
                raise ValueError("knn_recompute_sims: direct mode takes keys [n, k, d] contiguous or [n * k, d]")
            k = keys.shape[1]
            keys = keys.view(n * k, keys.shape[2])
        else:
            k = keys.shape[0] // n if n else 1
            if keys.dim() != 2 or k < 1 or keys.shape[0] != n * k:
                raise ValueError("knn_recompute_sims: direct mode takes keys [n, k, d] contiguous or [n * k, d]")
    else:
        if ids.dim() != 2 or ids.shape[0] != n:
            raise ValueError("knn_recompute_sims: ids [n, k]")
        k = ids.shape[1]
    if keys.dim() != 2 or keys.shape[1] != d or (keys.shape[0] > 1 and keys.stride(1) != 1):
        raise ValueError("knn_recompute_sims: keys [n_rows, d] with unit element stride")
    if out is None:
        out = torch.empty(n, k, device=queries.device, dtype=torch.float32)
    elif out.shape != (n, k):
        raise ValueError("knn_recompute_sims: out [n, k]")
    r = _lib.gnnlm_knn_resim_t()
    r.queries, r.ldq = queries.data_ptr(), max(queries.stride(0), d)
    if ids is not None:
        r.ids, r.ld_ids = ids.data_ptr(), max(ids.stride(0), k)
    r.keys, r.keys_itemsize = keys.data_ptr(), keys.element_size()
    r.ld_keys, r.n_rows = max(keys.stride(0), d), keys.shape[0]
    r.d, r.n, r.k = d, n, k
    r.metric, r.normalize_keys = metric, int(bool(normalize_keys))
    r.out, r.ld_out = out.data_ptr(), max(out.stride(0), k)
    call_desc("gnnlm_knn_recompute_sims", r)
    return out


def topk_merge(scores, best_val, best_id, col0=0, col_ids=None, col_scale=None, col_bias=None, alpha=1.0, largest=True,
               init=False, row_ncols=None, ids=None):
    """Fold the score chunk ``scores`` [n, ncols] into the running top-k state (``best_val`` f32 / ``best_id`` i64
    [n, k], best first): value of column c = col_bias[c] + alpha * col_scale[c] * scores[:, c], id = col_ids[c] or
    col0 + c.  In place; ``init=True`` treats the state as empty (first chunk)."""
    _dev(scores, best_val, best_id, col_ids, col_scale, col_bias, row_ncols)
    _f32(scores, best_val, col_scale, col_bias)
    _dtype(best_id, torch.int64, "best_id"), _dtype(col_ids, torch.int64, "col_ids"), _dtype(row_ncols, torch.int32, "row_ncols")
    n, ncols = scores.shape
    assert best_val.shape == best_id.shape and best_val.shape[0] == n and best_val.is_contiguous() and best_id.is_contiguous()
    d = _lib.gnnlm_topk_t()
    d.scores, d.ld, d.n, d.ncols = scores.data_ptr(), scores.stride(0), n, ncols
    d.col0 = col0
    if col_ids is not None:
        d.col_ids = col_ids.data_ptr()
    if col_scale is not None:
        d.col_scale = col_scale.data_ptr()
    if col_bias is not None:
        d.col_bias = col_bias.data_ptr()
    if row_ncols is not None:
        d.row_ncols = row_ncols.data_ptr()
    if ids is not None:                                  # per-row ids [n, ncols]
        _dev(ids)
        _dtype(ids, torch.int64, "ids")
        assert ids.shape == scores.shape
        d.ids, d.ld_ids = ids.data_ptr(), ids.stride(0)
    d.alpha, d.k, d.largest, d.init = alpha, best_val.shape[1], int(largest), int(init)
    d.best_val, d.best_id = best_val.data_ptr(), best_id.data_ptr()
    call_desc("gnnlm_topk_merge", d)
    return best_val, best_id


def ivfpq_pack_tiles(codes):
    """codes [N, 64] u8 -> the int8-MFMA scan's image (csrc/ivfpq8_prep.hip): ceil(N / 16) tiles x [4 groups][16 rows][16 bytes],
    byte p of (tile t, group g, row i) = codes[16 t + i][16 g + (i + p) % 16]; rows beyond N are zero."""
    _dev(codes)
    _dtype(codes, torch.uint8, "codes")
    N, M = codes.shape
    out = torch.empty(-(-N // 16) * 16 * M, dtype=torch.uint8, device=codes.device)
    call("gnnlm_ivfpq_pack_tiles", ptr(codes), N, M, ptr(out), stream())
    return out


def ivfpq_key_terms(list_codes, list_off, coarse, pq):
    """The L2 scan's term of every key (gnnlm_ivfpq_key_terms): list_codes [N, M] u8 in list order, list_off [nlist + 1] i64,
    coarse [nlist, M * dsub] f32, pq [M, 256, dsub] f32 -> key_term [N] f32 = sum_m (|p_m,c|^2 + 2 <c_l,m, p_m,c>) of the row's
    codes c and list l, accumulated in float64."""
    for t in (list_codes, list_off, coarse, pq):
        _dev(t)
    _dtype(list_codes, torch.uint8, "list_codes")
    _dtype(list_off, torch.int64, "list_off")
    _dtype(coarse, torch.float32, "coarse")
    _dtype(pq, torch.float32, "pq")
    N, M = list_codes.shape
    nlist, dsub = coarse.shape[0], pq.shape[2]
    if list_off.numel() != nlist + 1 or pq.shape[0] != M or pq.shape[1] != 256 or coarse.shape[1] != M * dsub:
        raise ValueError("ivfpq_key_terms: list_off [nlist + 1], coarse [nlist, M * dsub], pq [M, 256, dsub]")
    out = torch.empty(N, dtype=torch.float32, device=list_codes.device)
    call("gnnlm_ivfpq_key_terms", ptr(list_codes), ptr(list_off), N, nlist, ptr(coarse), ptr(pq), M, dsub, ptr(out), stream())
    return out


def ivfpq_select_probes(cs, pv, pi, col_bias=None, select=True):
    """The pv.shape[1] best columns of every row of cs [n, ncols] (+ col_bias), best first, into pv / pi: gnnlm_ivfpq_select_probes
    (csrc/ivfpq_select.hip); shapes it does not take (and select=False) go to gnnlm_topk_merge, which returns the same bits.  The
    search picks its probes with it and the add path files a key with it at one probe: the list the search ranks first."""
    if not select or cs.shape[1] > 4096 or pv.shape[1] > 64:
        return topk_merge(cs, pv, pi, largest=True, init=True, col_bias=col_bias)
    d = _lib.gnnlm_ivfpq_select_probes_t()
    d.scores, d.ld, d.n, d.ncols = cs.data_ptr(), cs.stride(0), cs.shape[0], cs.shape[1]
    if col_bias is not None:
        d.col_bias = col_bias.data_ptr()
    d.k, d.largest, d.out_val, d.out_id = pv.shape[1], 1, pv.data_ptr(), pi.data_ptr()
    call_desc("gnnlm_ivfpq_select_probes", d)


def ivfpq_coarse_slabs(n, nlist, k):
    """Slabs the lists are cut into for ``ivfpq_coarse_probes`` (pure numbers): enough workgroups (64 rows x one slab each) for four
    per compute unit, slabs no narrower than 4096 lists (a slab's first chunks compact their rows every time), slabs * k columns at
    most 4096 for the merge."""
    tiles = max(1, -(-int(n) // 64))
    return max(1, min(-(-1024 // tiles), int(nlist) // 4096, 4096 // max(int(k), 1), 64))


def ivfpq_coarse_probes(x, coarse, pv, pi, col_bias=None, slabs=None):
    """The pv.shape[1] <= 64 best rows of coarse [nlist, d] for every row of x [n, d] (row stride free) by <x, c> (+ col_bias),
    best first, into pv [n, P] f32 / pi [n, P] i64: ``ivfpq_select_probes`` over ``gemm_nt(x, coarse)`` without the [n, nlist]
    matrix (gnnlm_ivfpq_coarse_probes, csrc/ivfpq_coarse.hip).  ``slabs``: runs the lists are cut into (default
    ``ivfpq_coarse_slabs``); beyond one, the slabs' lists go through an [n, slabs, P] partial and gnnlm_topk_merge."""
    _dev(x, coarse, pv, pi, col_bias)
    _f32(x, coarse, pv, col_bias)
    _dtype(pi, torch.int64, "pi")
    if x.dim() != 2 or coarse.dim() != 2 or not coarse.is_contiguous() or coarse.shape[1] != x.shape[1] or x.stride(1) != 1:
        raise ValueError("ivfpq_coarse_probes: x [n, d] with unit column stride, coarse [nlist, d] contiguous")
    (n, d), nlist, P = x.shape, coarse.shape[0], pv.shape[1] if pv.dim() == 2 else -1
    if pv.shape != (n, P) or pi.shape != (n, P) or not (pv.is_contiguous() and pi.is_contiguous()):
        raise ValueError("ivfpq_coarse_probes: pv / pi [n, P] contiguous")
    if col_bias is not None and (col_bias.shape != (nlist,) or not col_bias.is_contiguous()):
        raise ValueError("ivfpq_coarse_probes: col_bias [nlist] contiguous")
    c = _lib.gnnlm_ivfpq_coarse_t()
    c.x, c.ldx, c.n = x.data_ptr(), max(x.stride(0), d), n
    c.coarse, c.nlist, c.d = coarse.data_ptr(), nlist, d
    if col_bias is not None:
        c.col_bias = col_bias.data_ptr()
    c.k = P
    c.slabs = ivfpq_coarse_slabs(n, nlist, P) if slabs is None else int(slabs)
    if c.slabs > 1:
        part_val = torch.empty(n, c.slabs, P, dtype=torch.float32, device=x.device)
        part_id = torch.empty(n, c.slabs, P, dtype=torch.int64, device=x.device)
        c.part_val, c.part_id = part_val.data_ptr(), part_id.data_ptr()
    c.out_val, c.out_id = pv.data_ptr(), pi.data_ptr()
    call_desc("gnnlm_ivfpq_coarse_probes", c)


def ivfpq_encode_rows(x, assign, coarse, pq, norm2=None, out=None, list_cnt=None, n_bad=None):
    """The residual PQ codes of assigned rows (gnnlm_ivfpq_encode_rows): x [n, d] f32 rotated rows (row stride free), assign [n]
    i64 the list of each row, coarse [nlist, d], pq [M, 256, dsub], norm2 [M, 256] = |p_mc|^2 (computed if None) -> codes [n, M] u8
    (``out``: a buffer or a row slice of one).  list_cnt [nlist] i64 is incremented per encoded row, n_bad [1] i32 per row whose
    list does not exist (its codes are left alone)."""
    _dev(x, assign, coarse, pq, norm2, out, list_cnt, n_bad)
    _f32(x, coarse, pq, norm2)
    _dtype(assign, torch.int64, "assign"), _dtype(out, torch.uint8, "out")
    _dtype(list_cnt, torch.int64, "list_cnt"), _dtype(n_bad, torch.int32, "n_bad")
    if x.dim() != 2 or pq.dim() != 3 or pq.shape[1] != 256 or coarse.dim() != 2 or not (coarse.is_contiguous() and pq.is_contiguous()):
        raise ValueError("ivfpq_encode_rows: x [n, d], coarse [nlist, d] and pq [M, 256, dsub] contiguous")
    (n, d), (M, _, dsub), nlist = x.shape, pq.shape, coarse.shape[0]
    if coarse.shape[1] != d or assign.shape != (n,) or (list_cnt is not None and list_cnt.shape != (nlist,)):
        raise ValueError("ivfpq_encode_rows: coarse [nlist, d], assign [n], list_cnt [nlist]")
    if norm2 is None:
        norm2 = (pq ** 2).sum(2).contiguous()
    if norm2.shape != (M, 256) or not norm2.is_contiguous():
        raise ValueError("ivfpq_encode_rows: norm2 [M, 256] contiguous")
    if out is None:
        out = torch.empty(n, M, dtype=torch.uint8, device=x.device)
    elif out.shape != (n, M):
        raise ValueError("ivfpq_encode_rows: out [n, M]")
    e = _lib.gnnlm_ivfpq_encode_t()
    e.x, e.ldx, e.n, e.assign = x.data_ptr(), max(x.stride(0), d), n, assign.data_ptr()
    e.coarse, e.nlist, e.pq, e.norm2 = coarse.data_ptr(), nlist, pq.data_ptr(), norm2.data_ptr()
    e.M, e.dsub, e.d = M, dsub, d
    e.codes, e.ld_codes = out.data_ptr(), max(out.stride(0), M)
    if list_cnt is not None:
        e.list_cnt = list_cnt.data_ptr()
    if n_bad is not None:
        e.n_bad = n_bad.data_ptr()
    call_desc("gnnlm_ivfpq_encode_rows", e)
    return out


def ivfpq_list_place(assign, list_off_old):
    """Where new rows go: assign [n] i64 (the list of each new row, every one in [0, nlist)), list_off_old [nlist + 1] i64 ->
    (new_off [nlist + 1], dest [n]): new_off the cumulative sum of old length + new count per list; the new rows of a list keep
    the order given (a stable sort of assign) behind its old rows, dest = new_off[l] + old_len[l] + rank."""
    _dev(assign, list_off_old)
    _dtype(assign, torch.int64, "assign"), _dtype(list_off_old, torch.int64, "list_off_old")
    nlist, n = list_off_old.numel() - 1, assign.numel()
    old_len = list_off_old[1:] - list_off_old[:-1]
    cnt = torch.bincount(assign, minlength=nlist) if n else torch.zeros_like(old_len)
    if cnt.numel() != nlist:
        raise ValueError("ivfpq_list_place: assign outside [0, nlist)")
    new_off = torch.zeros(nlist + 1, dtype=torch.int64, device=assign.device)
    new_off[1:] = torch.cumsum(old_len + cnt, 0)
    order = torch.sort(assign, stable=True).indices
    start = torch.cumsum(cnt, 0) - cnt                                   # first sorted position of every list's new rows
    srt = assign[order]
    dest = torch.empty(n, dtype=torch.int64, device=assign.device)
    dest[order] = new_off[:-1][srt] + old_len[srt] + (torch.arange(n, device=assign.device) - start[srt])
    return new_off, dest


def ivfpq_list_merge(list_off_old, ids_old, codes_old, dest, ids_new, codes_new, new_off, n_bad=None):
    """Old rows and new rows into the merged list-ordered arrays (gnnlm_ivfpq_list_merge): a list's old rows move as one run to
    new_off[l], new row i goes to dest[i] (``ivfpq_list_place``).  -> (ids [N0 + n] i64, codes [N0 + n, M] u8), new buffers."""
    _dev(list_off_old, ids_old, codes_old, dest, ids_new, codes_new, new_off, n_bad)
    for t, what in ((list_off_old, "list_off_old"), (ids_old, "ids_old"), (dest, "dest"), (ids_new, "ids_new"), (new_off, "new_off")):
        _dtype(t, torch.int64, what)
    _dtype(codes_old, torch.uint8, "codes_old"), _dtype(codes_new, torch.uint8, "codes_new"), _dtype(n_bad, torch.int32, "n_bad")
    N0, n, nlist = ids_old.numel(), ids_new.numel(), new_off.numel() - 1
    M = codes_new.shape[1] if codes_new.dim() == 2 else -1
    if (codes_old.shape != (N0, M) or codes_new.shape[0] != n or dest.shape != (n,) or list_off_old.numel() != nlist + 1
            or not codes_old.is_contiguous()):
        raise ValueError("ivfpq_list_merge: ids_old [N0], codes_old [N0, M] contiguous, dest / ids_new [n], codes_new [n, M], offsets [nlist + 1]")
    ids = torch.empty(N0 + n, dtype=torch.int64, device=new_off.device)
    codes = torch.empty(N0 + n, M, dtype=torch.uint8, device=new_off.device)
    m = _lib.gnnlm_ivfpq_list_merge_t()
    m.list_off_old, m.nlist, m.N0 = list_off_old.data_ptr(), nlist, N0
    m.ids_old, m.codes_old, m.M = ids_old.data_ptr(), codes_old.data_ptr(), M
    m.n, m.dest, m.ids_new, m.codes_new, m.ld_new = n, dest.data_ptr(), ids_new.data_ptr(), codes_new.data_ptr(), max(codes_new.stride(0), M)
    m.new_off, m.ids, m.codes = new_off.data_ptr(), ids.data_ptr(), codes.data_ptr()
    if n_bad is not None:
        m.n_bad = n_bad.data_ptr()
    call_desc("gnnlm_ivfpq_list_merge", m)
    return ids, codes


def ivfpq_keep_flags(list_ids, list_off, ranges):
    """Which rows of an index survive the removal of id ranges (gnnlm_ivfpq_keep_flags): list_ids [N] i64, list_off [nlist + 1] i64,
    ranges [n, 2] i64 half-open [lo, hi), sorted by lo and pairwise disjoint (``ivfpq_train.normalize_ranges``), all on the device
    -> (keep [N] u8: 1 survives, list_keep [nlist] i64: survivors per list)."""
    _dev(list_ids, list_off, ranges)
    for t, what in ((list_ids, "list_ids"), (list_off, "list_off"), (ranges, "ranges")):
        _dtype(t, torch.int64, what)
    N, nlist = list_ids.numel(), list_off.numel() - 1
    if (list_ids.dim() != 1 or list_off.dim() != 1 or nlist < 0 or ranges.dim() != 2 or ranges.shape[1] != 2
            or not (list_ids.is_contiguous() and list_off.is_contiguous() and ranges.is_contiguous())):
        raise ValueError("ivfpq_keep_flags: list_ids [N], list_off [nlist + 1], ranges [n, 2], contiguous")
    keep = torch.empty(N, dtype=torch.uint8, device=list_ids.device)
    list_keep = torch.empty(nlist, dtype=torch.int64, device=list_ids.device)
    f = _lib.gnnlm_ivfpq_keep_flags_t()
    f.ids, f.N, f.list_off, f.nlist = list_ids.data_ptr(), N, list_off.data_ptr(), nlist
    f.ranges, f.n_ranges = ranges.data_ptr() if ranges.shape[0] else None, ranges.shape[0]
    f.keep, f.list_keep = keep.data_ptr(), list_keep.data_ptr()
    call_desc("gnnlm_ivfpq_keep_flags", f)
    return keep, list_keep


def ivfpq_list_compact(list_off_old, ids_old, codes_old, keep, new_off, n_bad=None):
    """The rows with keep != 0 of the list-ordered arrays, list by list in their order (gnnlm_ivfpq_list_compact): new_off
    [nlist + 1] is the cumulative sum of ``ivfpq_keep_flags``'s list_keep.  -> (ids [n] i64, codes [n, M] u8), new buffers of
    n = new_off[-1] rows (one read of that number).  n_bad [1] i32 is incremented per list whose survivors are not
    new_off[l + 1] - new_off[l]."""
    _dev(list_off_old, ids_old, codes_old, keep, new_off, n_bad)
    for t, what in ((list_off_old, "list_off_old"), (ids_old, "ids_old"), (new_off, "new_off")):
        _dtype(t, torch.int64, what)
    _dtype(codes_old, torch.uint8, "codes_old"), _dtype(keep, torch.uint8, "keep"), _dtype(n_bad, torch.int32, "n_bad")
    N0, nlist = ids_old.numel(), new_off.numel() - 1
    M = codes_old.shape[1] if codes_old.dim() == 2 else -1
    if (ids_old.dim() != 1 or codes_old.shape != (N0, M) or keep.shape != (N0,) or nlist < 0 or list_off_old.shape != (nlist + 1,)
            or new_off.dim() != 1 or not (codes_old.is_contiguous() and ids_old.is_contiguous() and keep.is_contiguous()
                                          and list_off_old.is_contiguous() and new_off.is_contiguous())):
        raise ValueError("ivfpq_list_compact: ids_old / keep [N0], codes_old [N0, M], offsets [nlist + 1], contiguous")
    n = int(new_off[-1].item()) if N0 and nlist > 0 else 0
    if n < 0 or n > N0:
        raise ValueError(f"ivfpq_list_compact: new_off ends at {n}, the index has {N0} rows")
    ids = torch.empty(n, dtype=torch.int64, device=new_off.device)
    codes = torch.empty(n, M, dtype=torch.uint8, device=new_off.device)
    ws_bytes = _lib.lib().gnnlm_ivfpq_list_compact_workspace_bytes(N0, nlist)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=new_off.device)
    out_ids = ids if n else torch.empty(1, dtype=torch.int64, device=new_off.device)         # (never written: the entry wants pointers)
    out_codes = codes if n else torch.empty(1, max(M, 16), dtype=torch.uint8, device=new_off.device)
    c = _lib.gnnlm_ivfpq_list_compact_t()
    c.list_off_old, c.nlist, c.N0 = list_off_old.data_ptr(), nlist, N0
    c.ids_old, c.codes_old, c.M, c.keep = ids_old.data_ptr(), codes_old.data_ptr(), M, keep.data_ptr()
    c.new_off, c.ids, c.codes = new_off.data_ptr(), out_ids.data_ptr(), out_codes.data_ptr()
    if n_bad is not None:
        c.n_bad = n_bad.data_ptr()
    c.workspace, c.workspace_bytes = ws.data_ptr(), ws_bytes
    call_desc("gnnlm_ivfpq_list_compact", c)
    return ids, codes


def ivfpq_quantize_lut(lut, M=64):
    """lut [n, M * 256] f32 -> (qlut [n, 2, 256, 32] u8, qmeta [n, 4] f32 = {delta, sum_m lo_m, max |lut|, 0}) with
    lut[m][c] < lo_m + (u + 1) * delta for every entry, u = qlut[m // 32][c][m % 32] ^ 0x80 (the table stores the signed
    byte u - 128, what the i8 matrix instruction reads) -- the filter's one-sided bound."""
    _dev(lut)
    _f32(lut)
    n = lut.shape[0]
    qlut = torch.empty(n, 2, 256, 32, dtype=torch.uint8, device=lut.device)
    qmeta = torch.empty(n, 4, dtype=torch.float32, device=lut.device)
    call("gnnlm_ivfpq_quantize_lut", ptr(lut), lut.stride(0), n, M, ptr(qlut), ptr(qmeta), stream())
    return qlut, qmeta


def masked_sum_f64(x, mask=None, acc=None):
    if acc is None:
        acc = torch.zeros(1, device=x.device, dtype=torch.float64)
    call("gnnlm_masked_sum_f64", ptr(x), ptr(mask), x.numel(), ptr(acc), stream())
    return acc


def rows_sum_f64(x, out):
    """out[g] += sum(x[g, :]) in float64 for every row of ``x`` [G, n] in one launch (``gnnlm_rows_sum_f64``); row g is added
    up in ``masked_sum_f64``'s order."""
    _dev(x, out)
    _f32(x)
    _dtype(out, torch.float64, "out")
    if x.dim() != 2 or out.dim() != 1 or out.shape[0] != x.shape[0] or not out.is_contiguous():
        raise ValueError("rows_sum_f64: x [G, n] float32, out [G] float64")
    x = x.contiguous()
    call("gnnlm_rows_sum_f64", ptr(x), x.shape[1], x.shape[0], x.shape[1], ptr(out), stream())
    return out
