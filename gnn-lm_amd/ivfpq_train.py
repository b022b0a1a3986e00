"""The offline producer of an IVF-PQ index (``IVFPQIndex.build`` delegates here; the reference delegates it to faiss:
knn/index_builder.py:79-150): plain Lloyd k-means for the product quantizers, spherical k-means (unit-norm centroids, what faiss's
index_factory sets for inner-product indexes) for the coarse one, a random orthonormal matrix for R or OPQ rounds from it (faiss
alternates OPQ updates; any orthonormal R gives a valid index).  Training runs on the GPU with torch ops -- offline tooling, not the
hot path; ``quantize_features.py`` trains its feature quantizer with the same ``kmeans`` / ``train_opq``.  ADDING keys (``add_rows``:
to an empty index for a build, to an existing one to grow it) runs on this library's kernels: csrc/ivfpq_add.hip; REMOVING keys
(``remove_rows``) and merging two indexes (``merge_lists``) on csrc/ivfpq_remove.hip and the add path's merge."""
import os

import numpy as np
import torch

from . import ops


# List counts from which the coarse step runs WITHOUT its [rows, nlist] score matrix (``ops.ivfpq_coarse_probes``, csrc/ivfpq_coarse.hip):
# the search (``ivfpq.choose_coarse``), ``add_rows`` and the assignment step of ``kmeans``.  The smallest list count timed by
# tools/ivfpq_coarse_bench.py from which the fused step is no slower than GEMM + selection (profiles/r25_coarse_bench.txt, 8192 rows
# of 64 dimensions: 0.96x at 16,384 lists, 1.03x at 65,536, 2.7x at 1,048,576), never below 16384: every index of
# 8192 lists or fewer runs the launches it always ran.
COARSE_FUSED_MIN_LISTS = 65536


def coarse_fused(nlist, d, forced=None):
    """Does a coarse step over ``nlist`` centroids of ``d`` dimensions take the fused kernel?  ``forced``: "dense" / "fused" / None;
    the environment's GNNLM_IVF_COARSE stands in for None (A/B runs)."""
    env = os.environ.get("GNNLM_IVF_COARSE") or None
    if forced not in (None, "dense", "fused") or env not in (None, "dense", "fused"):
        raise ValueError(f"coarse step: 'dense' or 'fused', got {forced or env!r}")
    if forced is not None:
        return forced == "fused"                                            # (the kernel refuses d % 4 != 0 itself)
    return (env == "fused" or (env is None and nlist >= COARSE_FUSED_MIN_LISTS)) and d % 4 == 0


def kmeans(x, k, iters, gen, spherical=False, init=None, coarse=None):
    """Lloyd's algorithm (squared L2) on the device; empty clusters are re-seeded from random points.  ``spherical``: the
    centroids are L2-normalised after every update (faiss ClusteringParameters.spherical, set by index_factory for
    METRIC_INNER_PRODUCT coarse quantizers).  ``init``: centroids to start from (OPQ's inner PQ rounds).  From
    ``COARSE_FUSED_MIN_LISTS`` centroids on (``coarse``: "dense" / "fused" forces it) the assignment is the fused coarse step at one
    probe with the bias -|c|^2 / 2 -- no [rows, k] matrix; below, the torch expression."""
    fused = coarse_fused(k, x.shape[1], coarse)
    n = x.shape[0]
    if init is not None:
        cen = init.clone()
    else:
        cen = x[torch.randperm(n, generator=gen, device=x.device)[:k]].clone()
    if cen.shape[0] < k:
        cen = torch.cat([cen, cen[torch.randint(0, cen.shape[0], (k - cen.shape[0],), generator=gen, device=x.device)]])
    for _ in range(iters):
        assign = torch.empty(n, dtype=torch.int64, device=x.device)
        c2 = (cen ** 2).sum(1)
        if fused:                                                            # argmin |x - c|^2 = argmax <x, c> - |c|^2 / 2
            ops.ivfpq_coarse_probes(x, cen.contiguous(), torch.empty(n, 1, dtype=torch.float32, device=x.device), assign.view(n, 1),
                                    col_bias=(-0.5 * c2).contiguous())
            if bool((assign < 0).any()):
                raise ValueError("kmeans: rows without a nearest centroid (NaN rows?)")
        else:
            for s in range(0, n, 1 << 18):
                xs = x[s:s + (1 << 18)]
                assign[s:s + (1 << 18)] = (c2[None, :] - 2 * xs @ cen.t()).argmin(1)
        cnt = torch.bincount(assign, minlength=k)
        new = torch.zeros_like(cen).index_add_(0, assign, x)
        live = cnt > 0
        new[live] /= cnt[live, None].to(x.dtype)
        dead = (~live).nonzero().reshape(-1)
        if dead.numel():
            new[dead] = x[torch.randint(0, n, (dead.numel(),), generator=gen, device=x.device)]
        cen = new / new.norm(dim=1, keepdim=True).clamp_min(1e-20) if spherical else new
    return cen


def pq_assign(x, cen):
    """x [n, dsub], cen [256, dsub] -> nearest centroid per row (squared L2), in chunks."""
    out = torch.empty(x.shape[0], dtype=torch.int64, device=x.device)
    c2 = (cen ** 2).sum(1)
    for s in range(0, x.shape[0], 1 << 18):
        out[s:s + (1 << 18)] = (c2[None, :] - 2 * x[s:s + (1 << 18)] @ cen.t()).argmin(1)
    return out


def train_opq(x, M, R0, iters, gen, pq_iters=4):
    """The OPQ rotation (Ge et al., "Optimized Product Quantization", the non-parametric solution; what faiss's OPQMatrix trains
    for the ``OPQ64_1024`` block of the reference's index type, knn/index_builder.py:60-64): alternate (a) a product quantizer of
    M x 256 centroids on the rotated vectors x R^T (k-means per sub-space, warm-started from the previous round) and (b) the
    orthogonal Procrustes solution R^T = U V^T, U S V^T = x^T y, y = the quantizer's reconstruction of x R^T -- the rotation
    under which the quantizer loses least.  x [n, d] f32 on the device, R0 [d_out, d] with orthonormal rows; -> R [d_out, d]."""
    n, d = x.shape
    dsub = R0.shape[0] // M                                                   # R0 [d_out, d]: d_out < d for an `OPQ<M>_<d_out>` block that reduces
    R, cents = R0.clone(), [None] * M
    for _ in range(iters):
        xr = x @ R.t()
        y = torch.empty_like(xr)
        for m in range(M):
            sub = xr[:, m * dsub:(m + 1) * dsub].contiguous()
            cents[m] = kmeans(sub, 256, pq_iters, gen, init=cents[m])
            y[:, m * dsub:(m + 1) * dsub] = cents[m][pq_assign(sub, cents[m])]
        U, _, Vt = torch.linalg.svd((x.t() @ y).double(), full_matrices=False)
        R = (U @ Vt).t().to(torch.float32).contiguous()
    return R


def _initial_rotation(x, d_out, gen):
    """[d_out, d_in] with orthonormal rows: a random rotation (d_out == d_in) or a random rotation of the d_out leading
    principal directions (d_out < d_in: what an OPQ<M>_<d_out> block starts from)."""
    d_in = x.shape[1]
    cpu_gen = torch.Generator().manual_seed(int(gen.initial_seed()))
    Q = torch.linalg.qr(torch.randn(d_out, d_out, generator=cpu_gen, dtype=torch.float64))[0]
    if d_out == d_in:
        return Q.to(torch.float32).to(x.device)
    xc = x.double()
    _, V = torch.linalg.eigh(xc.t() @ xc)                                     # ascending eigenvalues
    P = V[:, -d_out:].t().cpu()                                               # [d_out, d_in] leading directions
    return (Q @ P).to(torch.float32).to(x.device)


def _rows(keys, lo, hi, device, cosine):
    """rows lo .. hi of a key table (numpy array / memmap / torch tensor, fp16 or f32) on the device in f32, normalised if cosine"""
    x = torch.from_numpy(np.ascontiguousarray(keys[lo:hi]).astype(np.float32)).to(device) if not isinstance(keys, torch.Tensor) \
        else keys[lo:hi].to(device, torch.float32)
    return x / (x ** 2).sum(1, keepdim=True).sqrt() if cosine else x


def rotated_rows(keys, lo, hi, R, cosine):
    """rows lo .. hi as the index sees them: normalised if cosine, rotated on ``gnnlm_gemm_nt`` (float32, on R's device)"""
    return ops.gemm_nt(_rows(keys, lo, hi, R.device, cosine), R)


def train(keys, nlist, M, device="cuda", cosine=True, iters=10, train_size=262144, seed=0, chunk=1 << 18, opq_iters=0, metric="ip",
          d_out=None):
    """Train (rotation, coarse centroids, residual product quantizer) on a sample of the keys.  ``opq_iters`` = 0: a random
    orthonormal rotation (spreads the variance over the sub-spaces); > 0: that many rounds of OPQ training from it (``train_opq``:
    what the reference's ``OPQ64_1024`` block asks faiss for).  ``d_out`` < d (the ``OPQ16_64`` block of the One Billion Word recipe,
    gnnlm_scripts/one_billion/find_knn.sh:8-21): R [d_out, d] with orthonormal rows, from the d_out leading principal directions of the
    sample, randomly rotated (``_initial_rotation``); centroids and sub-spaces live in d_out dimensions.  -> (R, coarse, pq); the
    reference's ``IndexBuilder.train`` (knn/index_builder.py:66-95)."""
    device = torch.device(device)
    gen = torch.Generator(device=device)
    gen.manual_seed(seed)
    N, d = keys.shape
    d_out = d if d_out is None else int(d_out)
    assert 0 < d_out <= d, "d_out lies in 1 .. d"
    assert d_out % M == 0 and (d_out // M) % 4 == 0 and M % 16 == 0, "need dsub % 4 == 0 and M % 16 == 0"
    dsub = d_out // M
    cpu_gen = torch.Generator().manual_seed(seed)
    R = torch.linalg.qr(torch.randn(d, d, generator=cpu_gen, dtype=torch.float64))[0].to(torch.float32).to(device)
    pick = np.sort(np.random.RandomState(seed).choice(N, size=min(N, train_size), replace=False))
    xt = torch.cat([_rows(keys, int(s), int(min(N, s + chunk)), device, cosine)[torch.from_numpy(pick[(pick >= s) & (pick < s + chunk)] - s).to(device)]
                    for s in range(0, N, chunk)])
    if d_out < d:
        R = _initial_rotation(xt, d_out, gen)
    if opq_iters > 0:
        R = train_opq(xt, M, R, opq_iters, gen)
    xt = xt @ R.t()
    l2 = metric == "l2"
    assert not (l2 and cosine), "the L2 index takes the keys as they are"
    coarse = kmeans(xt, nlist, iters, gen, spherical=cosine)
    # the list of a vector: the centroid with the largest inner product (IndexFlatIP quantizer) / the nearest one (IndexFlatL2)
    if coarse_fused(nlist, d_out):
        near = torch.empty(xt.shape[0], 1, dtype=torch.int64, device=device)
        ops.ivfpq_coarse_probes(xt, coarse.contiguous(), torch.empty(xt.shape[0], 1, dtype=torch.float32, device=device), near,
                                col_bias=(-0.5 * (coarse ** 2).sum(1)).contiguous() if l2 else None)
        nearest = lambda x: near[:, 0]
    else:
        nearest = lambda x: ((x @ coarse.t()) - (0.5 * (coarse ** 2).sum(1)[None, :] if l2 else 0.0)).argmax(1)
    resid = xt - coarse[nearest(xt)]
    pq = torch.stack([kmeans(resid[:, m * dsub:(m + 1) * dsub].contiguous(), 256, iters, gen) for m in range(M)])
    return R.contiguous(), coarse.contiguous(), pq.contiguous()


def add_rows(R, coarse, pq, list_off, list_ids, list_codes, keys, ids, cosine=True, metric="ip", chunk=1 << 18, coarse_route=None):
    """Add ``keys`` [n, d] with the ids ``ids`` [n] (i64, on the device) to the list-ordered arrays of an index -> the merged
    (list_off, list_ids, list_codes), new tensors; the reference's ``add_with_ids`` loop (knn/index_builder.py:97-109).  Per chunk
    of rows: rotation and coarse scores on ``gnnlm_gemm_nt``, the list of a row by the SEARCH's probe selection at one probe (the
    list the search ranks first for the key as a query, by the same arithmetic; ties to the lowest list), the residual codes by
    ``gnnlm_ivfpq_encode_rows`` (no residual tensor).  Then one placement and one ``gnnlm_ivfpq_list_merge``: new rows go behind
    the old rows of their lists in the order given.  From ``COARSE_FUSED_MIN_LISTS`` lists on (``coarse_route``: "dense" / "fused"
    forces it) the list of a row comes from ``ops.ivfpq_coarse_probes`` at one probe, the search's own coarse step there: no
    [chunk, nlist] scores."""
    device, n, nlist = coarse.device, keys.shape[0], coarse.shape[0]
    M = pq.shape[0]
    assign = torch.empty(n, dtype=torch.int64, device=device)
    codes = torch.empty(n, M, dtype=torch.uint8, device=device)
    n_bad = torch.zeros(1, dtype=torch.int32, device=device)
    norm2 = (pq ** 2).sum(2).contiguous()
    col_bias = -0.5 * (coarse ** 2).sum(1).contiguous() if metric == "l2" else None   # (``IVFPQIndex._block_begin``'s expression)
    select = os.environ.get("GNNLM_IVF_SELECT", "1") != "0"
    fused = coarse_fused(nlist, coarse.shape[1], coarse_route)
    for s in range(0, n, chunk):
        xr = rotated_rows(keys, s, min(n, s + chunk), R, cosine)
        pv = torch.empty(xr.shape[0], 1, dtype=torch.float32, device=device)
        pi = torch.empty(xr.shape[0], 1, dtype=torch.int64, device=device)
        if fused:
            ops.ivfpq_coarse_probes(xr, coarse, pv, pi, col_bias)
        else:
            ops.ivfpq_select_probes(ops.gemm_nt(xr, coarse), pv, pi, col_bias, select)
        a = assign[s:s + chunk]
        a.copy_(pi[:, 0])
        ops.ivfpq_encode_rows(xr, a, coarse, pq, norm2, out=codes[s:s + chunk], n_bad=n_bad)
    if n and int(n_bad.item()):
        raise ValueError(f"ivfpq add: {int(n_bad.item())} keys have no list (NaN rows?)")
    new_off, dest = ops.ivfpq_list_place(assign, list_off)
    new_ids, new_codes = ops.ivfpq_list_merge(list_off, list_ids, list_codes, dest, ids, codes, new_off)
    return new_off, new_ids, new_codes


def normalize_ranges(ids=None, ranges=None, device="cuda"):
    """What to remove, as ``gnnlm_ivfpq_keep_flags`` reads it: i64 [n, 2] on ``device``, half-open [lo, hi) sorted by lo, pairwise
    disjoint and not touching.  ``ids``: single ids (numpy or torch, any order, duplicates allowed), each the range [id, id + 1);
    ``ranges``: (lo, hi) pairs in any order, lo >= hi raises ``ValueError``; overlapping and touching ranges are merged."""
    device = torch.device(device)
    parts = []
    if ranges is not None:
        r = torch.as_tensor(ranges if isinstance(ranges, torch.Tensor) else np.asarray(ranges, dtype=np.int64)).to(device, torch.int64).reshape(-1, 2)
        if r.shape[0] and bool((r[:, 0] >= r[:, 1]).any()):
            raise ValueError("normalize_ranges: every range needs lo < hi (half-open [lo, hi))")
        parts.append(r)
    if ids is not None:
        i = torch.as_tensor(ids if isinstance(ids, torch.Tensor) else np.asarray(ids)).to(device, torch.int64).reshape(-1)
        if i.numel() and int(i.max().item()) == torch.iinfo(torch.int64).max:
            raise ValueError("normalize_ranges: id 2^63 - 1 has no half-open range")
        parts.append(torch.stack([i, i + 1], 1))
    if not parts or sum(p.shape[0] for p in parts) == 0:
        return torch.empty(0, 2, dtype=torch.int64, device=device)
    r = torch.cat(parts)
    r = r[torch.sort(r[:, 0], stable=True).indices]
    lo, hi = r[:, 0], torch.cummax(r[:, 1], 0).values                       # hi of everything that starts no later
    first = torch.ones(r.shape[0], dtype=torch.bool, device=device)
    first[1:] = lo[1:] > hi[:-1]                                            # a range opens where nothing before reaches it
    last = torch.ones_like(first)
    last[:-1] = first[1:]
    return torch.stack([lo[first], hi[last]], 1).contiguous()


def remove_rows(list_off, list_ids, list_codes, ranges):
    """The list-ordered arrays without the keys whose ids lie in ``ranges`` (``normalize_ranges``) -> (new_off, ids, codes), new
    tensors: ``gnnlm_ivfpq_keep_flags``, the cumulative sum of the lists' survivor counts, one read of the total to size the
    outputs exactly, ``gnnlm_ivfpq_list_compact``.  Ids stay what they are (datastore rows); order inside a list is kept."""
    device, nlist = list_off.device, list_off.numel() - 1
    keep, list_keep = ops.ivfpq_keep_flags(list_ids, list_off, ranges)
    new_off = torch.zeros(nlist + 1, dtype=torch.int64, device=device)
    new_off[1:] = torch.cumsum(list_keep, 0)
    n_bad = torch.zeros(1, dtype=torch.int32, device=device)
    ids, codes = ops.ivfpq_list_compact(list_off, list_ids, list_codes, keep, new_off, n_bad=n_bad)
    if int(n_bad.item()):
        raise ValueError(f"ivfpq remove: {int(n_bad.item())} lists do not hold the survivors counted for them")
    return new_off, ids, codes


def merge_lists(off_a, ids_a, codes_a, off_b, ids_b, codes_b):
    """Two sets of list-ordered arrays over the SAME lists as one -> (new_off, ids, codes): per list A's rows, then B's, both in their
    order, through ``ops.ivfpq_list_merge`` with A as the old rows and B's row i of list l at new_off[l] + len_a[l] + (i - off_b[l])."""
    if off_a.shape != off_b.shape or codes_a.shape[1:] != codes_b.shape[1:]:
        raise ValueError("merge_lists: the two indexes differ in their lists or code width")
    nlist, n_b = off_a.numel() - 1, ids_b.numel()
    len_a, len_b = off_a[1:] - off_a[:-1], off_b[1:] - off_b[:-1]
    new_off = torch.zeros(nlist + 1, dtype=torch.int64, device=off_a.device)
    new_off[1:] = torch.cumsum(len_a + len_b, 0)
    list_b = torch.repeat_interleave(torch.arange(nlist, device=off_a.device), len_b, output_size=n_b)   # the list of each row of B
    dest = new_off[:-1][list_b] + len_a[list_b] + (torch.arange(n_b, device=off_a.device) - off_b[:-1][list_b])
    n_bad = torch.zeros(1, dtype=torch.int32, device=off_a.device)
    ids, codes = ops.ivfpq_list_merge(off_a, ids_a, codes_a, dest, ids_b.contiguous(), codes_b.contiguous(), new_off, n_bad=n_bad)
    if int(n_bad.item()):
        raise ValueError(f"ivfpq merge: {int(n_bad.item())} rows have no place (offsets that do not match the rows?)")
    return new_off, ids, codes


def empty_lists(nlist, M, device):
    """the list arrays of an index without keys"""
    return (torch.zeros(nlist + 1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.int64, device=device),
            torch.empty(0, M, dtype=torch.uint8, device=device))


def build_arrays(keys, nlist, M, device="cuda", cosine=True, iters=10, train_size=262144, seed=0, chunk=1 << 18, opq_iters=0,
                 metric="ip", d_out=None):
    """``train`` and ``add_rows`` of every key over an empty index, ids 0 .. N - 1: lists in order, ids ascending inside a list.
    -> (R, coarse, pq, list_off, list_ids, list_codes), the constructor arguments of ``IVFPQIndex``."""
    device = torch.device(device)
    R, coarse, pq = train(keys, nlist, M, device, cosine, iters, train_size, seed, chunk, opq_iters, metric, d_out)
    ids = torch.arange(keys.shape[0], dtype=torch.int64, device=device)
    return (R, coarse, pq) + add_rows(R, coarse, pq, *empty_lists(nlist, M, device), keys, ids, cosine, metric, chunk)
