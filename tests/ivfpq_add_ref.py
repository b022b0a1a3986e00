"""float64 numpy restatement of ADDING keys to an IVF-PQ index (include/gnnlm.h: gnnlm_ivfpq_encode_rows, gnnlm_ivfpq_list_merge;
gnn-lm_amd/ivfpq_train.py: add_rows; the reference: faiss ``add_with_ids`` behind knn/index_builder.py:97-109) -- TEST
INFRASTRUCTURE, pinned by tests/test_ivfpq_add_ref_cpu.py:

  assign      the list of a rotated row: the best coarse score (inner product; L2: <x, c> - |c|^2 / 2), the lowest list on ties
  encode      dist[r, m, c] = norm2[m, c] - 2 <x[r]_m - coarse[assign[r]]_m, pq[m, c]>, code = the first minimiser, and the bound B
              on what the float32 evaluation of the kernel may differ from dist
  place       where new rows go (behind the old rows of their lists, in the order given), merge: the merged arrays
  layout      the list-ordered arrays of a set of (assign, id, code) rows: the stable argsort of assign
  rotated     the exact rotated rows of raw keys and the bound on what float32 normalisation + rotation may differ from them
  assign_bound  the bound on a float32 coarse score computed from the raw key (``rotated``, coarse GEMM, L2 bias)

Every bound is DERIVED from the operations (u = 2^-24, gamma_k = k u / (1 - k u): the standard bound of a k-term float32 sum of
products, any order, fused or not), never measured."""
import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


# ======================================================================================================== assignment
def coarse_scores(xr, coarse, metric="ip"):
    xr, c = np.asarray(xr, np.float64), np.asarray(coarse, np.float64)
    s = xr @ c.T
    return s - 0.5 * (c ** 2).sum(1)[None, :] if metric == "l2" else s


def assign(xr, coarse, metric="ip"):
    """xr [n, d] rotated rows -> the list of each row: the largest score, the lowest list on ties (np.argmax: the first)"""
    return coarse_scores(xr, coarse, metric).argmax(1).astype(np.int64)


def rotated(x, R, cosine):
    """x [n, d] RAW keys (float32 values) -> (xr [n, D] float64 = the exact rotated rows, dx [n, D]): what the float32 pipeline
    x^ = x / sqrt(sum x^2) (cosine), xr^ = x^ R^T may differ from xr, per component.  Derivation: the sum of d squares is good to
    gamma_(d+1) relatively (positive terms), its root to half of that plus u, the quotient to one more u: every component of x^ is off
    by at most en = gamma_(d+1) relatively (cosine; else 0).  A d-term float32 dot product is off by at most gamma_d sum |a_e| |b_e|
    in any order, so dx_j = (gamma_d (1 + en) + en) sum_e |xn_e| |R_je|."""
    x, R = np.asarray(x, np.float64), np.asarray(R, np.float64)
    d = x.shape[1]
    en = gamma(d + 1) if cosine else 0.0
    xn = x / np.sqrt((x ** 2).sum(1, keepdims=True)) if cosine else x
    return xn @ R.T, (gamma(d) * (1 + en) + en) * (np.abs(xn) @ np.abs(R).T)


def assign_bound(x, R, coarse, cosine, metric="ip"):
    """x [n, d] RAW keys -> (score [n, nlist] float64 of the exact pipeline, B [n, nlist]): what the float32 pipeline

        xr^ (``rotated``),  cs = xr^ coarse^T,  score = cs + (-0.5 * sum c^2)  (L2)

    may differ from it.  Derivation: cs_l is off by gamma_D sum_j (|xr_j| + dx_j) |c_lj| for its own D-term sum plus sum_j dx_j |c_lj|
    for its operand (D = the rotated width).  L2: |c|^2 is good to gamma_(D+1) |c|^2, halving is exact, the final addition rounds
    once: u (|cs| + Bcs + |c|^2 (1 + gamma) / 2)."""
    c = np.asarray(coarse, np.float64)
    xr, dx = rotated(x, R, cosine)
    D = xr.shape[1]
    cs = xr @ c.T
    B = gamma(D) * ((np.abs(xr) + dx) @ np.abs(c).T) + dx @ np.abs(c).T
    if metric == "l2":
        n2 = (c ** 2).sum(1)[None, :]
        B = B + 0.5 * gamma(D + 1) * n2 + U * (np.abs(cs) + B + 0.5 * n2 * (1 + gamma(D + 1)))
        cs = cs - 0.5 * n2
    return cs, B


# ======================================================================================================== encode
def encode(x, asg, coarse, pq, norm2):
    """x [n, d] rotated rows (float32 values), asg [n] lists in range -> (dist, B) float64 [n, M, 256].

    dist = norm2[m, c] - 2 sum_e r_e p_e with the EXACT residual r = x - coarse[asg] (float64: differences and products of float32
    values, sums good to 2^-53).  The kernel evaluates, in float32,

        r^_e = fl(x_e - c_e),   dot = fmaf(r^_e, p_e, dot)  (e = 0 .. dsub - 1),   dis = fl(norm2 - 2 dot)

    Derivation of B (A = sum_e |r_e| |p_e|): the fmaf chain is a dsub-term recursive sum, off by at most gamma_dsub sum |r^_e| |p_e|
    <= gamma_dsub (1 + u) A from sum r^_e p_e;  the ONE rounding of the residual moves that sum by at most u A;  so
    |dot - sum r_e p_e| <= ed A with ed = gamma_dsub (1 + u) + u.  Doubling is exact.  The ONE rounding of the result adds at most
    u |norm2 - 2 dot| <= u (|norm2| + 2 (1 + ed) A) (fused into a multiply-add or not).  The reference's own float64 sums add
    (dsub + 2) 2^-53 (|norm2| + 2 A).  B = 2 ed A + u (|norm2| + 2 (1 + ed) A) + (dsub + 2) 2^-53 (|norm2| + 2 A)."""
    n = x.shape[0]
    M, _, dsub = pq.shape
    r = (np.asarray(x, np.float64) - np.asarray(coarse, np.float64)[asg]).reshape(n, M, dsub)
    p64, n2 = np.asarray(pq, np.float64), np.asarray(norm2, np.float64)[None]
    dots = lambda a, b: np.matmul(a.transpose(1, 0, 2), b.transpose(0, 2, 1)).transpose(1, 0, 2)      # "nme,mce->nmc"
    dist = n2 - 2.0 * dots(r, p64)
    A = dots(np.abs(r), np.abs(p64))
    ed = gamma(dsub) * (1 + U) + U
    B = 2 * ed * A + U * (np.abs(n2) + 2 * (1 + ed) * A) + (dsub + 2) * 2.0 ** -53 * (np.abs(n2) + 2 * A)
    return dist, B


def codes_of(dist):
    """the first minimiser: ties go to the lowest c"""
    return dist.argmin(-1).astype(np.uint8)


def encode_excess(codes, dist, B):
    """the worst of dist[chosen] - (min_c dist + B[chosen] + B[argmin]) over every (row, m): <= 0 iff every chosen code satisfies the
    bound condition dist64(chosen) <= min_c dist64(c) + B(chosen) + B(argmin)"""
    c = codes.astype(np.int64)[..., None]
    best = dist.argmin(-1)[..., None]
    pick = lambda a, i: np.take_along_axis(a, i, -1)[..., 0]
    return float((pick(dist, c) - (pick(dist, best) + pick(B, c) + pick(B, best))).max())


def encode_emulate(x, asg, coarse, pq, norm2):
    """float32 codes by the kernel's own chain (each fmaf: the exact float64 product plus the float32 partial sum, rounded once)"""
    n = x.shape[0]
    M, _, dsub = pq.shape
    r = (x.astype(np.float32) - coarse.astype(np.float32)[asg]).reshape(n, M, dsub)
    dot = np.zeros((n, M, 256), dtype=np.float32)
    for e in range(dsub):
        dot = (r[:, :, None, e].astype(np.float64) * pq[None, :, :, e].astype(np.float64) + dot.astype(np.float64)).astype(np.float32)
    return (norm2[None].astype(np.float32) - np.float32(2) * dot).argmin(-1).astype(np.uint8)


# ======================================================================================================== placement and merge
def place(asg, list_off_old):
    """-> (new_off [nlist + 1], dest [n]): new_off = cumulative (old length + new count); the new rows of a list in the order given
    behind its old rows"""
    asg, off = np.asarray(asg, np.int64), np.asarray(list_off_old, np.int64)
    nlist = len(off) - 1
    old_len = off[1:] - off[:-1]
    cnt = np.bincount(asg, minlength=nlist).astype(np.int64)
    new_off = np.zeros(nlist + 1, np.int64)
    new_off[1:] = np.cumsum(old_len + cnt)
    dest = np.empty(len(asg), np.int64)
    seen = np.zeros(nlist, np.int64)
    for i, l in enumerate(asg):
        dest[i] = new_off[l] + old_len[l] + seen[l]
        seen[l] += 1
    return new_off, dest


def merge(list_off_old, ids_old, codes_old, dest, ids_new, codes_new, new_off, fill=0):
    """-> (ids [N0 + n], codes [N0 + n, M], n_bad); positions nothing lands on keep `fill`; a dest outside [0, N0 + n) is skipped"""
    off = np.asarray(list_off_old, np.int64)
    N0, n, M = len(ids_old), len(ids_new), codes_new.shape[1]
    ids = np.full(N0 + n, fill, np.int64)
    codes = np.full((N0 + n, M), fill, np.uint8)
    for l in range(len(off) - 1):
        lo, hi = int(off[l]), int(off[l + 1])
        ids[new_off[l]:new_off[l] + hi - lo] = ids_old[lo:hi]
        codes[new_off[l]:new_off[l] + hi - lo] = codes_old[lo:hi]
    bad = 0
    for i in range(n):
        if 0 <= dest[i] < N0 + n:
            ids[dest[i]], codes[dest[i]] = ids_new[i], codes_new[i]
        else:
            bad += 1
    return ids, codes, bad


def layout(asg, ids, codes, nlist):
    """the list-ordered arrays of rows given in id order: (list_off, list_ids, list_codes) by the stable argsort of the lists"""
    asg = np.asarray(asg, np.int64)
    order = np.argsort(asg, kind="stable")
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(asg, minlength=nlist))
    return off, np.asarray(ids)[order], np.asarray(codes)[order]


def add(R, coarse, pq, list_off, list_ids, list_codes, keys, ids, cosine=False, metric="ip"):
    """the whole add path in float64 (exact on integer-valued operands): -> the merged (list_off, list_ids, list_codes)"""
    x = np.asarray(keys, np.float64)
    if cosine:
        x = x / np.sqrt((x ** 2).sum(1, keepdims=True))
    xr = x @ np.asarray(R, np.float64).T
    asg = assign(xr, coarse, metric)
    dist, _ = encode(xr, asg, coarse, pq, (np.asarray(pq, np.float64) ** 2).sum(2))
    new_off, dest = place(asg, list_off)
    ids_m, codes_m, bad = merge(list_off, list_ids, list_codes, dest, np.asarray(ids, np.int64), codes_of(dist), new_off)
    assert bad == 0
    return new_off, ids_m, codes_m
