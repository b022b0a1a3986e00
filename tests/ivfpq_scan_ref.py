"""Float64 restatement of ``gnnlm_ivfpq_scan`` (include/gnnlm.h: gnnlm_ivfpq_scan_t) over plain arrays, shared by
test_ivfpq_scan_ref_cpu.py and test_ivfpq_scan_abi_gpu.py: the three score formulas with the magnitude the error bar is taken
of, the task table of ``IVFPQIndex._scan``, the two packed layouts of gnnlm_ivfpq_pack_codes / gnnlm_ivfpq_pack_lut, and the
hand-made data set the descriptor-level tests run on.  numpy only.

The bar.  The kernels add M table entries, the bias and (L2) the key's term in float32, in an order of their own.  A float32
sum of M + 2 terms in any order differs from the exact sum by at most (M + 3) * 2^-24 * (sum of the terms' absolute values) to
first order (one rounding of at most 2^-24 relative per addition, each acting on a partial sum no larger than the sum of the
absolute values; the list_term formula rounds 2 a - b once more per entry, the key_term formula's fma and subtraction are two of
the M + 1 operations).  ``bar(M, mag)`` is that bound: derived, not measured."""
import numpy as np

SIZES = [0, 1, 63, 64, 65, 129, 0, 7, 1100, 2300]        # rows per list: empty lists, lists inside / across 64-row blocks, a last
N_ROWS = int(np.sum(SIZES))                              # partial block, more than 16 waves x 64 rows, more than STAGE_CAP = 1024
N_QUERIES, N_PROBES = 5, 4
BIG_ID = (1 << 40) + 12345
# probed lists [query, slot].  Slots 1..3 give 15 tasks (odd, no multiple of 16), sorted by list:
#   -1 0 | 1 2 | 3 4 | 5 5 | 6 7 | 8 8 | 9 9 | 9      a -1 slot, pairs across a list boundary, pairs inside one list (129, 1100 and
# 2300 rows), a last workgroup with one task.  Slots 0..3 give 20 tasks:  -1 0 | 1 1 | 2 2 | 3 3 | 4 5 | 5 6 | 7 8 | 8 8 | 8 9 | 9 9
PROBES = np.array([[3, 9, 5, -1],
                   [8, 9, 0, 2],
                   [8, 4, 9, 7],
                   [1, 8, 6, 5],
                   [2, 8, 1, 3]], dtype=np.int64)
FORMULAS = ("ip", "list_term", "key_term")


def bar(M, mag):
    return (M + 3) * 2.0 ** -24 * np.asarray(mag, dtype=np.float64)


def scan_ref(codes, list_off, lut, probe_list, probe_bias, q, slot, list_term=None, key_term=None):
    """Scores of task (q, slot) over the rows of its list, float64: (scores [len], mag [len], rows [len]) -- ``rows`` the row
    numbers in the list-ordered arrays (ids[rows] are the keys); empty for a -1 slot or an empty list.
        inner product:  bias + sum_m lut[q, m, code]
        list_term:      bias + sum_m (2 lut[q, m, code] - list_term[l, m, code])
        key_term:       bias + 2 sum_m lut[q, m, code] - key_term[r]
    ``mag`` is the sum of the absolute values of every term that enters the score."""
    assert list_term is None or key_term is None
    l = int(probe_list[q, slot])
    if l < 0:
        z = np.zeros(0)
        return z, z.copy(), np.zeros(0, dtype=np.int64)
    rows = np.arange(int(list_off[l]), int(list_off[l + 1]), dtype=np.int64)
    M = codes.shape[1]
    c = codes[rows].astype(np.int64)                                          # [len, M]
    t = np.asarray(lut[q], dtype=np.float64)[np.arange(M)[None, :], c]         # [len, M]
    bias = float(probe_bias[q, slot])
    if list_term is not None:
        lt = np.asarray(list_term[l], dtype=np.float64)[np.arange(M)[None, :], c]
        return bias + (2.0 * t - lt).sum(1), abs(bias) + (2.0 * np.abs(t) + np.abs(lt)).sum(1), rows
    if key_term is not None:
        kt = np.asarray(key_term, dtype=np.float64)[rows]
        return bias + 2.0 * t.sum(1) - kt, abs(bias) + 2.0 * np.abs(t).sum(1) + np.abs(kt), rows
    return bias + t.sum(1), abs(bias) + np.abs(t).sum(1), rows


def task_table(probe_list, p_lo, p_hi):
    """(task_q, task_p) int32 of the probe slots [p_lo, p_hi) of every query, as ``IVFPQIndex._scan`` makes them: a stable sort of
    the (query, slot) pairs by list."""
    w = p_hi - p_lo
    order = np.argsort(probe_list[:, p_lo:p_hi].reshape(-1), kind="stable")
    return (order // w).astype(np.int32), (order % w + p_lo).astype(np.int32)


def pack_codes_ref(codes):
    """codes [N, M] (M = 32 or 64) -> the packed image, ceil(N / 64) * 64 * M bytes: blocks of 64 rows stored [M/16][64][16 B];
    byte s of half h of row r is code[r][32 h + (r + s) mod 32]; rows beyond N are zero."""
    N, M = codes.shape
    nb = (N + 63) // 64
    img = np.zeros((nb, M // 16, 64, 16), dtype=np.uint8)
    r = np.arange(N)
    for pc in range(M // 16):
        for i in range(16):
            idx = pc * 16 + i
            h, s = idx // 32, idx % 32
            img[r // 64, pc, r % 64, i] = codes[r, 32 * h + (r + s) % 32]
    return img.reshape(-1)


def unpack_codes_ref(img, N, M):
    """The inverse of pack_codes_ref, by the same formula read the other way."""
    img = np.asarray(img, dtype=np.uint8).reshape(-1, M // 16, 64, 16)
    codes = np.zeros((N, M), dtype=np.uint8)
    r = np.arange(N)
    for h in range(M // 32):
        for s in range(32):
            idx = 32 * h + s
            codes[r, 32 * h + (r + s) % 32] = img[r // 64, idx // 16, r % 64, idx % 16]
    return codes


def pack_lut_ref(lut):
    """lut [n, M, 256] -> [n, M/32, 256, 32]: entry (q, h, c, s) = lut[q, 32 h + s, c]."""
    n, M, _ = lut.shape
    return np.ascontiguousarray(lut.reshape(n, M // 32, 32, 256).transpose(0, 1, 3, 2))


def make_data(M, seed=None):
    """The data set of the descriptor-level tests for one M: random tables, biases, codes and L2 terms (the scan does not care where
    they come from), ids = a permutation plus an offset with one id above 2^40 (in the 2300-row list)."""
    rs = np.random.RandomState(1000 + M if seed is None else seed)
    nlist = len(SIZES)
    off = np.zeros(nlist + 1, dtype=np.int64)
    off[1:] = np.cumsum(SIZES)
    ids = rs.permutation(N_ROWS).astype(np.int64) + 11
    ids[int(off[9]) + 1500] = BIG_ID
    return dict(M=M, N=N_ROWS, n=N_QUERIES, P=N_PROBES, nlist=nlist, list_off=off, ids=ids,
                codes=rs.randint(0, 256, (N_ROWS, M)).astype(np.uint8),
                lut=rs.randn(N_QUERIES, M, 256).astype(np.float32),
                probe_list=PROBES.copy(), probe_bias=(3.0 * rs.randn(N_QUERIES, N_PROBES)).astype(np.float32),
                list_term=rs.randn(nlist, M, 256).astype(np.float32),
                key_term=(np.sqrt(M) * rs.randn(N_ROWS)).astype(np.float32))


def formula_terms(D, formula):
    """The optional arguments of scan_ref for a formula name."""
    assert formula in FORMULAS
    return dict(list_term=D["list_term"] if formula == "list_term" else None, key_term=D["key_term"] if formula == "key_term" else None)


def query_scores(D, formula, q, p_lo, p_hi):
    """Every (score, mag, row) of query q over its probe slots [p_lo, p_hi), concatenated in slot order."""
    parts = [scan_ref(D["codes"], D["list_off"], D["lut"], D["probe_list"], D["probe_bias"], q, p, **formula_terms(D, formula))
             for p in range(p_lo, p_hi)]
    return tuple(np.concatenate(x) for x in zip(*parts))


def gap_threshold(scores, rank):
    """tau of the filtered tests: the midpoint (as float32) of the widest gap among the 32 order statistics around ``rank`` of the
    descending scores."""
    s = np.sort(scores)[::-1][rank - 16:rank + 16]
    assert len(s) == 32
    g = int(np.argmax(s[:-1] - s[1:]))
    return np.float32(0.5 * (s[g] + s[g + 1]))
