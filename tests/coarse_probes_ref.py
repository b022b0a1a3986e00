"""Float64 restatement of gnnlm_ivfpq_coarse_probes (include/gnnlm.h, gnnlm_ivfpq_coarse_t): the P best lists of every row.

    score[r][l] = <x[r], coarse[l]> (+ col_bias[l]),  taken in float64
    a list whose score is NaN or -inf is no entry;  the others are ordered by larger score first, then lower list (-0 == +0);
    the first P of them are returned, rows with fewer are padded with (-inf, -1).

tests/test_coarse_probes_ref_cpu.py pins it against oracle/ivfpq.py; the GPU tests hold the kernel to it."""
import numpy as np


def scores(x, coarse, col_bias=None):
    """[n, nlist] float64"""
    with np.errstate(invalid="ignore"):
        s = np.asarray(x, np.float64) @ np.asarray(coarse, np.float64).T
        if col_bias is not None:
            s = s + np.asarray(col_bias, np.float64)[None, :]
    return s


def select(s, P):
    """The P best columns of every row of s [n, ncols] by the rules above -> (val [n, P] float64, id [n, P] int64)."""
    n, ncols = s.shape
    val = np.full((n, P), -np.inf, np.float64)
    idx = np.full((n, P), -1, np.int64)
    for r in range(n):
        row = s[r]
        live = np.nonzero(~np.isnan(row) & (row != -np.inf))[0]
        if live.size == 0:
            continue
        v = row[live] + 0.0                                            # (-0 -> +0: the two tie)
        order = np.lexsort((live, -v))[:P]                             # larger value first, then the lower list
        val[r, :order.size] = v[order]
        idx[r, :order.size] = live[order]
    return val, idx


def coarse_probes(x, coarse, P, col_bias=None):
    return select(scores(x, coarse, col_bias), P)
