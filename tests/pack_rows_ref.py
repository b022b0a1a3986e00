"""Restatement of ``gnnlm_pack_rows`` (include/gnnlm.h) for the tests: which source row every output row is, the copy, the unit rows
in float64, and the bound a float32 evaluation of the unit rows has to meet.  Imports neither the package under test nor the reference.

The kernel's expression for the unit rows is the reference's own (knn/knn_model.py:181-184), a DIVISION:

    y = fl32(x / fl32(sqrt(s^))),   s^ = a float32 sum of the d squares x_i^2 in some order (products fused into the sum or not)

Bound, with u = 2^-24 the unit roundoff of float32 (the way tests/ivfpq_scan_ref.py derives its bound: count the roundings, take the
standard gamma bound for the sum, add nothing measured):

  * the sum: every term passes through at most d roundings (its own product, then at most d - 1 additions; a fused product has one
    fewer), all terms are >= 0, so s^ = s (1 + e1) with |e1| <= gamma_d = d u / (1 - d u), whatever the order;
  * the square root is correctly rounded: n^ = sqrt(s^) (1 + e2), |e2| <= u, and sqrt(1 + e1) lies within 1 +- gamma_d / 2 (1 + gamma_d);
  * the division is correctly rounded: y = (x / n^) (1 + e3), |e3| <= u -- or, when the quotient is subnormal, off by at most 2^-149.

  |y - x / sqrt(s)| <= |x / sqrt(s)| * (d / 2 + 2) u * (1 + 1e-2) + 2^-149

The factor 1.01 pays for every second-order term: at d = 1024 gamma_d is 6.1e-5, so the products of two relative errors are below
1e-4 of the first-order term.  A zero row is 0 / 0 = NaN in every element, as the reference's expression gives; an overflowing sum
(s^ = inf) gives 0 -- neither is special-cased, and the tests keep |x| far from 1.8e19.
"""
import numpy as np

U = 2.0 ** -24


def tables(lengths, skips=None, base=0):
    """-> (block_off [n + 1] with block_off[0] = base, skip [n], out_off [n + 1]) as int32, from block lengths and skips."""
    lengths = np.asarray(lengths, np.int64)
    skips = np.zeros_like(lengths) if skips is None else np.asarray(skips, np.int64)
    block_off = base + np.concatenate([[0], np.cumsum(lengths)])
    out_off = np.concatenate([[0], np.cumsum(lengths - skips)])
    return block_off.astype(np.int32), skips.astype(np.int32), out_off.astype(np.int32)


def source_rows(block_off, skip, out_off):
    """The source row of every output row, int64 [n_out]."""
    block_off = np.asarray(block_off, np.int64) - int(block_off[0])
    n = len(block_off) - 1
    skip = np.zeros(n, np.int64) if skip is None else np.asarray(skip, np.int64)
    rows = [np.arange(block_off[b] + skip[b], block_off[b + 1]) for b in range(n)]
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    assert len(rows) == int(out_off[-1]) - int(out_off[0])
    return rows.astype(np.int64)


def pack(src, block_off, skip, out_off, d):
    """-> (rows float32 [n_out, d] -- the copy --, unit float64 [n_out, d] = x / sqrt(sum x^2) in float64; a zero row is NaN)."""
    r = source_rows(block_off, skip, out_off)
    rows = np.asarray(src)[r, :d].astype(np.float32)
    x = rows.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = x / np.sqrt((x ** 2).sum(-1, keepdims=True))
    return rows, unit


def unit_tolerance(unit64, d):
    """Element-wise bound on |y - unit64| for a float32 evaluation y of the kernel's expression (module docstring)."""
    return np.abs(unit64) * ((d / 2.0 + 2.0) * U * 1.01) + 2.0 ** -149


def unit_f32(rows, order="forward"):
    """The kernel's expression evaluated in numpy float32 with the sum taken in a given order -- what the bound must cover."""
    x = np.asarray(rows, np.float32)
    sq = (x * x).astype(np.float32)
    if order == "forward":
        s = np.zeros(x.shape[0], np.float32)
        for j in range(x.shape[1]):
            s = (s + sq[:, j]).astype(np.float32)
    elif order == "reverse":
        s = np.zeros(x.shape[0], np.float32)
        for j in range(x.shape[1] - 1, -1, -1):
            s = (s + sq[:, j]).astype(np.float32)
    elif order == "lanes":                     # 64 partial sums with stride 64, then a tree over them: the shape of a wave's reduction
        part = np.zeros((x.shape[0], 64), np.float32)
        for j in range(x.shape[1]):
            part[:, j % 64] = (part[:, j % 64] + sq[:, j]).astype(np.float32)
        w = 64
        while w > 1:
            w //= 2
            part = (part[:, :w] + part[:, w:2 * w]).astype(np.float32)
        s = part[:, 0]
    else:
        raise ValueError(order)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x / np.sqrt(s).astype(np.float32)[:, None]).astype(np.float32)
