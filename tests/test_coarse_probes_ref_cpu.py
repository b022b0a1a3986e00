"""tests/coarse_probes_ref.py pinned: against oracle/ivfpq.py on a small index (the oracle's search at nprobe = P must be the float64
search restricted to exactly the lists the restatement picks, inner product and L2), and its tie and padding rules by hand."""
import numpy as np
import pytest

import coarse_probes_ref as ref
from oracle import ivfpq as oracle


def _index(seed, nlist=40, d=16, M=4, N=900):
    rs = np.random.RandomState(seed)
    R = np.linalg.qr(rs.randn(d, d))[0].astype(np.float32)
    coarse = rs.randn(nlist, d).astype(np.float32)
    pq = (0.3 * rs.randn(M, 256, d // M)).astype(np.float32)
    assign = np.sort(rs.randint(0, nlist - 3, N))                          # the last three lists are empty
    list_off = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int64)
    list_ids = rs.permutation(N).astype(np.int64)
    list_codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
    return R, coarse, pq, list_off, list_ids, list_codes


def _restricted(qr, lists, bias, coarse, pq, list_off, list_ids, list_codes, k, metric):
    """float64 search of every row over the lists given (best first, -1: none), by the oracle's formulas"""
    M, _, dsub = pq.shape
    cen, pq64 = coarse.astype(np.float64), pq.astype(np.float64)
    sign = -1.0 if metric == "l2" else 1.0
    out_v = np.full((len(qr), k), sign * -np.inf)
    out_i = np.full((len(qr), k), -1, np.int64)
    for r in range(len(qr)):
        vs, ids = [], []
        for l in lists[r]:
            lo, hi = int(list_off[l]), int(list_off[l + 1])
            if l < 0 or hi == lo:
                continue
            c = list_codes[lo:hi].astype(np.int64)
            dec = pq64[np.arange(M)[None, :], c].reshape(hi - lo, M * dsub)
            if metric == "l2":
                vs.append((((qr[r] - cen[l])[None, :] - dec) ** 2).sum(1))
            else:
                lut = np.einsum("md,mcd->mc", qr[r].reshape(M, dsub), pq64)
                vs.append(qr[r] @ cen[l] + lut[np.arange(M)[None, :], c].sum(1))
            ids.append(list_ids[lo:hi])
        if not vs:                                                         # every list picked is empty
            continue
        v, i = np.concatenate(vs), np.concatenate(ids)
        top = np.lexsort((i, sign * -v))[:k]
        out_v[r, :len(top)], out_i[r, :len(top)] = v[top], i[top]
    return out_v, out_i


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("P", [1, 5, 40])
def test_oracle_search_probes_the_lists_the_restatement_picks(metric, P):
    R, coarse, pq, list_off, list_ids, list_codes = _index(3)
    q = np.random.RandomState(4).randn(23, 16).astype(np.float32)
    k = 7
    qr = q.astype(np.float64) @ R.astype(np.float64).T
    bias = -0.5 * (coarse.astype(np.float64) ** 2).sum(1) if metric == "l2" else None
    pv, pi = ref.coarse_probes(qr, coarse, P, bias)
    assert (pi >= 0).all() and (np.diff(pv, axis=1) <= 0).all()
    want_v, want_i = oracle.search(q, R, coarse, pq, list_off, list_ids, list_codes, k, P, metric=metric)
    got_v, got_i = _restricted(qr, pi, bias, coarse, pq, list_off, list_ids, list_codes, k, metric)
    assert np.array_equal(got_i, want_i)
    np.testing.assert_allclose(got_v, want_v, rtol=1e-12, atol=1e-12)
    if metric == "l2":                                                    # the value of a probe is the list's distance: 2 pv - |q'|^2 = -|q' - c|^2
        d2 = ((qr[:, None, :] - coarse.astype(np.float64)[pi]) ** 2).sum(2)
        np.testing.assert_allclose(2.0 * pv - (qr ** 2).sum(1, keepdims=True), -d2, rtol=1e-9, atol=1e-9)


def test_ties_go_to_the_lower_list_and_zeros_tie():
    s = np.array([[1.0, 3.0, 3.0, 2.0, 3.0, -0.0, 0.0],
                  [0.0, -0.0, -1.0, 0.0, -0.0, -2.0, -1.0]])
    v, i = ref.select(s, 4)
    assert i.tolist() == [[1, 2, 4, 3], [0, 1, 3, 4]]
    assert v.tolist() == [[3.0, 3.0, 3.0, 2.0], [0.0, 0.0, 0.0, 0.0]]
    x = np.array([[1.0, 0.0], [0.0, 1.0]])
    c = np.array([[2.0, 5.0], [2.0, 5.0], [2.0, 4.0]])
    v, i = ref.coarse_probes(x, c, 2)
    assert i.tolist() == [[0, 1], [0, 1]] and v.tolist() == [[2.0, 2.0], [5.0, 5.0]]
    v, i = ref.coarse_probes(x, c, 2, col_bias=np.array([0.0, 1.0, 3.0]))
    assert i.tolist() == [[2, 1], [2, 1]] and v.tolist() == [[5.0, 3.0], [7.0, 6.0]]


def test_no_entry_and_padding():
    inf, nan = np.inf, np.nan
    s = np.array([[nan, -inf, 2.0, inf, nan],
                  [nan, nan, -inf, -inf, nan],
                  [1.0, 2.0, 3.0, 4.0, 5.0]])
    v, i = ref.select(s, 3)
    assert i.tolist() == [[3, 2, -1], [-1, -1, -1], [4, 3, 2]]
    assert v[0].tolist() == [inf, 2.0, -inf] and np.isneginf(v[1]).all()
    v, i = ref.select(np.zeros((2, 0)), 2)                                # no list at all
    assert (i == -1).all() and np.isneginf(v).all()
    x = np.array([[1.0, 1.0], [nan, 1.0]])                                # a NaN row has no list; its neighbour is not disturbed
    c = np.array([[1.0, 0.0], [0.0, 2.0]])
    v, i = ref.coarse_probes(x, c, 2, col_bias=np.array([0.0, nan]))
    assert i.tolist() == [[0, -1], [-1, -1]] and v[0, 0] == 1.0
