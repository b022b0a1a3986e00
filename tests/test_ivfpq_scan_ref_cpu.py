"""tests/ivfpq_scan_ref.py is right before it judges a kernel: its three score formulas, sorted and cut to k, are the float64
IVFADC oracle's search (oracle/ivfpq.py) over a hand-made index, and its packed layouts invert.  No GPU."""
import numpy as np
import pytest

import ivfpq_scan_ref as ref
from oracle import ivfpq as oivf

M, DSUB, NPROBE = 16, 4, 3
LIST_SIZES = [0, 1, 63, 64, 65, 129, 0, 7]


@pytest.fixture(scope="module")
def index():
    """Index arrays made by hand (the style of random_index_arrays in test_ivfpq_l2_gpu.py), everything the scan needs in float64."""
    rs = np.random.RandomState(5)
    nlist, N, d = len(LIST_SIZES), int(np.sum(LIST_SIZES)), M * DSUB
    R = np.linalg.qr(rs.randn(d, d))[0].astype(np.float32)
    coarse = rs.randn(nlist, d).astype(np.float32)
    pq = (0.3 * rs.randn(M, 256, DSUB)).astype(np.float32)
    off = np.zeros(nlist + 1, dtype=np.int64)
    off[1:] = np.cumsum(LIST_SIZES)
    ids = rs.permutation(N).astype(np.int64) + 11
    codes = rs.randint(0, 256, (N, M)).astype(np.uint8)
    q = rs.randn(6, d).astype(np.float32)
    qr = q.astype(np.float64) @ R.astype(np.float64).T
    cen, pq64 = coarse.astype(np.float64), pq.astype(np.float64)
    lut = np.einsum("nmd,mcd->nmc", qr.reshape(len(q), M, DSUB), pq64)                       # <q'_m, p_mc>
    list_term = (pq64 ** 2).sum(2)[None] + 2.0 * np.einsum("lmd,mcd->lmc", cen.reshape(nlist, M, DSUB), pq64)
    lists = np.searchsorted(off, np.arange(N), side="right") - 1
    key_term = list_term[lists[:, None], np.arange(M)[None, :], codes.astype(np.int64)].sum(1)
    return dict(arrs=[R, coarse, pq, off, ids, codes], q=q, qr=qr, cen=cen, lut=lut, list_term=list_term, key_term=key_term, N=N)


def search_with_ref(ix, probes, bias, k, **terms):
    """Every score of the probed lists by scan_ref, best first (ties by ascending id), cut to k: (scores [n, k], ids [n, k]), -inf / -1
    where the lists run out."""
    _, _, _, off, ids, codes = ix["arrs"]
    n = len(probes)
    out_v, out_i = np.full((n, k), -np.inf), np.full((n, k), -1, dtype=np.int64)
    for r in range(n):
        parts = [ref.scan_ref(codes, off, ix["lut"], probes, bias, r, p, **terms) for p in range(probes.shape[1])]
        v, rows = np.concatenate([x[0] for x in parts]), np.concatenate([x[2] for x in parts])
        i = ids[rows]
        top = np.lexsort((i, -v))[:k]
        out_v[r, :len(top)], out_i[r, :len(top)] = v[top], i[top]
    return out_v, out_i


@pytest.mark.parametrize("k", [10, 400])
def test_inner_product_is_the_oracle(index, k):
    cs = index["qr"] @ index["cen"].T
    probes = np.argsort(-cs, axis=1, kind="stable")[:, :NPROBE]
    v, i = search_with_ref(index, probes, np.take_along_axis(cs, probes, 1), k)
    v_ref, i_ref = oivf.search(index["q"], *index["arrs"], k=k, nprobe=NPROBE, metric="ip")
    assert np.array_equal(i, i_ref)
    assert (i[:, 0] >= 0).all() and (k < 400 or (i[:, -1] == -1).all())        # k = 400 runs past the probed lists of every query
    np.testing.assert_allclose(v, v_ref, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("route", ["list_term", "key_term"])
@pytest.mark.parametrize("k", [10, 400])
def test_l2_is_the_oracle(index, k, route):
    qr, cen = index["qr"], index["cen"]
    d2c = (qr ** 2).sum(1)[:, None] - 2 * qr @ cen.T + (cen ** 2).sum(1)[None, :]
    probes = np.argsort(d2c, axis=1, kind="stable")[:, :NPROBE]
    bias = -((qr[:, None, :] - cen[probes]) ** 2).sum(2)                       # -|q' - c_l|^2
    v, i = search_with_ref(index, probes, bias, k, **{route: index[route]})
    d_ref, i_ref = oivf.search(index["q"], *index["arrs"], k=k, nprobe=NPROBE, metric="l2")
    assert np.array_equal(i, i_ref)
    np.testing.assert_allclose(-v, d_ref, rtol=1e-9, atol=1e-9)


def test_minus_one_slot_and_magnitude(index):
    _, _, _, off, _, codes = index["arrs"]
    probes, bias = np.array([[-1, 5]]), np.array([[0.5, -2.0]])
    s, mag, rows = ref.scan_ref(codes, off, index["lut"][:1], probes, bias, 0, 0)
    assert len(s) == len(mag) == len(rows) == 0
    for terms in ({}, {"list_term": index["list_term"]}, {"key_term": index["key_term"]}):
        s, mag, rows = ref.scan_ref(codes, off, index["lut"][:1], probes, bias, 0, 1, **terms)
        assert len(s) == 129 and np.array_equal(rows, np.arange(off[5], off[6])) and (mag >= np.abs(s)).all() and (mag >= 2.0).all()


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 3729])
@pytest.mark.parametrize("M_", [32, 64])
def test_packed_codes_round_trip(N, M_):
    codes = np.random.RandomState(N + M_).randint(0, 256, (N, M_)).astype(np.uint8)
    img = ref.pack_codes_ref(codes)
    assert img.dtype == np.uint8 and img.shape == ((N + 63) // 64 * 64 * M_,)
    assert np.array_equal(ref.unpack_codes_ref(img, N, M_), codes)
    if N % 64:                                                                 # rows beyond N are zero
        assert not img.reshape(-1, M_ // 16, 64, 16)[-1, :, N % 64:, :].any()
    if N > 40:                                                                 # one entry spelled out: row 37, half h, byte 5 -> code (37 + 5) mod 32
        for h in range(M_ // 32):
            assert img[(2 * h) * 1024 + 37 * 16 + 5] == codes[37, 32 * h + 10]


def test_packed_tables_and_tasks():
    lut = np.random.RandomState(2).randn(3, 64, 256).astype(np.float32)
    out = ref.pack_lut_ref(lut)
    assert out.shape == (3, 2, 256, 32) and out[2, 1, 200, 7] == lut[2, 39, 200] and out[0, 0, 3, 31] == lut[0, 31, 3]
    tq, tp = ref.task_table(ref.PROBES, 1, 4)
    assert len(tq) == 15 and ref.PROBES[tq, tp].tolist() == [-1, 0, 1, 2, 3, 4, 5, 5, 6, 7, 8, 8, 9, 9, 9]
    assert (tq[6], tp[6], tq[7], tp[7]) == (0, 2, 3, 3)                        # stable: equal lists keep (query, slot) order
    tq, tp = ref.task_table(ref.PROBES, 0, 4)
    assert ref.PROBES[tq, tp].tolist() == [-1, 0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 7, 8, 8, 8, 8, 9, 9, 9]


@pytest.mark.parametrize("M_", [16, 32, 64, 128])
@pytest.mark.parametrize("formula", ref.FORMULAS)
def test_thresholds_of_the_filtered_test_are_decided_by_the_reference(M_, formula):
    """The condition test_ivfpq_scan_abi_gpu.py's filtered test rests on, on its own data: no reference score within one bar of tau."""
    D = ref.make_data(M_)
    for q in range(D["n"]):
        s, mag, _ = ref.query_scores(D, formula, q, 0, D["P"])
        for rank in (20, 100, 1000):
            tau = float(ref.gap_threshold(s, rank))
            assert (np.abs(s - tau) > ref.bar(M_, mag)).all(), (q, rank, float((np.abs(s - tau) / ref.bar(M_, mag)).min()))
