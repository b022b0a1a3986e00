"""Adding keys to an IVF-PQ index without a GPU: the float64 restatement (tests/ivfpq_add_ref.py) pinned three ways -- brute-force
minimisers on a tiny case; merge(build(A), B) against the stable-argsort layout of A u B, array for array; both layouts through
``oracle.ivfpq.search`` -- the derived encode bound against a float32 emulation of the kernel's chain, and the ABI additions."""
import ctypes
import re

import numpy as np

import ivfpq_add_ref as ar
from oracle import ivfpq as oracle_ivfpq


def _index(rs, nlist, M, dsub, integer=True):
    d = M * dsub
    if integer:
        coarse = rs.randint(-4, 5, size=(nlist, d)).astype(np.float32)
        pq = rs.randint(-3, 4, size=(M, 256, dsub)).astype(np.float32)
        R = np.eye(d, dtype=np.float32)[rs.permutation(d)]
    else:
        coarse, pq = rs.randn(nlist, d).astype(np.float32), (0.5 * rs.randn(M, 256, dsub)).astype(np.float32)
        R = np.linalg.qr(rs.randn(d, d))[0].astype(np.float32)
    return R, coarse, pq


def test_brute_force_minimisers():
    rs = np.random.RandomState(0)
    nlist, M, dsub, n = 3, 2, 4, 7
    _, coarse, pq = _index(rs, nlist, M, dsub)
    pq[:, 9] = pq[:, 200]                                                 # exact ties exist
    x = rs.randint(-8, 9, size=(n, M * dsub)).astype(np.float32)
    for metric in ("ip", "l2"):
        asg = ar.assign(x, coarse, metric)
        for r in range(n):
            if metric == "ip":
                sc = [sum(float(x[r, e]) * float(coarse[l, e]) for e in range(M * dsub)) for l in range(nlist)]
            else:
                sc = [-0.5 * sum((float(x[r, e]) - float(coarse[l, e])) ** 2 for e in range(M * dsub)) for l in range(nlist)]   # nearest = best
            best = max(sc)
            assert asg[r] == min(l for l in range(nlist) if sc[l] == best)
        norm2 = (pq.astype(np.float64) ** 2).sum(2)
        dist, B = ar.encode(x, asg, coarse, pq, norm2)
        codes = ar.codes_of(dist)
        for r in range(n):
            for m in range(M):
                res = x[r, m * dsub:(m + 1) * dsub].astype(np.float64) - coarse[asg[r], m * dsub:(m + 1) * dsub]
                full = [float(((res - pq[m, c]) ** 2).sum()) for c in range(256)]          # |r - p|^2 = |r|^2 + dist
                lo = min(full)
                assert codes[r, m] == min(c for c in range(256) if full[c] == lo)
                assert np.allclose(np.array(full) - (res ** 2).sum(), dist[r, m], atol=1e-9)
        assert (B > 0).all() and ar.encode_excess(codes, dist, B) <= 0
    assert (codes == 9).sum() + (codes == 200).sum() == (codes == 9).sum()    # of a tied pair the lower code wins


def test_l2_assignment_is_the_nearest_centroid():
    rs = np.random.RandomState(1)
    coarse, x = rs.randn(9, 8), rs.randn(50, 8)
    d2 = ((x[:, None, :] - coarse[None]) ** 2).sum(-1)
    assert np.array_equal(ar.assign(x, coarse, "l2"), d2.argmin(1))


def test_merge_of_build_equals_the_layout_of_the_union():
    rs = np.random.RandomState(2)
    for nlist, M, dsub, nA, nB in [(1, 16, 4, 10, 5), (5, 16, 4, 300, 120), (7, 16, 4, 0, 50), (7, 16, 4, 40, 0), (40, 16, 4, 30, 25)]:
        R, coarse, pq = _index(rs, nlist, M, dsub)
        keys = rs.randint(-8, 9, size=(nA + nB, M * dsub)).astype(np.float32)
        empty = (np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, M), np.uint8))
        ids = np.arange(nA + nB)
        one = ar.add(R, coarse, pq, *empty, keys, ids)
        two = ar.add(R, coarse, pq, *ar.add(R, coarse, pq, *empty, keys[:nA], ids[:nA]), keys[nA:], ids[nA:])
        xr = keys.astype(np.float64) @ R.T.astype(np.float64)
        asg = ar.assign(xr, coarse)
        want = ar.layout(asg, ids, ar.codes_of(ar.encode(xr, asg, coarse, pq, (pq.astype(np.float64) ** 2).sum(2))[0]), nlist)
        for a, b, c in zip(one, two, want):
            assert np.array_equal(a, c) and np.array_equal(b, c) and a.dtype == c.dtype
        off, lids, _ = two
        assert off[-1] == nA + nB and all((np.diff(lids[off[l]:off[l + 1]]) > 0).all() for l in range(nlist))      # ids ascend inside a list
        # ... and both give the same search results
        q = rs.randint(-8, 9, size=(6, M * dsub)).astype(np.float32)
        for metric in ("ip", "l2"):
            v1, i1 = oracle_ivfpq.search(q, R, coarse, pq, *one, k=8, nprobe=min(3, nlist), metric=metric)
            v2, i2 = oracle_ivfpq.search(q, R, coarse, pq, *two, k=8, nprobe=min(3, nlist), metric=metric)
            assert np.array_equal(i1, i2) and np.array_equal(v1, v2)


def test_place_and_merge_edges():
    off = np.array([0, 2, 2, 5], np.int64)                                # list 1 empty on the old side
    asg = np.array([2, 0, 2, 0, 0], np.int64)                             # ... and on the new side
    new_off, dest = ar.place(asg, off)
    assert new_off.tolist() == [0, 5, 5, 10] and dest.tolist() == [8, 2, 9, 3, 4]
    ids_old, codes_old = np.arange(100, 105), np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    ids_new, codes_new = np.arange(200, 205), 255 - np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    dest[4] = 10                                                          # out of range: skipped and counted
    ids, codes, bad = ar.merge(off, ids_old, codes_old, dest, ids_new, codes_new, new_off, fill=7)
    assert bad == 1 and ids.tolist() == [100, 101, 201, 203, 7, 102, 103, 104, 200, 202]
    assert np.array_equal(codes[5:8], codes_old[2:5]) and np.array_equal(codes[8], codes_new[0]) and (codes[4] == 7).all()


def test_encode_bound_covers_the_float32_chain_and_has_teeth():
    rs = np.random.RandomState(3)
    for M, dsub in [(16, 4), (16, 16), (4, 32)]:
        nlist, n = 5, 40
        _, coarse, pq = _index(rs, nlist, M, dsub, integer=False)
        x = (coarse[rs.randint(0, nlist, n)] + 0.7 * rs.randn(n, M * dsub)).astype(np.float32)
        asg = ar.assign(x, coarse)
        norm2 = (pq ** 2).sum(2)
        dist, B = ar.encode(x, asg, coarse, pq, norm2)
        got = ar.encode_emulate(x, asg, coarse, pq, norm2)
        assert ar.encode_excess(got, dist, B) <= 0
        print(f"M={M} dsub={dsub}: {100 * (got == ar.codes_of(dist)).mean():.2f} % of the emulated codes are the float64 argmin")
        assert (B / (np.abs(norm2)[None] + 1e-30)).max() < 1e-3            # a bound, not a licence
        # teeth: the runner-up everywhere is outside the bound almost everywhere
        second = np.argsort(dist, -1)[..., 1].astype(np.uint8)
        assert ar.encode_excess(second, dist, B) > 0


def test_assign_bound_covers_a_float32_pipeline():
    rs = np.random.RandomState(4)
    d, nlist, n = 64, 9, 200
    R, coarse, _ = _index(rs, nlist, 16, 4, integer=False)
    x = rs.randn(n, d).astype(np.float32)
    for cosine, metric in ((True, "ip"), (False, "ip"), (False, "l2")):
        s64, B = ar.assign_bound(x, R, coarse, cosine, metric)
        xn = (x / np.sqrt((x ** 2).sum(1, keepdims=True, dtype=np.float32))).astype(np.float32) if cosine else x
        cs = (xn @ R.T).astype(np.float32) @ coarse.T
        if metric == "l2":
            cs = cs + np.float32(-0.5) * (coarse ** 2).sum(1, dtype=np.float32)[None]
        assert cs.dtype == np.float32 and (np.abs(cs - s64) <= B).all()
        assert B.max() < 1e-3 * np.abs(s64).max()


def test_abi_additions():
    from gnnlm_amd import _lib
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", text) and _lib.ABI_VERSION == 12        # additions only
    syms = _lib.exported_symbols()
    assert "gnnlm_ivfpq_encode_rows" in syms and "gnnlm_ivfpq_list_merge" in syms
    L = _lib.lib()
    for name in ("gnnlm_ivfpq_encode_t", "gnnlm_ivfpq_list_merge_t"):
        assert L.gnnlm_sizeof(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0
    assert [f[0] for f in _lib.STRUCTS["gnnlm_ivfpq_encode_t"]._fields_] == [
        "x", "ldx", "n", "assign", "coarse", "nlist", "pq", "norm2", "M", "dsub", "d", "codes", "ld_codes", "list_cnt", "n_bad"]
    assert [f[0] for f in _lib.STRUCTS["gnnlm_ivfpq_list_merge_t"]._fields_] == [
        "list_off_old", "nlist", "N0", "ids_old", "codes_old", "M", "n", "dest", "ids_new", "codes_new", "ld_new", "new_off", "ids", "codes", "n_bad"]
    assert hasattr(L, "gnnlm_ivfpq_encode_rows") and hasattr(L, "gnnlm_ivfpq_list_merge")
    # refusals are decided on the host, before anything is launched
    e = _lib.gnnlm_ivfpq_encode_t()
    e.M, e.dsub, e.d, e.n = 8, 4, 32, 1
    assert L.gnnlm_ivfpq_encode_rows(ctypes.byref(e), None) == -22 and b"M % 16" in L.gnnlm_last_error()
    assert L.gnnlm_ivfpq_encode_rows(None, None) == -22
    m = _lib.gnnlm_ivfpq_list_merge_t()
    m.M, m.nlist = 24, 1
    assert L.gnnlm_ivfpq_list_merge(ctypes.byref(m), None) == -22
