"""Adding keys to an IVF-PQ index through the Python interface: ``IVFPQIndex.train`` / ``add``, ``attach_vals`` afterwards, an index
read from a faiss file, and ``run_index_build``'s train-once / resume / grow protocol (knn/index_builder.py:66-109).

Integer-valued fixtures (a permutation for R, small integers everywhere: every float32 sum is exact in any order) must give arrays
bit-identical to the float64 restatement tests/ivfpq_add_ref.py, whatever the chunking.  Trained indexes are held to the DERIVED
bounds of the restatement (the list of a key: its float64 coarse score within the float32 bound of the whole pipeline; the codes of
every key: within the encode bound alone, on the rotated rows the library itself produces) and searched against ``oracle.ivfpq.search`` over the index's own arrays with
the bars of tests/test_knn_search_gpu.py: scores within 2e-5, ids identical -- an id may differ from the oracle's only where float32
cannot tell the two apart: both keys score within those 2e-5 of the k-th best (float32 near-ties at the k-th place, as there)."""
import json
import logging
import os

import numpy as np
import pytest
import torch

import ivfpq_add_ref as ref
from oracle import ivfpq as oivf
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

ARRAYS = ("R", "coarse", "pq", "list_off", "list_ids", "list_codes")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def arrays(index):
    return [getattr(index, a).cpu().numpy() for a in ARRAYS]


def lists_of(index):
    """list_off, list_ids, list_codes as numpy"""
    return arrays(index)[3:]


def integer_index(rs, d, M, nlist):
    dsub = d // M
    R = np.eye(d, dtype=np.float32)[rs.permutation(d)]
    coarse = rs.randint(-4, 5, size=(nlist, d)).astype(np.float32)
    pq = rs.randint(-3, 4, size=(M, 256, dsub)).astype(np.float32)
    pq[:, 77] = pq[:, 11]                                                   # exact ties
    return R, coarse, pq


# ======================================================================================================== hand-made index, bit for bit
@pytest.mark.parametrize("d,M", [(64, 16), (256, 64)])
def test_add_to_hand_made_index_bit_for_bit(dev, d, M):
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(d)
    nlist, N0, n = 8, 3000, 1000
    R, coarse, pq = integer_index(rs, d, M, nlist)
    keys = rs.randint(-8, 9, size=(N0 + n, d)).astype(np.float32)
    empty = (np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, M), np.uint8))
    old = ref.add(R, coarse, pq, *empty, keys[:N0], np.arange(N0))
    want = ref.add(R, coarse, pq, *old, keys[N0:], np.arange(N0, N0 + n))
    one_shot = ref.add(R, coarse, pq, *empty, keys, np.arange(N0 + n))
    assert all(np.array_equal(a, b) for a, b in zip(want, one_shot))
    base = IVFPQIndex(*[up(a, dev) for a in (R, coarse, pq) + old], nprobe=3, cosine=False)
    before = lists_of(base)
    for chunk, src in ((1 << 18, keys[N0:]), (1, keys[N0:]), (333, keys[N0:].astype(np.float16)), (1000, torch.from_numpy(keys[N0:]))):
        grown = base.add(src, chunk=chunk)
        assert grown.ntotal == N0 + n and grown.nprobe == 3 and not grown.cosine and grown.route == base.route
        for got, w in zip(lists_of(grown), want):
            assert np.array_equal(got, w), chunk
    assert all(np.array_equal(a, b) for a, b in zip(lists_of(base), before)) and base.ntotal == N0     # the old index is untouched
    # explicit ids, and an empty add
    ids = np.arange(n)[::-1] * 5 + 10 ** 10
    g2 = base.add(keys[N0:], ids=ids, chunk=400)
    w2 = ref.add(R, coarse, pq, *old, keys[N0:], ids)
    assert all(np.array_equal(a, b) for a, b in zip(lists_of(g2), w2))
    g3 = base.add(keys[:0])
    assert all(np.array_equal(a, b) for a, b in zip(lists_of(g3), before))
    with pytest.raises(ValueError):
        base.add(keys[:5, :d - 4])
    with pytest.raises(ValueError):
        base.add(np.full((3, d), np.nan, np.float32))                       # keys without a list


# ======================================================================================================== trained indexes
CONFIGS = [("cosine", 256, 64, "int8", None), ("ip", 128, 32, "packed", None), ("ip", 64, 16, "rowmajor", None), ("l2", 256, 64, "packed", "key_term")]


@pytest.mark.parametrize("metric,d,M,route,term", CONFIGS, ids=[c[0] + "-M" + str(c[2]) for c in CONFIGS])
def test_train_then_add(dev, tmp_path, metric, d, M, route, term):
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(M + len(metric))
    nlist, nA, nB, nprobe = 32, 6000, 2000, 6
    cosine, base_metric = metric == "cosine", "l2" if metric == "l2" else "ip"
    centres = (2.0 if metric == "l2" else 1.0) * rs.randn(50, d).astype(np.float32)
    keys = (centres[rs.randint(0, 50, nA + nB)] + 0.6 * rs.randn(nA + nB, d)).astype(np.float32)
    A, B = keys[:nA], keys[nA:]
    t0 = IVFPQIndex.train(A, nlist, M, device=dev, cosine=cosine, nprobe=nprobe, iters=4, seed=3, metric=base_metric)
    assert t0.ntotal == 0 and t0.max_list == 0 and t0.list_codes.shape == (0, M) and int(t0.list_off.abs().sum()) == 0
    t0.save(str(tmp_path / "trained.npz"))                                   # a trained index saves, loads and adds
    t1 = IVFPQIndex.load(str(tmp_path / "trained.npz"), device=dev)
    assert t1.ntotal == 0 and t1.metric == base_metric and t1.cosine == cosine and t1.nprobe == nprobe
    ia = t1.add(A, chunk=2500)
    ib = ia.add(B.astype(np.float16) if metric != "l2" else B, chunk=1 << 18)
    if metric != "l2":
        keys[nA:] = B.astype(np.float16).astype(np.float32)                  # what the index saw
    assert ia.ntotal == nA and ib.ntotal == nA + nB and ia.route == ib.route == route
    assert (ib.key_term is not None) == (term == "key_term") and (ib.tiles is not None) == (route == "int8")
    R, coarse, pq, off, lids, codes = arrays(ib)
    assert all(np.array_equal(a, b) for a, b in zip(arrays(t0)[:3], (R, coarse, pq)))       # nothing was retrained
    # the lists: offsets, lengths, every id once, ascending inside a list; A's rows did not move relative to each other
    assert off[0] == 0 and off[-1] == nA + nB == len(lids) and (np.diff(off) >= 0).all() and ib.max_list == np.diff(off).max()
    assert np.array_equal(np.sort(lids), np.arange(nA + nB))
    assert all((np.diff(lids[off[l]:off[l + 1]]) > 0).all() for l in range(nlist))
    list_of = np.empty(nA + nB, np.int64)
    list_of[lids] = np.repeat(np.arange(nlist), np.diff(off))
    code_of = np.empty((nA + nB, M), np.uint8)
    code_of[lids] = codes
    offa, lidsa, codesa = lists_of(ia)
    la = np.empty(nA, np.int64)
    la[lidsa] = np.repeat(np.arange(nlist), np.diff(offa))
    ca = np.empty((nA, M), np.uint8)
    ca[lidsa] = codesa
    assert np.array_equal(la, list_of[:nA]) and np.array_equal(ca, code_of[:nA])
    # every key sits in a list whose float64 coarse score is within the float32 bound of the best
    s64, Bs = ref.assign_bound(keys, R, coarse, cosine, base_metric)
    rows, best = np.arange(nA + nB), s64.argmax(1)
    gap = s64[rows, best] - s64[rows, list_of] - (Bs[rows, best] + Bs[rows, list_of])
    print(f"{metric} M={M}: {100 * (best == list_of).mean():.3f} % of the keys in the float64-best list, worst gap over the bound {gap.max():.3e}")
    assert gap.max() <= 0
    # the codes of EVERY key: the encode bound alone, on the float32 rotated rows the library itself makes (the same normalisation and
    # gnnlm_gemm_nt over the same chunks as the two adds above); the float64 tables are [n, M, 256], so in slices of 500 keys
    from gnnlm_amd import ivfpq_train
    srcs = [(A, lo, min(nA, lo + 2500)) for lo in range(0, nA, 2500)] + [(B.astype(np.float16) if metric != "l2" else B, 0, nB)]
    xr = np.concatenate([ivfpq_train.rotated_rows(src, lo, hi, ib.R, cosine).cpu().numpy() for src, lo, hi in srcs])
    norm2 = (up(pq, dev) ** 2).sum(2).cpu().numpy()                          # (as add_rows computes it)
    excess, exact = -np.inf, 0
    for lo in range(0, nA + nB, 500):
        dist, Bd = ref.encode(xr[lo:lo + 500], list_of[lo:lo + 500], coarse, pq, norm2)
        excess = max(excess, ref.encode_excess(code_of[lo:lo + 500], dist, Bd))
        exact += int((code_of[lo:lo + 500] == ref.codes_of(dist)).sum())
    print(f"{metric} M={M}: {100 * exact / code_of.size:.3f} % float64 argmins, worst excess over the bound {excess:.3e}")
    assert excess <= 0
    # the search over the grown index against the oracle over the same arrays
    q = (centres[rs.randint(0, 50, 64)] + 0.6 * rs.randn(64, d)).astype(np.float32)
    if cosine:
        q = q / np.sqrt((q ** 2).sum(1, keepdims=True))
    for k in (8, 100):
        v, i = ib.search(q, k)
        v_ref, i_ref = oivf.search(q, R, coarse, pq, off, lids, codes, k=k, nprobe=nprobe, metric=base_metric)
        assert (i >= 0).all() and (i_ref >= 0).all()
        np.testing.assert_allclose(v, v_ref, rtol=2e-5, atol=2e-5)
        if not np.array_equal(np.sort(i, 1), np.sort(i_ref, 1)):            # a float32 near-tie at the k-th place: both keys within 2e-5 of it
            v_all, i_all = oivf.search(q, R, coarse, pq, off, lids, codes, k=k + 8, nprobe=nprobe, metric=base_metric)
            for r in range(len(q)):
                for x in set(i[r].tolist()) ^ set(i_ref[r].tolist()):
                    at = np.nonzero(i_all[r] == x)[0]
                    assert len(at) == 1 and abs(v_all[r, at[0]] - v_ref[r, k - 1]) <= 2e-5 * (1 + abs(v_ref[r, k - 1])), (k, r, x)


def test_attach_vals_after_add(dev):
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(5)
    d, M, nlist, nA, nB, V = 256, 64, 16, 3000, 1500, 300
    centres = rs.randn(30, d).astype(np.float32)
    keys = (centres[rs.randint(0, 30, nA + nB)] + 0.6 * rs.randn(nA + nB, d)).astype(np.float32)
    vals = rs.randint(0, V, nA + nB).astype(np.int32)
    a = IVFPQIndex.train(keys[:nA], nlist, M, device=dev, cosine=True, nprobe=4, iters=3).add(keys[:nA]).attach_vals(up(vals[:nA], dev))
    b = a.add(keys[nA:])
    assert a.has_vals and not b.has_vals                                    # labels are not carried over
    b.attach_vals(up(vals, dev))
    q = keys[rs.randint(0, nA + nB, 40)]
    q = q / np.sqrt((q ** 2).sum(1, keepdims=True))
    v, i, lab = b.search_device(up(q, dev), 16, return_vals=True)
    i, lab = i.cpu().numpy(), lab.cpu().numpy()
    assert (i >= 0).all() and (i >= nA).any() and np.array_equal(lab, vals[i])


def test_add_to_index_from_faiss_file(dev, tmp_path):
    from gnnlm_amd import faiss_io
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(6)
    d, M, nlist, nA, nB = 128, 32, 24, 4000, 500
    centres = rs.randn(30, d).astype(np.float32)
    keys = (centres[rs.randint(0, 30, nA + nB)] + 0.5 * rs.randn(nA + nB, d)).astype(np.float32)
    built = IVFPQIndex.build(keys[:nA], nlist, M, device=dev, cosine=True, nprobe=1, iters=4, seed=2)
    f = str(tmp_path / "faiss_store.cosine")
    faiss_io.write_ivfpq_index(f, *arrays(built), nprobe=1)
    idx = IVFPQIndex.from_faiss_file(f, device=dev, cosine=True, nprobe=1)
    assert idx.ntotal == nA
    grown = idx.add(keys[nA:])
    off, lids, codes = lists_of(grown)
    assert grown.ntotal == nA + nB and np.array_equal(np.sort(lids)[nA:], np.arange(nA, nA + nB))     # new ids start at ntotal
    o0, l0, c0 = lists_of(idx)
    for l in range(nlist):                                                   # behind the old rows of their lists
        assert np.array_equal(lids[off[l]:off[l] + o0[l + 1] - o0[l]], l0[o0[l]:o0[l + 1]])
    # a key of B as a query: the one list the search probes is the list the key was filed in (the same arithmetic), so with every
    # member of that list returned the key's own id is among them
    qB = keys[nA:] / np.sqrt((keys[nA:] ** 2).sum(1, keepdims=True))
    k = int(np.diff(off).max())
    _, i = grown.search(qB, k)
    assert all((nA + r) in i[r] for r in range(nB))


# ======================================================================================================== run_index_build
def _write_dstore(dd, keys, vals, V):
    os.makedirs(dd, exist_ok=True)
    keys.astype(np.float16).tofile(dd / "keys.npy")
    vals.astype(np.int16).tofile(dd / "vals.npy")
    json.dump({"dstore_size": len(keys), "hidden_size": keys.shape[1], "vocab_size": V, "dstore_fp16": True, "val_size": 1}, open(dd / "info.json", "w"))


def _build(dd, *extra):
    from gnnlm_amd import run_index_build
    return run_index_build.main(run_index_build.get_parser().parse_args(
        ["--dstore-dir", str(dd), "--index-type", "IVF32,PQ16", "--metric", "cosine", "--nprobe", "8"] + list(extra)))


def _npz(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


def test_run_index_build_trains_once_resumes_and_grows(dev, tmp_path, caplog):
    from gnnlm_amd.ivfpq import IVFPQIndex
    from gnnlm_amd.knn_model import KNNModel
    rs = np.random.RandomState(8)
    d, V, N1, N2 = 64, 50, 4000, 5000
    centres = rs.randn(40, d).astype(np.float32)
    keys = (centres[rs.randint(0, 40, N2)] + 0.5 * rs.randn(N2, d)).astype(np.float16)
    vals = rs.randint(0, V, N2)
    dd = tmp_path / "train_dstore"
    _write_dstore(dd, keys[:N1], vals[:N1], V)
    out = _build(dd)
    trained = str(dd / "faiss_store.trained.cosine.gnnlm.npz")
    assert out == str(dd / "faiss_store.cosine.gnnlm.npz") and os.path.exists(out) and os.path.exists(trained)
    t0, f0 = _npz(trained), _npz(out)
    assert t0["list_ids"].shape == (0,) and t0["list_off"][-1] == 0 and f0["list_off"][-1] == N1
    stamp = (os.stat(out).st_mtime_ns, os.stat(trained).st_mtime_ns)
    assert _build(dd) == out and (os.stat(out).st_mtime_ns, os.stat(trained).st_mtime_ns) == stamp       # nothing to do: nothing rewritten
    # the datastore grows: only the new rows are added, nothing is retrained
    _write_dstore(dd, keys, vals, V)
    with caplog.at_level(logging.WARNING, logger="gnnlm_amd.knn_model"):
        KNNModel(str(dd / "faiss_store.cosine"), str(dd), k=16, probe=8, no_load_keys=True, metric_type="do_not_recomp_ip", device=dev)
    assert any("4000" in r.getMessage() and "5000" in r.getMessage() for r in caplog.records)          # the stale index is named
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="gnnlm_amd.run_index_build"):
        assert _build(dd, "--index-type", "IVF16,PQ16") == out              # the file on disk wins over other flags, and says so
    assert any("32 lists" in r.getMessage() and "16 lists" in r.getMessage() for r in caplog.records)
    caplog.clear()
    f1 = _npz(out)
    assert f1["list_off"][-1] == N2 and os.stat(trained).st_mtime_ns == stamp[1]
    assert all(np.array_equal(f1[k], t0[k]) for k in ("R", "coarse", "pq", "meta"))
    where = lambda f: (np.repeat(np.arange(len(f["list_off"]) - 1), np.diff(f["list_off"]))[np.argsort(f["list_ids"])], f["list_codes"][np.argsort(f["list_ids"])])
    (l0, c0), (l1, c1) = where(f0), where(f1)
    assert np.array_equal(l1[:N1], l0) and np.array_equal(c1[:N1], c0)      # the first 4000 ids keep their lists and codes
    # the grown index behind KNNModel: no warning, and get_knn_prob against the oracle path of tests/test_knn_search_gpu.py
    with caplog.at_level(logging.WARNING, logger="gnnlm_amd.knn_model"):
        m = KNNModel(str(dd / "faiss_store.cosine"), str(dd), k=64, probe=8, no_load_keys=True, metric_type="do_not_recomp_ip", device=dev)
    assert not any("rerun" in r.getMessage() for r in caplog.records)
    assert isinstance(m.index, IVFPQIndex) and m.index.ntotal == N2 and m.index.has_vals
    n = 33
    q = (centres[rs.randint(0, 40, n)] + 0.5 * rs.randn(n, d)).astype(np.float32)
    targets = rs.randint(0, V, n).astype(np.int64)
    p, rec = m.get_knn_prob(torch.from_numpy(q).to(dev), targets=torch.from_numpy(targets).to(dev), t=1.0, return_recall=True)
    v_ref, i_ref = oivf.search(q, *arrays(m.index), k=64, nprobe=8, cosine_queries=True)
    p_ref, rec_ref = oknn.knn_target_prob(v_ref.astype(np.float32), i_ref, vals.astype(np.int16), targets, 1.0)
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.numpy(), rtol=2e-4, atol=1e-6)
    assert np.abs(rec.cpu().numpy() - rec_ref.numpy()).max() <= 1
    # a datastore smaller than the index is refused; --overwrite retrains
    _write_dstore(dd, keys[:N1], vals[:N1], V)
    with pytest.raises(ValueError, match="5000.*4000"):
        _build(dd)
    assert _build(dd, "--overwrite", "--seed", "1") == out
    t2, f2 = _npz(trained), _npz(out)
    assert f2["list_off"][-1] == N1 and not np.array_equal(t2["coarse"], t0["coarse"]) and np.array_equal(f2["coarse"], t2["coarse"])


def test_run_index_build_integer_fixture_resume_equals_one_shot(dev, tmp_path):
    """a hand-written trained file (a permutation and small integers: exact arithmetic) -> grown in two runs, resumed with
    --save-every 1, and built in one shot: the same arrays, and the float64 restatement's"""
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(9)
    d, M, nlist, V = 64, 16, 8, 20
    R, coarse, pq = integer_index(rs, d, M, nlist)
    keys = rs.randint(-8, 9, size=(5000, d)).astype(np.float32)
    vals = rs.randint(0, V, 5000)
    empty = (np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, M), np.uint8))
    want = ref.add(R, coarse, pq, *empty, keys, np.arange(5000))
    finals = []
    for name, sizes, extra in (("grown", (4000, 5000), ()), ("resumed", (2000, 5000), ("--save-every", "1", "--chunk-size", "1000")), ("one_shot", (5000,), ())):
        dd = tmp_path / name
        os.makedirs(dd)
        IVFPQIndex(*[up(a, dev) for a in (R, coarse, pq) + empty], nprobe=8, cosine=False).save(str(dd / "faiss_store.trained.ip.gnnlm.npz"))
        for size in sizes:
            _write_dstore(dd, keys[:size], vals[:size], V)
            from gnnlm_amd import run_index_build
            out = run_index_build.main(run_index_build.get_parser().parse_args(
                ["--dstore-dir", str(dd), "--index-type", "IVF8,PQ16", "--metric", "ip"] + list(extra)))
            assert np.load(out)["list_off"][-1] == size
        finals.append(_npz(out))
    for f in finals:
        assert np.array_equal(f["R"], R) and np.array_equal(f["coarse"], coarse) and np.array_equal(f["pq"], pq)
        for k, w in zip(("list_off", "list_ids", "list_codes"), want):
            assert np.array_equal(f[k], w) and f[k].dtype == w.dtype, k
