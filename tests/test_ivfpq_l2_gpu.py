"""The L2 IVF-PQ search with one term per key: `gnnlm_ivfpq_key_terms`, the packed float32 scan at M = 64, the
row-major scan for indexes whose per-list table would not fit, and the entries above them (`KNNModel`, `GnnLmEngine.score`) --
against the float64 IVFADC oracle (oracle/ivfpq.py) over the same index arrays, with the project's L2 bars
(`rtol = atol = 2e-4` on squared distances, mean id overlap > 0.998: those of test_ivfpq_l2_index)."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ivfpq as oivf
from oracle import knn as oknn

ARRAYS = ("R", "coarse", "pq", "list_off", "list_ids", "list_codes")
BAR = dict(rtol=2e-4, atol=2e-4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to_dev(arrs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrs]


def check_against_oracle(dist, ids, d_ref, i_ref, k):
    assert (dist[:, 1:] >= dist[:, :-1]).all()                               # ascending squared distances (+inf padding last)
    assert np.array_equal(ids == -1, i_ref == -1)                            # the same padding: every key of the probed lists is there
    # (overlap among the keys there are: len(set & set) / k of a full row; a padded row is not credited with its -1 entries)
    assert np.mean([len((set(a) & set(b)) - {-1}) / max(1, int((b >= 0).sum())) for a, b in zip(ids, i_ref)]) > 0.998
    np.testing.assert_allclose(dist, d_ref, **BAR)


def random_index_arrays(rs, sizes, M, dsub):
    """Index arrays made by hand: lists of the given lengths (zeros allowed), random centroids, codes and a permutation as ids."""
    nlist, N, d = len(sizes), int(np.sum(sizes)), M * dsub
    R = np.linalg.qr(rs.randn(d, d))[0].astype(np.float32)
    coarse = rs.randn(nlist, d).astype(np.float32)
    pq = (0.3 * rs.randn(M, 256, dsub)).astype(np.float32)
    off = np.zeros(nlist + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    return [R, coarse, pq, off, rs.permutation(N).astype(np.int64) + 11, rs.randint(0, 256, (N, M)).astype(np.uint8)]


# ----------------------------------------------------------------------------------------------------- 2. key terms
@pytest.mark.parametrize("M,dsub", [(16, 4), (32, 8), (64, 4)])
def test_key_terms(dev, M, dsub):
    """key_term[r] = sum_m (|p_m,c|^2 + 2 <c_l,m, p_m,c>) within one float32 ulp of the float64 value; 37 lists, empty ones at the
    front, in the middle and at the end, one list of a single row."""
    from gnnlm_amd import ops
    rs = np.random.RandomState(100 + M)
    N, nlist = 5000, 37
    sizes = rs.multinomial(N - 1, np.ones(nlist - 4) / (nlist - 4))
    sizes = np.concatenate([[0], sizes[:10], [0], sizes[10:20], [1], sizes[20:], [0]])     # empty: first, 12th, last
    assert len(sizes) == nlist and sizes.sum() == N and (sizes == 0).sum() >= 2 and (sizes == 1).sum() >= 1
    _, coarse, pq, off, _, codes = random_index_arrays(rs, sizes, M, dsub)
    got = ops.ivfpq_key_terms(*to_dev((codes, off, coarse, pq), dev)).cpu().numpy()
    lists = np.searchsorted(off, np.arange(N), side="right") - 1
    p = pq.astype(np.float64)[np.arange(M)[None, :], codes.astype(np.int64)]              # [N, M, dsub]
    c = coarse.astype(np.float64)[lists].reshape(N, M, dsub)
    ref = ((p ** 2).sum(2) + 2.0 * (c * p).sum(2)).sum(1)
    ref32 = ref.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (N,)
    assert (np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= np.spacing(np.abs(ref32)).astype(np.float64)).all()
    # the identity the search rests on: key_term = |c_l + r|^2 - |c_l|^2 of the reconstruction
    rec = c + p
    np.testing.assert_allclose(ref, (rec ** 2).sum((1, 2)) - (c ** 2).sum((1, 2)), rtol=1e-9, atol=1e-9)


# ----------------------------------------------------------------------------------------------------- 3 / 4 / 7. M = 64
@pytest.fixture(scope="module")
def l2_m64(dev):
    """test_ivfpq_l2_index's data family at d = 256, M = 64: the built index, its arrays, the queries and the oracle's answers."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(31)
    N, d, M, nlist = 40_000, 256, 64, 40
    centres = 2.0 * rs.randn(25, d).astype(np.float32)
    keys = (centres[rs.randint(0, 25, N)] + 0.7 * rs.randn(N, d)).astype(np.float32)
    q = (centres[rs.randint(0, 25, 33)] + 0.7 * rs.randn(33, d)).astype(np.float32)
    idx = IVFPQIndex.build(keys, nlist, M, device=dev, cosine=False, metric="l2", nprobe=8, iters=6, seed=4)
    arrs = [getattr(idx, a).cpu().numpy() for a in ARRAYS]
    ref = {k: oivf.search(q, *arrs, k=k, nprobe=8, metric="l2") for k in (1024, 64)}
    return dict(idx=idx, arrs=arrs, q=q, keys=keys, ref=ref, rs=rs)


def test_m64_route_against_oracle(dev, l2_m64):
    from gnnlm_amd.ivfpq import IVFPQIndex
    idx, q = l2_m64["idx"], l2_m64["q"]
    assert idx.metric == "l2" and idx.tiles is None
    assert idx.packed_codes is not None and idx.list_term is None and idx.key_term is not None
    assert idx.key_term.shape == (idx.ntotal,) and idx.key_term.dtype == torch.float32
    for k in (1024, 64):
        dist, ids = idx.search(q, k)
        check_against_oracle(dist, ids, *l2_m64["ref"][k], k)
    small = IVFPQIndex(*[getattr(idx, a) for a in ARRAYS], nprobe=1, cosine=False, metric="l2")
    assert small.packed_codes is not None and small.key_term is not None
    dist, ids = small.search(q[:4], 2000)                                     # fewer keys than k in the probed list: +inf / -1 padding
    _, i_ref = oivf.search(q[:4], *l2_m64["arrs"], k=2000, nprobe=1, metric="l2")
    pad = ids == -1
    assert pad.any() and np.array_equal(pad, i_ref == -1) and np.isinf(dist[pad]).all() and (dist[pad] > 0).all() and np.isfinite(dist[~pad]).all()
    if small.max_list < 2000:                                                 # (every list is shorter than k: the last column is padding)
        assert (ids[:, -1] == -1).all() and np.isinf(dist[:, -1]).all() and (dist[:, -1] > 0).all()


def test_thresholded_round_loses_nothing(dev, l2_m64):
    """Two lists scored in full + the rest above the threshold == every probed list scored in full."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    idx, q = l2_m64["idx"], l2_m64["q"]
    assert idx.dense_probes == 2
    full = IVFPQIndex(*[getattr(idx, a) for a in ARRAYS], nprobe=8, cosine=False, metric="l2", dense_probes=8)
    qd = torch.from_numpy(q).to(dev)
    for k in (1024, 64):
        d2, i2 = idx.search_device(qd, k)
        assert idx.stats["candidates"] > 0                                    # the thresholded round ran and let keys through
        d8, i8 = full.search_device(qd, k)
        assert torch.equal(d2, d8)
        assert all(set(a) == set(b) for a, b in zip(i2.cpu().numpy().tolist(), i8.cpu().numpy().tolist()))


def test_mirrors(dev, l2_m64, tmp_path):
    """The faiss file of the M = 64 index -> KNNModel(metric_type="do_not_recomp_l2"): sims = -distances, the kNN probability."""
    from gnnlm_amd import faiss_io
    from gnnlm_amd.ivfpq import IVFPQIndex
    from gnnlm_amd.knn_model import KNNModel
    arrs, q, keys = l2_m64["arrs"], l2_m64["q"], l2_m64["keys"]
    N, d, V = keys.shape[0], keys.shape[1], 50
    vals = np.random.RandomState(5).randint(0, V, N).astype(np.int16)
    dd = tmp_path / "train_dstore"
    os.makedirs(dd)
    keys.astype(np.float16).tofile(dd / "keys.npy"); vals.tofile(dd / "vals.npy")
    json.dump({"dstore_size": N, "hidden_size": d, "vocab_size": V, "dstore_fp16": True, "val_size": 1}, open(dd / "info.json", "w"))
    f = str(dd / "faiss_store.l2")
    faiss_io.write_ivfpq_index(f, *arrs, nprobe=1, metric="l2")
    m = KNNModel(f, str(dd), k=64, probe=8, no_load_keys=True, metric_type="do_not_recomp_l2", device=dev)
    assert isinstance(m.index, IVFPQIndex) and m.index.metric == "l2" and not m.cosine and m.index.has_vals
    assert m.index.packed_codes is not None and m.index.key_term is not None and m.index.list_term is None
    d_ref, i_ref = l2_m64["ref"][64]
    sims, knns = m.search_sims(torch.from_numpy(q).to(dev), 64)
    assert np.mean([len(set(a) & set(b)) / 64 for a, b in zip(knns.cpu().numpy(), i_ref)]) > 0.998
    np.testing.assert_allclose(sims.cpu().numpy(), -d_ref, **BAR)                  # knn_model.py:153-154: sims = -dists
    targets = torch.from_numpy(vals[i_ref[:, 1]].astype(np.int64)).to(dev)
    p, rec = m.get_knn_prob(torch.from_numpy(q).to(dev), targets=targets, t=10.0, return_recall=True)
    p_ref, rec_ref = oknn.knn_target_prob((-d_ref).astype(np.float32), i_ref, vals, targets.cpu().numpy(), 10.0)
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.numpy(), rtol=2e-3, atol=1e-6)
    assert np.abs(rec.cpu().numpy() - rec_ref.numpy()).max() <= 1


# ----------------------------------------------------------------------------------------------------- 5. packed-kernel edges
@pytest.mark.parametrize("dense", [1, 2, 3])
def test_packed_kernel_edges(dev, dense):
    """Lists of 0, 1, 63, 64, 65, 129, 0, 7 rows: lists that start and end inside a 64-row block, a last partial block, empty lists;
    5 queries probing every list: 5 * dense and 5 * (8 - dense) tasks per round (odd for dense 1 and 3: the last workgroup has one
    task), pairs of tasks inside one list and across a list boundary.  Against the oracle, then against the per-list-table route."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(77)
    sizes = [0, 1, 63, 64, 65, 129, 0, 7]
    arrs = random_index_arrays(rs, sizes, 64, 4)
    N = int(np.sum(sizes))
    q = rs.randn(5, 256).astype(np.float32)
    t = to_dev(arrs, dev)
    new = IVFPQIndex(*t, nprobe=8, cosine=False, metric="l2", dense_probes=dense)
    old = IVFPQIndex(*t, nprobe=8, cosine=False, metric="l2", dense_probes=dense, scan="rowmajor")
    assert new.packed_codes is not None and new.key_term is not None and new.list_term is None
    assert old.packed_codes is None and old.key_term is None and old.list_term is not None
    for k in (16, N + 30):
        dist, ids = new.search(q, k)
        d_ref, i_ref = oivf.search(q, *arrs, k=k, nprobe=8, metric="l2")
        check_against_oracle(dist, ids, d_ref, i_ref, k)
        assert (ids[:, min(k, N):] == -1).all() and np.isinf(dist[:, min(k, N):]).all()
        # the route of the per-list table: the same neighbours (as sets: two keys whose distances differ by less than the bar may
        # swap places between two summation orders) at distances within the bar of each other
        d_old, i_old = old.search(q, k)
        assert all(set(a) == set(b) for a, b in zip(ids.tolist(), i_old.tolist()))
        np.testing.assert_allclose(dist, d_old, **BAR)


# ----------------------------------------------------------------------------------------------------- 6. any list count
@pytest.mark.parametrize("M,dsub", [(32, 4), (16, 4)])
def test_no_limit_on_list_count(dev, M, dsub):
    """An index whose [nlist, M, 256] table is over the budget (here: a budget of 0) is searched on row-major codes with key_term;
    2000 lists over 20 000 keys, most of them short and many empty."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(200 + M)
    nlist, N = 2000, 20_000
    w = rs.exponential(1.0, nlist) * (rs.random_sample(nlist) < 0.6)                  # ~40 % of the lists empty
    sizes = rs.multinomial(N, w / w.sum())
    assert (sizes == 0).sum() > 500
    arrs = random_index_arrays(rs, sizes, M, dsub)
    q = rs.randn(21, M * dsub).astype(np.float32)
    idx = IVFPQIndex(*to_dev(arrs, dev), nprobe=32, cosine=False, metric="l2", list_term_bytes=0)
    assert idx.list_term is None and idx.key_term is not None and idx.packed_codes is None and idx.tiles is None
    dist, ids = idx.search(q, 256)
    d_ref, i_ref = oivf.search(q, *arrs, k=256, nprobe=32, metric="l2")
    check_against_oracle(dist, ids, d_ref, i_ref, 256)


# ----------------------------------------------------------------------------------------------------- 8. the engine
def test_engine_l2_index(dev):
    """GnnLmEngine.score with an L2 index inside the step: the raw gcn_feat rows are the queries, sims = -distances."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=1, k=64, seed=1)
    eng, b = build_engine(prob, dev), to_batch(prob["block"], dev)
    x = eng.score(b)["gcn_feat"]
    rs = np.random.RandomState(9)
    scale = float(x.abs().mean().item())                                       # keys of the queries' own size: neighbours at mixed distances
    keys = (scale * rs.randn(3000, 64)).astype(np.float32)
    l2 = IVFPQIndex.build(keys, 8, 16, device=dev, cosine=False, metric="l2", nprobe=4, iters=4, seed=2, list_term_bytes=0)
    l2.attach_vals(eng.store.vals)
    ip = IVFPQIndex.build(keys, 8, 16, device=dev, cosine=False, metric="ip", nprobe=4, iters=4, seed=2).attach_vals(eng.store.vals)
    assert l2.key_term is not None and not l2.cosine and not ip.cosine and ip.metric == "ip"

    out = eng.score(b, 0.25, 1.0, knn_index=l2, k=64, knn_sim_func="do_not_recomp_l2")
    x = out["gcn_feat"]
    dist, ids, vals = l2.search_device(x.contiguous(), 64, return_vals=True)       # the UN-normalised features
    assert torch.equal(out["knn_ids"], ids) and torch.equal(out["knn_sims"], -dist)
    given = dataclasses.replace(b, knn_sims=(-dist).contiguous(), knn_ids=ids.contiguous(), knn_vals=vals.contiguous())
    want = eng.score(given, 0.25, 1.0)
    assert float((out["logp"] - want["logp"]).abs().max()) <= 2e-5
    assert not torch.equal(out["logp"], out["lm_logp"])                         # the neighbours are in the result
    xn = x / (x ** 2).sum(-1, keepdim=True).sqrt()
    assert not torch.equal(l2.search_device(xn.contiguous(), 64)[1], ids)       # (normalised queries find other neighbours here)

    for fn, index in (("do_not_recomp_l2", ip), ("do_not_recomp_ip", l2)):
        with pytest.raises(ValueError) as err:
            eng.score(b, 0.25, 1.0, knn_index=index, k=64, knn_sim_func=fn)
        assert "do_not_recomp_ip" in str(err.value) and "do_not_recomp_l2" in str(err.value)   # the message names both

    # an inner-product index that is not a cosine one: searched with the raw features too
    out = eng.score(b, 0.25, 1.0, knn_index=ip, k=64)
    s_raw, i_raw, _ = ip.search_device(x.contiguous(), 64, return_vals=True)
    assert torch.equal(out["knn_ids"], i_raw) and torch.equal(out["knn_sims"], s_raw)
    assert not torch.equal(ip.search_device(xn.contiguous(), 64)[0], s_raw)
