"""The fused coarse step (``ops.ivfpq_coarse_probes``) through the Python interface: the search with ``coarse_route`` forced both
ways (inner product and L2: the col_bias path), ``add`` on both sides of the threshold, the k-means assignment, and the producer of
the One Billion Word recipe's index family -- a REDUCING rotation from ``IVFPQIndex.train(d_out=...)`` and from
``run_index_build --index-type OPQ16_64,...``.

Integer-grid fixtures (a selection matrix for R, small integers everywhere: every float32 sum is exact in any order) must give the
same probes and bit-equal results on both routes.  Gaussian fixtures are held to ``oracle.ivfpq.search`` over the index's own arrays
with the bars of tests/test_knn_search_gpu.py::test_ivfpq_one_billion_index_family (scores rtol 2e-5 / atol 2e-4, the same number of
neighbours, more than 99.8 % of the ids)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ivfpq as oivf

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 2e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def arrays_of(index):
    return [t.cpu().numpy() for t in (index.R, index.coarse, index.pq, index.list_off, index.list_ids, index.list_codes)]


def with_route(index, route, **kw):
    """the same arrays behind the other coarse route"""
    from gnnlm_amd.ivfpq import IVFPQIndex
    ix = IVFPQIndex(index.R, index.coarse, index.pq, index.list_off, index.list_ids, index.list_codes, nprobe=index.nprobe,
                    cosine=index.cosine, metric=index.metric, coarse_route=route, **kw)
    assert ix.coarse_route == route and ix.route in ("packed", "rowmajor")
    return ix


def probes_of(index, q, k):
    from gnnlm_amd.ivfpq import _LazyStats
    blk = index._block_begin(index._plan(k, index.dense_probes, index.cand_cap), q, _LazyStats())
    assert (blk.cs is None) == (index.coarse_route == "fused")             # no [queries, nlist] tensor on the fused route
    return blk.pv.cpu().numpy(), blk.pi.cpu().numpy()


def integer_family(rs, d_in, d_out, M, nlist, N):
    """R selects every (d_in / d_out)-th dimension; centroids, product quantizer and clustered keys on the integer grid"""
    R = np.zeros((d_out, d_in), np.float32)
    R[np.arange(d_out), np.arange(d_out) * (d_in // d_out)] = 1.0
    coarse = rs.randint(-4, 5, size=(nlist, d_out)).astype(np.float32)
    pq = rs.randint(-2, 3, size=(M, 256, d_out // M)).astype(np.float32)
    keys = rs.randint(-1, 2, size=(N, d_in)).astype(np.float32)
    keys[:, ::d_in // d_out] += coarse[rs.randint(0, nlist, N)]
    return R, coarse, pq, keys


def against_oracle(index, q, k, metric="ip"):
    v, i = index.search(q, k)
    v_ref, i_ref = oivf.search(q, *arrays_of(index), k=k, nprobe=index.nprobe, metric=metric)
    ok = i_ref >= 0
    assert np.array_equal(i >= 0, ok)
    same = np.mean([len(set(a[a >= 0]) & set(b[b >= 0])) / max(1, (b >= 0).sum()) for a, b in zip(i, i_ref)])
    assert same > 0.998, same
    np.testing.assert_allclose(v[ok], v_ref[ok], rtol=RTOL, atol=ATOL)


# ============================================================================================= the one-billion family, forced routes
@pytest.fixture(scope="module")
def family_keys():
    rs = np.random.RandomState(31)
    N, d_in = 200_000, 256
    centres = rs.randn(300, d_in).astype(np.float32)
    keys = centres[rs.randint(0, 300, N)] + 0.5 * rs.randn(N, d_in).astype(np.float32)
    q = (centres[rs.randint(0, 300, 40)] + 0.5 * rs.randn(40, d_in)).astype(np.float32)
    return keys, q


def test_one_billion_family_gaussian_both_routes_against_the_oracle(dev, family_keys, monkeypatch):
    """d_in 256 -> d_out 64, M 16, 20,000 lists; with the threshold below them k-means, add and search all take the fused step"""
    from gnnlm_amd import ivfpq_train
    from gnnlm_amd.ivfpq import IVFPQIndex
    keys, q = family_keys
    monkeypatch.setattr(ivfpq_train, "COARSE_FUSED_MIN_LISTS", 16384)
    index = IVFPQIndex.build(keys, 20_000, 16, device=dev, cosine=False, nprobe=32, iters=3, seed=2, train_size=100_000, d_out=64)
    assert index.R.shape == (64, 256) and index.coarse.shape == (20_000, 64) and index.pq.shape == (16, 256, 4)
    assert index.coarse_route == "fused" and index.ntotal == len(keys)
    RRt = (index.R.double() @ index.R.double().t()).cpu().numpy()
    assert np.abs(RRt - np.eye(64)).max() < 1e-5
    against_oracle(index, q, 128)
    against_oracle(with_route(index, "dense"), q, 128)


def test_one_billion_family_integer_grid_routes_agree_bit_for_bit(dev, monkeypatch):
    from gnnlm_amd import ivfpq_train
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(5)
    d_in, d_out, M, nlist, N, k = 256, 64, 16, 20_000, 200_000, 64
    R, coarse, pq, keys = integer_family(rs, d_in, d_out, M, nlist, N)
    tR, tc, tp = up(R, dev), up(coarse, dev), up(pq, dev)
    ids = torch.arange(N, dtype=torch.int64, device=dev)
    built = {}
    for name, thr in (("fused", 1), ("dense", 10 ** 9)):                      # `add` on both sides of the threshold
        monkeypatch.setattr(ivfpq_train, "COARSE_FUSED_MIN_LISTS", thr)
        assert ivfpq_train.coarse_fused(nlist, d_out) == (name == "fused")
        built[name] = ivfpq_train.add_rows(tR, tc, tp, *ivfpq_train.empty_lists(nlist, M, dev), keys, ids, cosine=False, chunk=70_000)
    for a, b in zip(built["fused"], built["dense"]):
        assert torch.equal(a, b)                                            # list_off, list_ids, list_codes
    assert int(built["fused"][0][-1]) == N
    monkeypatch.undo()
    q = up(keys[rs.randint(0, N, 100)] + rs.randint(-1, 2, size=(100, d_in)).astype(np.float32), dev)
    out = {}
    for route in ("fused", "dense"):
        ix = IVFPQIndex(tR, tc, tp, *built["fused"], nprobe=32, cosine=False, coarse_route=route)
        assert ix.coarse_route == route
        out[route] = probes_of(ix, q, k) + tuple(t.cpu().numpy() for t in ix.search_device(q, k))
    for a, b in zip(out["fused"], out["dense"]):
        assert np.array_equal(a, b) and (a + 0).tobytes() == (b + 0).tobytes()   # probe values, probe ids, scores, ids (a zero of either sign)


# ============================================================================================= L2: the col_bias path
def test_l2_index_routes_agree_and_match_the_oracle(dev):
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(6)
    d, M, nlist, N, k = 64, 16, 3000, 40_000, 32
    R, coarse, pq, keys = integer_family(rs, d, d, M, nlist, N)
    base = IVFPQIndex(up(R, dev), up(coarse, dev), up(pq, dev), *[t for t in _lists(dev, R, coarse, pq, keys, "l2")], nprobe=16,
                      cosine=False, metric="l2")
    assert base.coarse_route == "dense"                                     # 3000 lists: below the threshold
    q = up(keys[rs.randint(0, N, 64)] + rs.randint(-1, 2, size=(64, d)).astype(np.float32), dev)
    out = {}
    for route in ("fused", "dense"):
        ix = with_route(base, route)
        out[route] = probes_of(ix, q, k) + tuple(t.cpu().numpy() for t in ix.search_device(q, k))
    for a, b in zip(out["fused"], out["dense"]):
        assert np.array_equal(a, b) and (a + 0).tobytes() == (b + 0).tobytes()
    assert (out["fused"][1] >= 0).all()
    # Gaussian keys: both routes against the float64 distances
    centres = rs.randn(100, d).astype(np.float32)
    gk = (centres[rs.randint(0, 100, N)] + 0.4 * rs.randn(N, d)).astype(np.float32)
    gq = (centres[rs.randint(0, 100, 30)] + 0.4 * rs.randn(30, d)).astype(np.float32)
    g = IVFPQIndex.build(gk, 1024, M, device=dev, cosine=False, nprobe=16, iters=3, seed=1, metric="l2")
    for route in ("fused", "dense"):
        against_oracle(with_route(g, route), gq, k, metric="l2")


def _lists(dev, R, coarse, pq, keys, metric):
    from gnnlm_amd import ivfpq_train
    ids = torch.arange(len(keys), dtype=torch.int64, device=dev)
    return ivfpq_train.add_rows(up(R, dev), up(coarse, dev), up(pq, dev), *ivfpq_train.empty_lists(len(coarse), pq.shape[0], dev), keys, ids,
                                cosine=False, metric=metric)


# ============================================================================================= training a reducing rotation
def test_train_with_a_reducing_rotation_then_add_and_search(dev, family_keys):
    from gnnlm_amd.ivfpq import IVFPQIndex
    keys, q = family_keys
    keys = keys[:30_000]
    trained = IVFPQIndex.train(keys, 256, 16, device=dev, cosine=False, nprobe=16, iters=3, seed=3, train_size=20_000, d_out=64, opq_iters=2)
    assert trained.R.shape == (64, 256) and trained.coarse.shape == (256, 64) and trained.pq.shape == (16, 256, 4) and trained.ntotal == 0
    RRt = (trained.R.double() @ trained.R.double().t()).cpu().numpy()
    assert np.abs(RRt - np.eye(64)).max() < 1e-5
    index = trained.add(keys)
    assert index.ntotal == len(keys) and index.R.shape == (64, 256)
    against_oracle(index, q, 64)
    with pytest.raises(AssertionError):
        IVFPQIndex.train(keys, 256, 16, device=dev, cosine=False, d_out=72)   # 72 / 16 is no multiple of 4


# ============================================================================================= run_index_build
def test_run_index_build_one_billion_index_type(dev, tmp_path, caplog):
    import logging
    from gnnlm_amd import run_index_build
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(8)
    N, d, V = 62_000, 256, 50                                              # 2048 lists need 30 keys each (knn/index_builder.py:56)
    centres = rs.randn(200, d).astype(np.float32)
    keys = (centres[rs.randint(0, 200, N)] + 0.5 * rs.randn(N, d).astype(np.float32)).astype(np.float16)
    dd = tmp_path / "dstore"
    os.makedirs(dd)
    keys.tofile(dd / "keys.npy")
    rs.randint(0, V, N).astype(np.int16).tofile(dd / "vals.npy")
    json.dump({"dstore_size": N, "hidden_size": d, "vocab_size": V, "dstore_fp16": True, "val_size": 1}, open(dd / "info.json", "w"))
    argv = ["--dstore-dir", str(dd), "--metric", "cosine", "--nprobe", "16", "--opq-iters", "1", "--max-train", "30000"]
    out = run_index_build.main(run_index_build.get_parser().parse_args(argv + ["--index-type", "OPQ16_64,IVF2048,PQ16"]))
    index = IVFPQIndex.load(out, device=dev)
    assert index.R.shape == (64, 256) and index.coarse.shape == (2048, 64) and index.pq.shape == (16, 256, 4) and index.ntotal == N
    # find_knn-style self-queries: the key's own id first at least as often as the float64 search over the same arrays finds it first
    rows = rs.choice(N, 200, replace=False)
    q = keys[rows].astype(np.float32)
    q /= np.sqrt((q ** 2).sum(1, keepdims=True))
    _, i = index.search(q, 4)
    _, i_ref = oivf.search(q, *arrays_of(index), k=4, nprobe=16)
    ours, theirs = float((i[:, 0] == rows).mean()), float((i_ref[:, 0] == rows).mean())
    print(f"self first: ours {ours:.3f}, oracle {theirs:.3f}")
    assert ours >= theirs and theirs > 0
    # a reused file whose rotation has another shape than the flags ask for: the file wins, and the warning says so
    os.remove(out)                                                          # (the trained file stays)
    with caplog.at_level(logging.WARNING, logger="gnnlm_amd.run_index_build"):
        assert run_index_build.main(run_index_build.get_parser().parse_args(argv + ["--index-type", "OPQ16_128,IVF2048,PQ16"])) == out
    assert any("64 dimensions" in r.getMessage() and "128 dimensions" in r.getMessage() for r in caplog.records)


# ============================================================================================= k-means
def test_kmeans_with_the_fused_assignment_recovers_separated_clusters(dev):
    from gnnlm_amd import ivfpq_train
    rs = np.random.RandomState(9)
    k, d, per = 48, 20, 150
    centres = (8.0 * rs.randn(k, d)).astype(np.float32)
    label = np.repeat(np.arange(k), per)
    x = up(centres[label] + 0.1 * rs.randn(k * per, d).astype(np.float32), dev)
    start = up(centres + 0.5 * rs.randn(k, d).astype(np.float32), dev)
    gen = torch.Generator(device=dev)
    got = {}
    for route in ("fused", "dense"):
        gen.manual_seed(0)
        got[route] = ivfpq_train.kmeans(x, k, 5, gen, init=start, coarse=route).cpu().numpy()
    means = np.stack([x.cpu().numpy()[label == c].mean(0) for c in range(k)])
    np.testing.assert_allclose(got["fused"], means, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(got["fused"], got["dense"], rtol=1e-5, atol=1e-5)
