"""gnnlm_ivfpq_tables (csrc/ivfpq8_prep.hip): the f32 ADC tables and their int8 image in one launch.  Contract under test: the
three outputs are BIT-identical to the pair it replaces (gnnlm_gemm_nt with the descriptor of IVFPQIndex._tables_begin, then
gnnlm_ivfpq_quantize_lut), and a whole search with it (the default) equals the float32 scan's.  Also: the work counters of a
search are its own when two searches are in flight on one index."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _two_launches(qr, pq, dsub):
    from gnnlm_amd import _lib, ops
    n = qr.shape[0]
    lut = torch.empty(n, 64 * 256, device=qr.device, dtype=torch.float32)
    g = _lib.gnnlm_gemm_t()
    g.A, g.lda, g.W, g.ldw, g.C, g.ldc = qr.data_ptr(), qr.stride(0), pq.data_ptr(), dsub, lut.data_ptr(), 64 * 256
    g.M, g.N, g.K, g.batch1 = n, 256, dsub, 64
    g.sA1, g.sW1, g.sC1 = dsub, 256 * dsub, 256
    _lib.call_desc("gnnlm_gemm_nt", g)
    qlut, qmeta = ops.ivfpq_quantize_lut(lut, 64)
    return lut, qlut, qmeta


def _one_launch(qr, pq, dsub):
    from gnnlm_amd import _lib
    n, dev = qr.shape[0], qr.device
    lut = torch.empty(n, 64 * 256, device=dev, dtype=torch.float32)
    qlut = torch.empty(n, 2, 256, 32, device=dev, dtype=torch.uint8)
    qmeta = torch.empty(n, 4, device=dev, dtype=torch.float32)
    t = _lib.gnnlm_ivfpq_tables_t()
    t.qr, t.ld_qr, t.n, t.pq, t.M, t.dsub = qr.data_ptr(), qr.stride(0), n, pq.data_ptr(), 64, dsub
    t.lut, t.ld_lut, t.qlut, t.qmeta = lut.data_ptr(), lut.stride(0), qlut.data_ptr(), qmeta.data_ptr()
    _lib.call_desc("gnnlm_ivfpq_tables", t)
    return lut, qlut, qmeta


@pytest.mark.parametrize("dsub", [4, 8, 16, 32])
@pytest.mark.parametrize("n", [45, 1000])        # 45: the GEMM's 64x64 tiles, a partial query block; 1000: its 128x128 tiles
def test_tables_bitwise_equal_to_gemm_plus_quantize(dev, dsub, n):
    rs = np.random.RandomState(dsub * 1000 + n)
    d = 64 * dsub
    qr = (rs.randn(n, d) / np.sqrt(d)).astype(np.float32)
    pq = (rs.randn(64, 256, dsub) * 0.3).astype(np.float32)
    pq[5] = 0.25                                              # constant sub-table (every code alike)
    qr[2] = 0.0                                               # flat query: every table entry +0
    pq[9] = 40.0 + 1e-4 * rs.randn(256, dsub)                 # a large offset with a tiny range (sub-table 9 of every query)
    qr[3, 9 * dsub:10 * dsub] = 30.0                          # ... and a huge one for query 3
    qr[4, :32 * dsub] *= 100.0                                # sub-tables of very different ranges
    qr_t, pq_t = torch.from_numpy(qr).to(dev), torch.from_numpy(pq).to(dev)
    ref = _two_launches(qr_t, pq_t, dsub)
    got = _one_launch(qr_t, pq_t, dsub)
    for what, a, b in zip(("lut", "qlut", "qmeta"), ref, got):
        assert torch.equal(a, b), (what, float((a != b).float().mean()))
    assert (ref[0][2] == 0).all() and float(ref[2][2, 0]) == float(np.float32(1e-30))   # (the flat query really is flat)


def test_tables_row_stride_and_refusals(dev):
    """qr as a column slice of a wider matrix (row stride > d); shapes the kernel does not cover are refused."""
    from gnnlm_amd import _lib
    rs = np.random.RandomState(5)
    dsub, n = 16, 70
    wide = torch.from_numpy(rs.randn(n, 64 * dsub + 12).astype(np.float32)).to(dev)
    qr = wide[:, 4:4 + 64 * dsub]
    pq = torch.from_numpy(rs.randn(64, 256, dsub).astype(np.float32)).to(dev)
    ref = _two_launches(qr, pq, dsub)
    got = _one_launch(qr, pq, dsub)
    for a, b in zip(ref, got):
        assert torch.equal(a, b)
    with pytest.raises(_lib.GnnlmError):
        _one_launch(torch.zeros(4, 64 * 12, device=dev), torch.zeros(64, 256, 12, device=dev), 12)


def _index(dev, d, N, seed):
    from gnnlm_amd.ivfpq import IVFPQIndex
    rs = np.random.RandomState(seed)
    centres = rs.randn(60, d).astype(np.float32)
    keys = (centres[rs.randint(0, 60, N)] + 0.6 * rs.randn(N, d).astype(np.float32)).astype(np.float16)
    index = IVFPQIndex.build(keys, 24, 64, device=dev, cosine=True, nprobe=9, iters=5, seed=3)
    assert index.tiles is not None
    q = (centres[rs.randint(0, 60, 77)] + 0.6 * rs.randn(77, d)).astype(np.float32)
    q /= np.sqrt((q ** 2).sum(1, keepdims=True))
    return index, torch.from_numpy(q).to(dev)


@pytest.mark.parametrize("d,N", [(256, 150_001), (1024, 60_000)])     # dsub 4 (the small_index shape) and 16 (the reference's)
def test_search_with_fused_tables_equals_f32_scan(dev, d, N):
    from gnnlm_amd.ivfpq import IVFPQIndex
    from test_ivfpq_mfma_gpu import _assert_same
    index, q = _index(dev, d, N, seed=d)
    f32 = IVFPQIndex(index.R, index.coarse, index.pq, index.list_off, index.list_ids, index.list_codes, nprobe=9, scan="f32")
    for k in (1024, 64):
        va, ia = index.search_device(q, k)
        vb, ib = f32.search_device(q, k)
        _assert_same(va.cpu().numpy(), ia.cpu().numpy(), vb.cpu().numpy(), ib.cpu().numpy(), k)


def test_stats_belong_to_the_search_that_finished(dev):
    """Two searches in flight on one index (bench.py --lanes, the pipelined eval_lm): index.stats describes the search that
    finished last, not the one that began last."""
    index, q = _index(dev, 256, 150_001, seed=256)
    a = index.search_begin(q, 1024)
    b = index.search_begin(q[:20].contiguous(), 1024)
    a.result()
    assert index.stats["queries"] == 77
    pairs_a = float(index.stats["pairs"])
    b.result()
    assert index.stats["queries"] == 20 and float(index.stats["pairs"]) < pairs_a
