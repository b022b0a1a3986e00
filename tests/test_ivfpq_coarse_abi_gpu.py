"""gnnlm_ivfpq_coarse_probes (csrc/ivfpq_coarse.hip) at the descriptor level, hand-filled descriptors, against the float64 restatement
tests/coarse_probes_ref.py.

Integer-valued operands (entries in -4 .. 4, d <= 1024, integer biases: every sum is exact in float32 in any order): values and lists
bit for bit against the restatement AND against gnnlm_gemm_nt + gnnlm_topk_merge on the same device operands.  d = 4 / 20 with such
entries gives hundreds of exact ties per row, straddling the cut and the slab boundaries (the slab count is set by hand); they go to
the lower list.  Rows are read through ldx > d (pad columns NaN); the outputs stand between guards.  Bias entries of -inf and NaN and
a NaN row give "no entry".  Gaussian operands: the search-score bar of the project (rtol 2e-5, atol 2e-4) on every value against the
float64 score of the list returned, rows descending, no omitted list above the row's last value by more than the bar."""
import ctypes

import numpy as np
import pytest
import torch

import coarse_probes_ref as ref
from gnnlm_amd import _lib, ops

pytestmark = pytest.mark.gpu

GUARD = 64
RTOL, ATOL = 2e-5, 2e-4                                                 # tests/test_knn_search_gpu.py::test_ivfpq_one_billion_index_family

# (n, d, nlist, P, bias, slabs): every n in {1, 67, 300}, d in {4, 20, 64, 1024}, nlist in {0, 1, 31, 4097, 70001}, P in {1, 32, 64}, with
# and without a bias; one slab and several (4097 lists in 2 slabs: 2112 + 1985; 70001 in 17: 4160 each, the last 3441)
CASES = [
    (1, 4, 0, 1, False, 1),
    (67, 64, 0, 32, True, 1),
    (67, 20, 1, 32, True, 1),
    (1, 1024, 1, 64, True, 1),
    (300, 64, 31, 64, False, 1),
    (67, 1024, 31, 1, False, 1),
    (67, 4, 4097, 32, True, 2),
    (300, 20, 4097, 1, False, 3),
    (300, 1024, 4097, 32, True, 2),
    (67, 64, 4097, 64, False, 1),
    (1, 64, 70001, 64, True, 5),
    (67, 64, 70001, 32, False, 4),
    (300, 4, 70001, 1, True, 17),
    (67, 20, 70001, 64, False, 1),
    (300, 4, 70001, 32, False, 8),
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Coarse:
    """the device operands of one call: x behind a row stride with NaN pads, the outputs between guards"""

    def __init__(self, x, coarse, bias, P, slabs, dev, pad=4):
        self.n, self.d = x.shape
        self.nlist, self.P, self.slabs = coarse.shape[0], P, slabs
        self.ldx = self.d + pad
        xp = np.full((self.n, self.ldx), np.nan, np.float32)
        xp[:, :self.d] = x
        self.x, self.coarse = up(xp, dev), up(coarse, dev)
        self.bias = None if bias is None else up(bias, dev)
        self.val = torch.full((2 * GUARD + self.n * P,), 7.0, dtype=torch.float32, device=dev)
        self.idx = torch.full((2 * GUARD + self.n * P,), 7, dtype=torch.int64, device=dev)
        self.part_val = torch.empty(self.n, slabs, P, dtype=torch.float32, device=dev)
        self.part_id = torch.empty(self.n, slabs, P, dtype=torch.int64, device=dev)

    def desc(self, **kw):
        c = _lib.gnnlm_ivfpq_coarse_t()
        c.x, c.ldx, c.n = self.x.data_ptr(), self.ldx, self.n
        c.coarse, c.nlist, c.d = self.coarse.data_ptr(), self.nlist, self.d
        if self.bias is not None:
            c.col_bias = self.bias.data_ptr()
        c.k, c.slabs = self.P, self.slabs
        if self.slabs > 1:
            c.part_val, c.part_id = self.part_val.data_ptr(), self.part_id.data_ptr()
        c.out_val, c.out_id = self.val.data_ptr() + 4 * GUARD, self.idx.data_ptr() + 8 * GUARD
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def run(self, **kw):
        _lib.call_desc("gnnlm_ivfpq_coarse_probes", self.desc(**kw))
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        v, i = self.val.cpu().numpy(), self.idx.cpu().numpy()
        m = self.n * self.P
        assert (v[:GUARD] == 7.0).all() and (v[GUARD + m:] == 7.0).all() and (i[:GUARD] == 7).all() and (i[GUARD + m:] == 7).all(), \
            "wrote outside the outputs"
        return v[GUARD:GUARD + m].reshape(self.n, self.P).copy(), i[GUARD:GUARD + m].reshape(self.n, self.P).copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.val == 7.0).all()) and bool((self.idx == 7).all())

    def two_step(self):
        """gnnlm_gemm_nt + gnnlm_topk_merge on the same operands (the dense route)"""
        pv = torch.empty(self.n, self.P, dtype=torch.float32, device=self.x.device)
        pi = torch.empty(self.n, self.P, dtype=torch.int64, device=self.x.device)
        if self.nlist == 0:
            cs = torch.empty(self.n, 0, dtype=torch.float32, device=self.x.device)
        else:
            cs = ops.gemm_nt(self.x[:, :self.d], self.coarse)
        ops.topk_merge(cs, pv, pi, largest=True, init=True, col_bias=self.bias)
        torch.cuda.synchronize()
        return pv.cpu().numpy(), pi.cpu().numpy()


def _integer_case(n, d, nlist, bias, seed):
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(n, d)).astype(np.float32)
    coarse = rs.randint(-4, 5, size=(nlist, d)).astype(np.float32)
    b = None
    if bias:
        b = rs.randint(-3, 4, size=nlist).astype(np.float32)
        if nlist >= 31:                                                  # lists without an entry, at both ends and inside
            b[[0, 7, nlist - 1]] = -np.inf
            b[[3, nlist // 2]] = np.nan
    if n >= 3:
        x[1] = np.nan                                                     # a row without a list between two ordinary rows
    if nlist >= 4097:
        x[0] = 0.0                                                        # row 0 scores a list by its first entry alone: nine values,
        x[0, 0] = 1.0                                                     # hundreds of lists each
    return x, coarse, b


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n,d,nlist,P,bias,slabs", CASES, ids=lambda v: str(v))
def test_integer_operands_bit_for_bit(dev, n, d, nlist, P, bias, slabs):
    x, coarse, b = _integer_case(n, d, nlist, bias, seed=n * 7 + d * 3 + nlist + P)
    c = Coarse(x, coarse, b, P, slabs, dev)
    val, idx = c.run()
    want_v, want_i = ref.coarse_probes(x, coarse, P, b)
    assert np.array_equal(idx, want_i)
    assert np.array_equal(val, want_v.astype(np.float32))                 # (equal as numbers: a zero may carry either sign)
    if n >= 3:
        assert (idx[1] == -1).all() and np.isneginf(val[1]).all()
    if nlist >= 4097:                                                     # row 0: the cut falls inside a run of exact ties
        last = val[0, P - 1]
        s = ref.scores(x[:1], coarse, b)[0]
        assert (s == last).sum() > (100 if b is None or nlist > 5000 else P) and idx[0, P - 1] < np.nonzero(s == last)[0].max()
    tv, ti = c.two_step()
    assert np.array_equal(idx, ti) and np.array_equal(_bits(val + 0.0), _bits(tv + 0.0))


def test_slab_boundary_ties_go_to_the_lower_list(dev):
    """every list scores the same: the P lowest lists, whichever slab they stand in; then the best lists are the LAST of each slab"""
    n, d, nlist, P = 5, 8, 4097, 64
    x = np.ones((n, d), np.float32)
    coarse = np.ones((nlist, d), np.float32)
    for slabs in (1, 2, 7, 64):
        val, idx = Coarse(x, coarse, None, P, slabs, dev).run()
        assert np.array_equal(idx, np.tile(np.arange(P), (n, 1))) and (val == d).all()
    # ties between the last lists of slab 0 (2112 lists wide) and the first of slab 1
    coarse[2100:2130] = 2.0
    val, idx = Coarse(x, coarse, None, 16, 2, dev).run()
    assert np.array_equal(idx, np.tile(np.arange(2100, 2116), (n, 1))) and (val == 2 * d).all()


def test_default_slab_rule_through_ops(dev):
    x, coarse, b = _integer_case(67, 64, 70001, True, seed=5)
    pv = torch.empty(67, 32, dtype=torch.float32, device=dev)
    pi = torch.empty(67, 32, dtype=torch.int64, device=dev)
    assert ops.ivfpq_coarse_slabs(67, 70001, 32) == 17 and ops.ivfpq_coarse_slabs(1 << 18, 1 << 20, 1) == 1
    ops.ivfpq_coarse_probes(up(x, dev), up(coarse, dev), pv, pi, col_bias=up(b, dev))
    want_v, want_i = ref.coarse_probes(x, coarse, 32, b)
    assert np.array_equal(pi.cpu().numpy(), want_i) and np.array_equal(pv.cpu().numpy(), want_v.astype(np.float32))


@pytest.fixture(scope="module")
def gaussian():
    rs = np.random.RandomState(11)
    n, d, nlist = 300, 64, 70001
    coarse = rs.randn(nlist, d).astype(np.float32)
    x = rs.randn(n, d).astype(np.float32)
    return x, coarse, ref.scores(x, coarse)


@pytest.mark.parametrize("slabs", [1, 6])
def test_gaussian_operands_within_the_search_score_bar(dev, gaussian, slabs):
    x, coarse, s64 = gaussian
    P = 32
    val, idx = Coarse(x, coarse, None, P, slabs, dev).run()
    assert (idx >= 0).all() and all(len(set(r)) == P for r in idx)
    got = np.take_along_axis(s64, idx, 1)
    bar = ATOL + RTOL * np.abs(got)
    assert (np.abs(val - got) <= bar).all(), float(np.abs(val - got).max())
    assert (val[:, :-1] >= val[:, 1:]).all()
    rest = s64.copy()
    np.put_along_axis(rest, idx, -np.inf, 1)
    worst = rest.max(1)
    assert (worst <= val[:, -1] + ATOL + RTOL * np.abs(worst)).all()


def test_refusals(dev):
    x, coarse, b = _integer_case(5, 8, 100, True, seed=1)
    c = Coarse(x, coarse, b, 4, 2, dev)
    host = np.zeros(4096, np.float32)
    hp = host.ctypes.data_as(ctypes.c_void_p).value
    bad = [dict(k=65), dict(k=0), dict(d=6), dict(d=0), dict(n=-1), dict(nlist=-1), dict(slabs=0), dict(slabs=2000), dict(ldx=4),
           dict(x=None), dict(out_val=None), dict(out_id=None), dict(coarse=None), dict(part_val=None), dict(part_id=None),
           dict(x=hp), dict(coarse=hp), dict(col_bias=hp), dict(out_val=hp), dict(out_id=hp), dict(part_val=hp), dict(part_id=hp)]
    for kw in bad:
        rc = _lib.lib().gnnlm_ivfpq_coarse_probes(ctypes.byref(c.desc(**kw)), _lib.stream())
        assert rc == -22 and b"ivfpq_coarse_probes" in _lib.lib().gnnlm_last_error(), kw
        assert c.untouched(), kw
    assert _lib.lib().gnnlm_ivfpq_coarse_probes(None, _lib.stream()) == -22
    assert _lib.lib().gnnlm_ivfpq_coarse_probes(ctypes.byref(c.desc(n=0, x=None, out_val=None)), _lib.stream()) == 0 and c.untouched()
    val, idx = c.run()                                                    # the library still works after the refusals
    want_v, want_i = ref.coarse_probes(x, coarse, 4, b)
    assert np.array_equal(idx, want_i) and np.array_equal(val, want_v.astype(np.float32))
