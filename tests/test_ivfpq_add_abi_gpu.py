"""gnnlm_ivfpq_encode_rows and gnnlm_ivfpq_list_merge (csrc/ivfpq_add.hip) at the descriptor level, hand-filled descriptors.

Encode: (a) integer-valued operands (|values| <= 8: every sum exact in any order, duplicated centroids give exact ties) bit for bit
against the float64 restatement tests/ivfpq_add_ref.py; (b) Gaussian operands bit for bit against gnnlm_pq_encode run on the residual
x - coarse[assign] that torch materialises; (c) the same Gaussian codes against the float64 distances under the DERIVED bound of
ivfpq_add_ref.encode -- dist64(chosen) <= min_c dist64(c) + B(chosen) + B(argmin), nothing beyond it.  Rows are read through
ldx > d (pad columns NaN) and written through ld_codes > M between guards over a fill byte: every code must be written, nothing else.

Merge: bit for bit against the restatement, and one case whose old code rows pass 2 GiB."""
import numpy as np
import pytest
import torch

import ivfpq_add_ref as ref
from gnnlm_amd import _lib

pytestmark = pytest.mark.gpu

FILL = 0xAB
GUARD = 256
SHAPES = [(16, 4), (16, 16), (64, 4), (64, 16)]
NS = [1, 63, 64, 65, 257, 1000]
NLISTS = [1, 5, 4097]
# every (M, dsub) meets every n, and every list count at two sizes
ENCODE_CASES = [(M, dsub, n, NLISTS[(i + j) % 3]) for i, (M, dsub) in enumerate(SHAPES) for j, n in enumerate(NS)]
# sub-spaces longer than the kernel's step of 16 dimensions: two full steps, a full and a short one, four steps
ENCODE_CASES += [(16, 32, 257, 5), (16, 20, 65, 4097), (16, 64, 63, 1)]
# bit-identical centroids: inside a thread's four, lanes next to each other, a thread's two halves, the two ends, across every step of
# the row group's reduction
DUPS = [(5, 6), (7, 8), (9, 137), (0, 255), (127, 128), (12, 76), (20, 52), (24, 40), (64, 72), (200, 3, 131)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _case(M, dsub, n, nlist, integer, seed):
    rs = np.random.RandomState(seed)
    d = M * dsub
    if integer:
        x = rs.randint(-8, 9, size=(n, d)).astype(np.float32)
        coarse = rs.randint(-8, 9, size=(nlist, d)).astype(np.float32)
        pq = rs.randint(-8, 9, size=(M, 256, dsub)).astype(np.float32)
        for dup in DUPS:
            pq[:, list(dup[1:])] = pq[:, dup[:1]]
    else:
        coarse = rs.randn(nlist, d).astype(np.float32)
        x = (coarse[rs.randint(0, nlist, n)] + 0.8 * rs.randn(n, d)).astype(np.float32)
        pq = (0.6 * rs.randn(M, 256, dsub)).astype(np.float32)
    asg = rs.randint(0, nlist, n).astype(np.int64)
    norm2 = (pq.astype(np.float64) ** 2).sum(2).astype(np.float32)
    return x, asg, coarse, pq, norm2


class Encode:
    """the device operands of one call: x behind a row stride with NaN pads, codes between guards over FILL"""

    def __init__(self, x, asg, coarse, pq, norm2, dev, pad_x=4, pad_c=3):
        self.n, self.d = x.shape
        self.M, _, self.dsub = pq.shape
        self.nlist = coarse.shape[0]
        self.ldx, self.ldc = self.d + pad_x, self.M + pad_c
        xp = np.full((self.n, self.ldx), np.nan, np.float32)
        xp[:, :self.d] = x
        self.x, self.asg, self.coarse, self.pq, self.norm2 = up(xp, dev), up(asg, dev), up(coarse, dev), up(pq, dev), up(norm2, dev)
        self.codes = torch.full((2 * GUARD + self.n * self.ldc,), FILL, dtype=torch.uint8, device=dev)
        self.cnt = torch.zeros(self.nlist, dtype=torch.int64, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)

    def desc(self, **kw):
        e = _lib.gnnlm_ivfpq_encode_t()
        e.x, e.ldx, e.n, e.assign = self.x.data_ptr(), self.ldx, self.n, self.asg.data_ptr()
        e.coarse, e.nlist, e.pq, e.norm2 = self.coarse.data_ptr(), self.nlist, self.pq.data_ptr(), self.norm2.data_ptr()
        e.M, e.dsub, e.d = self.M, self.dsub, self.d
        e.codes, e.ld_codes = self.codes.data_ptr() + GUARD, self.ldc
        e.list_cnt, e.n_bad = self.cnt.data_ptr(), self.bad.data_ptr()
        for k, v in kw.items():
            setattr(e, k, v)
        return e

    def run(self, **kw):
        _lib.call_desc("gnnlm_ivfpq_encode_rows", self.desc(**kw))
        return self.read()

    def read(self):
        torch.cuda.synchronize()
        raw = self.codes.cpu().numpy()
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + self.n * self.ldc:] == FILL).all(), "wrote outside the code rows"
        rows = raw[GUARD:GUARD + self.n * self.ldc].reshape(self.n, self.ldc)
        assert (rows[:, self.M:] == FILL).all(), "wrote into the pad columns"
        return rows[:, :self.M].copy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.codes == FILL).all()) and int(self.cnt.abs().sum()) == 0 and int(self.bad[0]) == 0


@pytest.mark.parametrize("M,dsub,n,nlist", ENCODE_CASES, ids=lambda v: str(v))
def test_encode_integer_operands_bit_for_bit(dev, M, dsub, n, nlist):
    x, asg, coarse, pq, norm2 = _case(M, dsub, n, nlist, True, seed=M * 1000 + dsub * 100 + n)
    want_bad = 0
    if n >= 3:                                                            # two rows without a list: skipped, counted, never read through
        asg[1], asg[n - 1], want_bad = -1, nlist, 2
    ok = (asg >= 0) & (asg < nlist)
    b = Encode(x, asg, coarse, pq, norm2, dev)
    got = b.run()
    dist, _ = ref.encode(x[ok], asg[ok], coarse, pq, norm2)
    assert np.array_equal(got[ok], ref.codes_of(dist))
    assert (got[~ok] == FILL).all()
    assert int(b.bad[0]) == want_bad
    assert np.array_equal(b.cnt.cpu().numpy(), np.bincount(asg[ok], minlength=nlist))
    # the duplicated centroids are never chosen above their first copy
    for dup in DUPS:
        assert not np.isin(got[ok], [c for c in dup if c != min(dup)]).any()


@pytest.mark.parametrize("M,dsub,n,nlist", ENCODE_CASES, ids=lambda v: str(v))
def test_encode_gaussian_operands(dev, M, dsub, n, nlist):
    x, asg, coarse, pq, norm2 = _case(M, dsub, n, nlist, False, seed=7 + M * 1000 + dsub * 100 + n)
    b = Encode(x, asg, coarse, pq, norm2, dev)
    got = b.run(list_cnt=None, n_bad=None)                               # both optional
    # bit for bit: gnnlm_pq_encode on the residual torch materialises (one rounding per element)
    resid = (b.x[:, :b.d] - b.coarse[b.asg]).contiguous()
    old = torch.empty(n, M, dtype=torch.uint8, device=dev)
    _lib.call("gnnlm_pq_encode", _lib.ptr(resid), resid.stride(0), _lib.ptr(b.pq), _lib.ptr(b.norm2), M, dsub, n, _lib.ptr(old), _lib.stream())
    assert np.array_equal(got, old.cpu().numpy())
    # the derived bound against float64, nothing beyond it
    dist, B = ref.encode(x, asg, coarse, pq, norm2)
    excess = ref.encode_excess(got, dist, B)
    print(f"M={M} dsub={dsub} n={n} nlist={nlist}: {100 * (got == ref.codes_of(dist)).mean():.3f} % float64 argmins, worst excess over the bound {excess:.3e}")
    assert excess <= 0


def test_encode_empty_and_refused(dev):
    x, asg, coarse, pq, norm2 = _case(16, 4, 5, 3, True, seed=1)
    b = Encode(x, asg, coarse, pq, norm2, dev)
    _lib.call_desc("gnnlm_ivfpq_encode_rows", b.desc(n=0, x=None, assign=None, coarse=None, pq=None, norm2=None, codes=None))   # n = 0 touches nothing
    assert b.untouched()
    refused = [dict(M=8, d=32), dict(M=24, d=96), dict(dsub=6, d=96), dict(dsub=2, d=32), dict(d=60), dict(d=68), dict(n=-1), dict(nlist=-1),
               dict(M=-16), dict(dsub=-4), dict(ldx=-1), dict(ld_codes=-1), dict(ldx=63), dict(ld_codes=15)]
    refused += [{k: None} for k in ("x", "assign", "coarse", "pq", "norm2", "codes")]
    for kw in refused:
        with pytest.raises(_lib.GnnlmError):
            _lib.call_desc("gnnlm_ivfpq_encode_rows", b.desc(**kw))
        assert b.untouched(), kw
    with pytest.raises(_lib.GnnlmError):
        _lib.check(_lib.lib().gnnlm_ivfpq_encode_rows(None, _lib.stream()), "null descriptor")
    got = b.run()                                                         # and the descriptor as it stands is taken
    assert np.array_equal(got, ref.codes_of(ref.encode(x, asg, coarse, pq, norm2)[0]))


# ======================================================================================================== merge
def _merge_case(nlist, M, N0, n, seed, empty_frac=0.4):
    rs = np.random.RandomState(seed)
    live_old, live_new = rs.rand(nlist) > empty_frac, rs.rand(nlist) > empty_frac      # lists empty on the old side, the new side, both
    live_old[rs.randint(nlist)] = live_new[rs.randint(nlist)] = True
    pick = lambda live, k: np.sort(rs.choice(np.nonzero(live)[0], size=k)) if live.any() and k else np.zeros(0, np.int64)
    old_asg = pick(live_old, N0)
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(old_asg, minlength=nlist))
    new_asg = rs.permutation(pick(live_new, n)).astype(np.int64)
    ids_old, ids_new = rs.randint(0, 1 << 40, N0).astype(np.int64), rs.randint(0, 1 << 40, n).astype(np.int64)
    codes_old, codes_new = rs.randint(0, 256, (N0, M)).astype(np.uint8), rs.randint(0, 256, (n, M)).astype(np.uint8)
    return off, ids_old, codes_old, new_asg, ids_new, codes_new


def _merge_run(dev, off, ids_old, codes_old, dest, ids_new, codes_new, new_off, pad_new=0, over=()):
    N0, n, M = len(ids_old), len(ids_new), codes_new.shape[1]
    cn = np.full((n, M + pad_new), 0xEE, np.uint8)
    cn[:, :M] = codes_new
    t = [up(a, dev) for a in (off, ids_old, codes_old, dest, ids_new, cn, new_off)]
    ids = torch.full((N0 + n + 2 * GUARD,), FILL, dtype=torch.int64, device=dev)
    codes = torch.full(((N0 + n) * M + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    m = _lib.gnnlm_ivfpq_list_merge_t()
    m.list_off_old, m.nlist, m.N0 = t[0].data_ptr(), len(off) - 1, N0
    m.ids_old, m.codes_old, m.M = t[1].data_ptr(), t[2].data_ptr(), M
    m.n, m.dest, m.ids_new, m.codes_new, m.ld_new = n, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), M + pad_new
    m.new_off, m.ids, m.codes, m.n_bad = t[6].data_ptr(), ids.data_ptr() + 8 * GUARD, codes.data_ptr() + GUARD, bad.data_ptr()
    for k, v in dict(over).items():
        setattr(m, k, v)
    _lib.call_desc("gnnlm_ivfpq_list_merge", m)
    torch.cuda.synchronize()
    ri, rc = ids.cpu().numpy(), codes.cpu().numpy()
    assert (ri[:GUARD] == FILL).all() and (ri[GUARD + N0 + n:] == FILL).all() and (rc[:GUARD] == FILL).all() and (rc[GUARD + (N0 + n) * M:] == FILL).all()
    return ri[GUARD:GUARD + N0 + n], rc[GUARD:GUARD + (N0 + n) * M].reshape(N0 + n, M), int(bad[0])


MERGE_CASES = [(nlist, M, N0, n, pad) for nlist in (1, 3, 4097) for M in (16, 64)
               for N0, n, pad in [(300, 200, 0), (0, 257, 16), (500, 0, 0), (1000, 777, 5)]]


@pytest.mark.parametrize("nlist,M,N0,n,pad", MERGE_CASES, ids=lambda v: str(v))
def test_merge_bit_for_bit(dev, nlist, M, N0, n, pad):
    off, ids_old, codes_old, new_asg, ids_new, codes_new = _merge_case(nlist, M, N0, n, seed=nlist * 7 + M + N0 + n)
    new_off, dest = ref.place(new_asg, off)
    if n > 3:
        dest[2] = N0 + n if (N0 + n) % 2 else -1                          # one position out of range: skipped and counted
    want = ref.merge(off, ids_old, codes_old, dest, ids_new, codes_new, new_off, fill=FILL)
    got = _merge_run(dev, off, ids_old, codes_old, dest, ids_new, codes_new, new_off, pad_new=pad)
    assert got[2] == want[2] == (1 if n > 3 else 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # ... and n_bad is optional
    got = _merge_run(dev, off, ids_old, codes_old, dest, ids_new, codes_new, new_off, pad_new=pad, over=dict(n_bad=None))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_merge_place_wrapper_matches_the_restatement(dev):
    from gnnlm_amd import ops
    off, ids_old, codes_old, new_asg, ids_new, codes_new = _merge_case(37, 16, 400, 333, seed=5)
    new_off, dest = ops.ivfpq_list_place(up(new_asg, dev), up(off, dev))
    w_off, w_dest = ref.place(new_asg, off)
    assert np.array_equal(new_off.cpu().numpy(), w_off) and np.array_equal(dest.cpu().numpy(), w_dest)
    ids, codes = ops.ivfpq_list_merge(up(off, dev), up(ids_old, dev), up(codes_old, dev), dest, up(ids_new, dev), up(codes_new, dev), new_off)
    want = ref.merge(off, ids_old, codes_old, w_dest, ids_new, codes_new, w_off)
    assert np.array_equal(ids.cpu().numpy(), want[0]) and np.array_equal(codes.cpu().numpy(), want[1])
    e_off, e_dest = ops.ivfpq_list_place(torch.zeros(0, dtype=torch.int64, device=dev), up(off, dev))
    assert np.array_equal(e_off.cpu().numpy(), off) and e_dest.numel() == 0


def test_merge_refused(dev):
    off, ids_old, codes_old, new_asg, ids_new, codes_new = _merge_case(3, 16, 20, 10, seed=9)
    new_off, dest = ref.place(new_asg, off)
    for kw in (dict(M=24), dict(M=8), dict(N0=-1), dict(n=-1), dict(nlist=0), dict(ids=None), dict(codes=None), dict(new_off=None),
               dict(dest=None), dict(ids_old=None), dict(codes_new=None), dict(list_off_old=None), dict(ld_new=8)):
        with pytest.raises(_lib.GnnlmError):
            _merge_run(dev, off, ids_old, codes_old, dest, ids_new, codes_new, new_off, over=kw)


def test_merge_beyond_2_gib(dev):
    """M = 64, N0 = 2^25 + 1000: codes_old passes 2 GiB; a new row in the first and in the last list; compared on the device"""
    M, N0 = 64, (1 << 25) + 1000
    off = torch.tensor([0, 1000, 1 << 25, N0], dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(11)
    codes_old = torch.randint(0, 256, (N0, M), dtype=torch.uint8, device=dev, generator=gen)
    ids_old = torch.arange(N0, dtype=torch.int64, device=dev) * 3 + 1
    codes_new = torch.randint(0, 256, (2, M), dtype=torch.uint8, device=dev, generator=gen)
    ids_new = torch.tensor([-5, -7], dtype=torch.int64, device=dev)
    new_off = torch.tensor([0, 1001, (1 << 25) + 1, N0 + 2], dtype=torch.int64, device=dev)
    dest = torch.tensor([1000, N0 + 1], dtype=torch.int64, device=dev)
    from gnnlm_amd import ops
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ids, codes = ops.ivfpq_list_merge(off, ids_old, codes_old, dest, ids_new, codes_new, new_off, n_bad=bad)
    assert int(bad[0]) == 0 and codes.numel() > (1 << 31)
    # first list: 1000 old rows and the new one; last list: 1000 old rows and the new one
    assert torch.equal(ids[:1000], ids_old[:1000]) and torch.equal(codes[:1000], codes_old[:1000])
    assert int(ids[1000]) == -5 and torch.equal(codes[1000], codes_new[0])
    assert torch.equal(ids[(1 << 25) + 1:N0 + 1], ids_old[1 << 25:]) and torch.equal(codes[(1 << 25) + 1:N0 + 1], codes_old[1 << 25:])
    assert int(ids[N0 + 1]) == -7 and torch.equal(codes[N0 + 1], codes_new[1])
    # 1000 sampled rows of the middle list, which moved by one
    j = torch.randint(1000, 1 << 25, (1000,), device=dev, generator=gen)
    assert torch.equal(ids[j + 1], ids_old[j]) and torch.equal(codes[j + 1], codes_old[j])
