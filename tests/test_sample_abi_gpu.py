"""gnnlm_sample_topk at the descriptor level: ids, next_logp and done exact.  The uniform numbers sit at the midpoints of the float64
CDF intervals of chosen columns whose relative width is >= 1e-3 -- three orders of magnitude above what a float32 prefix sum in any
association order can move a boundary (N * 2^-24 relative at N = 2048 is 1.2e-4 at the very worst, 2^-24 * log2 N typically) -- so
no case sits on a boundary and none is left out.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import decode_ref as dr

pytestmark = pytest.mark.gpu

PAD, EOS = 1, 2
MIN_WIDTH = 1e-3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def sorted_rows(N, n_rows, seed, tail):
    """Sorted log-probs [n_rows, N] (best first) with a flat enough profile that many columns are wide, ids a permutation that avoids
    pad and eos; ``tail``: that many -inf entries (id -1) at the end of every second row (N > 300: every row is cut, see below)."""
    rs = np.random.RandomState(seed)
    logp = -np.sort(rs.rand(n_rows, N) * (2.0 if N <= 65 else 0.5), axis=1) - 1.0
    ids = np.stack([rs.permutation(N) + 10 for _ in range(n_rows)]).astype(np.int64)
    for r in range(n_rows):
        # at most ~300 columns can each hold 1e-3 of the mass with room to spare: a wide row keeps 300 (200) finite entries
        cut = (300 - 100 * (r % 2)) if N > 300 else (N - tail if r % 2 and N > tail else N)
        logp[r, cut:], ids[r, cut:] = -np.inf, -1
    return logp.astype(np.float32), ids


def chosen_columns(logp_row):
    """The first column, the last with positive mass, the columns on either side of 64 and one in the middle -- those that exist and are wide enough."""
    c = dr.sample_cdf(logp_row)
    last = int(np.isfinite(logp_row).sum()) - 1
    cols = sorted({j for j in (0, 1, last // 2, 62, 63, 64, 65, last - 1, last) if 0 <= j <= last})
    lo = np.concatenate([[0.0], c[:-1]])
    keep = [j for j in cols if (c[j] - lo[j]) / c[-1] >= MIN_WIDTH]
    return keep, [float((lo[j] + c[j]) / (2 * c[-1])) for j in keep]


def run(dev, logp, ids, u=None, done=None, want_logp=True, ld_pad=0):
    from gnnlm_amd import _lib
    B, N = logp.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    lp = torch.full((B, N + ld_pad), float("nan"), device=dev)
    lp[:, :N] = t(logp)
    idt = torch.full((B, N + ld_pad), -7, dtype=torch.int64, device=dev)
    idt[:, :N] = t(ids)
    nxt = torch.full((B,), -99, dtype=torch.int64, device=dev)
    nlp = torch.full((B,), 777.0, device=dev)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = [lp, idt, nxt, nlp, n_bad]
    s = _lib.gnnlm_sample_topk_t()
    s.logp, s.ld_logp, s.ids, s.ld_ids, s.B, s.N = lp.data_ptr(), N + ld_pad, idt.data_ptr(), N + ld_pad, B, N
    if u is not None:
        ut = t(np.asarray(u, np.float32))
        keep.append(ut)
        s.u = ut.data_ptr()
    s.pad, s.eos, s.next = PAD, EOS, nxt.data_ptr()
    if want_logp:
        s.next_logp = nlp.data_ptr()
    dn = None
    if done is not None:
        dn = t(np.asarray(done, np.int32))
        s.done = dn.data_ptr()
    s.n_bad = n_bad.data_ptr()
    rc = _lib.lib().gnnlm_sample_topk(ctypes.byref(s), _lib.stream())
    torch.cuda.synchronize()
    return rc, nxt.cpu().numpy(), nlp.cpu().numpy(), None if dn is None else dn.cpu().numpy(), int(n_bad.item())


@pytest.mark.parametrize("N", [1, 2, 64, 65, 2048])
def test_sampling_picks_the_column_of_u(dev, N):
    logp, ids = sorted_rows(N, 4, 40 + N, tail=0 if N < 64 else 5)
    rows, us, cols = [], [], []
    for r in range(logp.shape[0]):
        keep, mids = chosen_columns(logp[r])
        assert 0 in keep or N > 1
        for j, u in zip(keep, mids):
            rows.append(r), us.append(u), cols.append(j)
    for r in range(logp.shape[0]):                                            # nothing chosen was left out for being narrow
        last = int(np.isfinite(logp[r]).sum()) - 1
        mine = {c for rr, c in zip(rows, cols) if rr == r}
        assert {0, last} <= mine and (N < 66 or {62, 63, 64, 65} <= mine)
    L, I = logp[rows], ids[rows]
    rc, nxt, nlp, done, bad = run(dev, L, I, u=us, done=np.zeros(len(rows)), ld_pad=3)
    want, col, wdone, wbad = dr.sample_ref(L, I, np.asarray(us, np.float32), PAD, EOS)
    assert rc == 0 and bad == wbad == 0
    assert col.tolist() == cols
    assert np.array_equal(nxt, want)
    assert np.array_equal(nlp.view(np.uint32), L[np.arange(len(rows)), cols].view(np.uint32))
    assert np.array_equal(done, wdone) and not done.any()
    # u = 0 is column 0; greedy is column 0
    for u in (np.zeros(len(rows), np.float32), None):
        rc, nxt, nlp, _, _ = run(dev, L, I, u=u)
        assert rc == 0 and np.array_equal(nxt, I[:, 0]) and np.array_equal(nlp.view(np.uint32), L[:, 0].view(np.uint32))


def test_done_eos_and_rows_with_nothing_to_pick(dev):
    N = 8
    logp, ids = sorted_rows(N, 6, 7, tail=0)
    ids[0, 0] = EOS                                   # greedy picks eos: done is set
    logp[2, :] = -np.inf                              # an empty top-N
    logp[3, 0] = np.nan
    logp[5, 0] = np.inf
    done = np.array([0, 1, 0, 0, 0, 0], np.int32)    # row 1 is done already
    for u in (None, np.full(6, 1e-6, np.float32)):
        rc, nxt, nlp, dn, bad = run(dev, logp, ids, u=u, done=done)
        assert rc == 0
        assert nxt.tolist() == [EOS, PAD, PAD, PAD, int(ids[4, 0]), PAD]
        assert dn.tolist() == [1, 1, 1, 1, 0, 1] and bad == 3
        assert nlp[0] == logp[0, 0] and nlp[4] == logp[4, 0]
        assert (nlp[[1, 2, 3, 5]] == 777.0).all()        # untouched
    # sampling reaches an eos that is not in column 0
    logp2, ids2 = sorted_rows(4, 1, 3, tail=0)
    ids2[0, 2] = EOS
    keep, mids = chosen_columns(logp2[0])
    assert 2 in keep
    rc, nxt, _, dn, _ = run(dev, logp2, ids2, u=[mids[keep.index(2)]], done=[0])
    assert nxt.tolist() == [EOS] and dn.tolist() == [1]
    # no done, no next_logp, no n_bad counter needed
    rc, nxt, nlp, dn, _ = run(dev, logp, ids, want_logp=False)
    assert rc == 0 and nxt.tolist() == [EOS, int(ids[1, 0]), PAD, PAD, int(ids[4, 0]), PAD] and (nlp == 777.0).all()


def test_refusals_and_wrapper(dev):
    from gnnlm_amd import _lib, ops
    logp, ids = sorted_rows(8, 2, 1, tail=0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s = _lib.gnnlm_sample_topk_t()
    nxt = torch.full((2,), -99, dtype=torch.int64, device=dev)
    lp, idt = t(logp), t(ids)
    s.logp, s.ld_logp, s.ids, s.ld_ids, s.B, s.N, s.next = lp.data_ptr(), 8, idt.data_ptr(), 8, 2, 8, nxt.data_ptr()
    L = _lib.lib()
    for field, value in (("N", 0), ("N", 2049), ("B", -1), ("ld_logp", 7), ("ld_ids", 7), ("logp", None), ("ids", None), ("next", None)):
        old = getattr(s, field)
        setattr(s, field, value)
        assert L.gnnlm_sample_topk(ctypes.byref(s), _lib.stream()) == -22, field
        setattr(s, field, old)
    assert L.gnnlm_sample_topk(None, _lib.stream()) == -22
    torch.cuda.synchronize()
    assert (nxt == -99).all()
    s.B = 0
    assert L.gnnlm_sample_topk(ctypes.byref(s), _lib.stream()) == 0
    got, got_lp = ops.sample_topk(lp, idt)
    assert torch.equal(got, idt[:, 0]) and torch.equal(got_lp, lp[:, 0])
    with pytest.raises(TypeError):
        ops.sample_topk(lp, idt.int())
