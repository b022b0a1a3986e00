"""gnnlm_ivfpq_keep_flags and gnnlm_ivfpq_list_compact (csrc/ivfpq_remove.hip) at the descriptor level, hand-filled descriptors,
bit for bit against the numpy restatement tests/ivfpq_remove_ref.py.

One index holds lists of 0, 1, 15, 255, 256, 257, 4097 and 70,001 rows (the compaction cuts the rows into chunks of 1024 whatever the
lists are: the long list crosses 68 chunk borders with a carried count, the short ones share chunks); ids are a random permutation with
negative ones and ones above 2^39, so id ranges hit rows scattered over the lists.  Outputs are longer than needed and pre-filled:
nothing outside [0, new_off[nlist]) may change, nor may any input."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ivfpq_remove_ref as rr
from gnnlm_amd import _lib

pytestmark = pytest.mark.gpu

FILL = 0xAB
GUARD = 512                                                               # rows behind new_off[nlist] that must stay as they were
NAMED = [0, 1, 15, 255, 256, 257, 4097, 70001]
REMOVALS = ["none", "all", "ends", "lists", "second", "miss", "one_range", "thousand", "mixed"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _index(nlist, M):
    """(list_off, ids, codes): nlist = 257 holds every named length, 3 holds (257, 0, 70001), 1 the long list alone"""
    rs = np.random.RandomState(nlist * 100 + M)
    if nlist == 1:
        lens = np.array([70001])
    elif nlist == 3:
        lens = np.array([257, 0, 70001])
    else:
        lens = rs.randint(0, 40, nlist)
        lens[rs.rand(nlist) < 0.2] = 0
        lens[rs.choice(nlist, len(NAMED), replace=False)] = NAMED
        lens[-1] = 0                                                      # a trailing empty list: its offset equals N
    off = np.zeros(nlist + 1, np.int64)
    off[1:] = np.cumsum(lens)
    N = int(off[-1])
    base = np.arange(N, dtype=np.int64) - 1000                            # negative ids ...
    base[N // 2:] += 1 << 39                                              # ... and ids above 2^39, a wide gap between
    ids = rs.permutation(base)
    codes = rs.randint(0, 256, (N, M)).astype(np.uint8)
    return off, ids, codes


def _ranges(kind, off, ids, rs):
    N = len(ids)
    lens = off[1:] - off[:-1]
    full = np.nonzero(lens)[0]
    if kind == "none":
        return rr.normalize_ranges()
    if kind == "all":
        return np.array([[ids.min(), ids.max() + 1]], np.int64)
    if kind == "ends":                                                    # first and last row of every non-empty list
        return rr.normalize_ranges(ids=np.concatenate([ids[off[full]], ids[off[full + 1] - 1]]))
    if kind == "lists":                                                   # whole lists, the longest among them
        pick = np.unique(np.concatenate([full[::2], [lens.argmax()]]))
        return rr.normalize_ranges(ids=np.concatenate([ids[off[l]:off[l + 1]] for l in pick]))
    if kind == "second":
        return rr.normalize_ranges(ids=ids[::2])
    if kind == "miss":                                                    # below, between and above the ids
        return np.array([[-(1 << 50), -1000], [N, 1 << 38], [(1 << 39) + N, 1 << 62]], np.int64)
    if kind == "one_range":
        return np.array([[100, (1 << 39) + N // 2 + 300]], np.int64)
    if kind == "thousand":
        lo = rs.choice(np.concatenate([np.arange(-1000, N // 2 - 1000), np.arange(N // 2, N) + (1 << 39) - 1000]), 2000)
        rg = rr.normalize_ranges(ranges=np.stack([lo, lo + rs.randint(1, 30, len(lo))], 1))
        return rg[np.sort(rs.choice(len(rg), 1000, replace=False))]
    if kind == "mixed":
        return rr.normalize_ranges(ids=ids[rs.rand(N) < 0.3], ranges=[(int(ids.min()), int(ids.min()) + 1), (N // 4, N // 4 + 777)])
    raise AssertionError(kind)


def _flags(dev, off, ids, ranges, over=()):
    """-> (keep, list_keep) as written over pre-filled buffers"""
    N, nlist = len(ids), len(off) - 1
    t_ids, t_off, t_rg = up(ids, dev), up(off, dev), up(ranges.reshape(-1, 2), dev)
    keep = torch.full((N + GUARD,), FILL, dtype=torch.uint8, device=dev)
    list_keep = torch.full((nlist + GUARD,), -7, dtype=torch.int64, device=dev)
    f = _lib.gnnlm_ivfpq_keep_flags_t()
    f.ids, f.N, f.list_off, f.nlist = t_ids.data_ptr(), N, t_off.data_ptr(), nlist
    f.ranges, f.n_ranges = (t_rg.data_ptr() if len(ranges) else None), len(ranges)
    f.keep, f.list_keep = keep.data_ptr(), list_keep.data_ptr()
    for k, v in dict(over).items():
        setattr(f, k, v)
    try:
        _lib.call_desc("gnnlm_ivfpq_keep_flags", f)
    finally:
        torch.cuda.synchronize()
        _flags.last = (keep.cpu().numpy(), list_keep.cpu().numpy())
    assert np.array_equal(t_ids.cpu().numpy(), ids) and np.array_equal(t_off.cpu().numpy(), off) and np.array_equal(t_rg.cpu().numpy(), ranges.reshape(-1, 2))
    k, lk = _flags.last
    assert (k[N:] == FILL).all() and (lk[nlist:] == -7).all()
    return k[:N], lk[:nlist]


def _compact(dev, off, ids_old, codes_old, keep, new_off, over=(), shift=0, want_bad=True):
    """-> (ids [rows], codes [rows, M], n_bad), rows = new_off[-1] + GUARD pre-filled rows; `shift`: codes_old starts that many bytes
    into its allocation"""
    N0, nlist, M = len(ids_old), len(off) - 1, codes_old.shape[1]
    rows = max(int(new_off[-1]), 0) + GUARD
    t_off, t_ids, t_keep, t_new = up(off, dev), up(ids_old, dev), up(keep, dev), up(new_off, dev)
    raw = torch.empty(N0 * M + 64, dtype=torch.uint8, device=dev)
    raw[shift:shift + N0 * M] = up(codes_old.reshape(-1), dev)
    ids = torch.full((rows,), FILL, dtype=torch.int64, device=dev)
    codes = torch.full((rows, M), FILL, dtype=torch.uint8, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = _lib.lib().gnnlm_ivfpq_list_compact_workspace_bytes(N0, nlist)
    ws = torch.full((ws_bytes // 8 + 1,), -1, dtype=torch.int64, device=dev)      # (contents free: no zeroing is owed)
    c = _lib.gnnlm_ivfpq_list_compact_t()
    c.list_off_old, c.nlist, c.N0 = t_off.data_ptr(), nlist, N0
    c.ids_old, c.codes_old, c.M, c.keep = t_ids.data_ptr(), raw.data_ptr() + shift, M, t_keep.data_ptr()
    c.new_off, c.ids, c.codes = t_new.data_ptr(), ids.data_ptr(), codes.data_ptr()
    c.n_bad = bad.data_ptr() if want_bad else None
    c.workspace, c.workspace_bytes = ws.data_ptr(), ws_bytes
    for k, v in dict(over).items():
        setattr(c, k, v(c) if callable(v) else v)
    try:
        _lib.call_desc("gnnlm_ivfpq_list_compact", c)
    finally:
        torch.cuda.synchronize()
        _compact.last = (ids.cpu().numpy(), codes.cpu().numpy(), int(bad[0]))
    # the inputs are what they were
    assert np.array_equal(t_off.cpu().numpy(), off) and np.array_equal(t_ids.cpu().numpy(), ids_old) and np.array_equal(t_keep.cpu().numpy(), keep)
    assert np.array_equal(t_new.cpu().numpy(), new_off) and np.array_equal(raw[shift:shift + N0 * M].cpu().numpy(), codes_old.reshape(-1))
    return _compact.last


@pytest.mark.parametrize("kind", REMOVALS)
@pytest.mark.parametrize("nlist,M", [(1, 16), (1, 64), (3, 16), (3, 64), (257, 16), (257, 64)], ids=lambda v: str(v))
def test_remove_bit_for_bit(dev, nlist, M, kind):
    off, ids, codes = _index(nlist, M)
    ranges = _ranges(kind, off, ids, np.random.RandomState(len(kind) + nlist))
    assert len(ranges) == {"none": 0, "all": 1, "one_range": 1, "thousand": 1000}.get(kind, len(ranges))
    w_keep, w_lk = rr.keep_flags(ids, off, ranges)
    keep, list_keep = _flags(dev, off, ids, ranges)
    assert np.array_equal(keep, w_keep) and np.array_equal(list_keep, w_lk)
    removed = int(len(ids) - w_keep.sum())
    assert {"none": removed == 0, "miss": removed == 0, "all": removed == len(ids)}.get(kind, removed > 0)
    new_off = rr.offsets(w_lk)
    rows = int(new_off[-1]) + GUARD
    want = rr.compact(off, ids, codes, w_keep, new_off, rows=rows, fill=FILL)
    got = _compact(dev, off, ids, codes, w_keep, new_off)
    assert got[2] == want[2] == 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])          # the rows from new_off[nlist] on included
    # the same bits from a second call, from codes_old at another 16-byte aligned address, and without n_bad
    for kw in (dict(), dict(shift=16), dict(shift=48, want_bad=False)):
        again = _compact(dev, off, ids, codes, w_keep, new_off, **kw)
        assert np.array_equal(again[0], got[0]) and np.array_equal(again[1], got[1])


def test_any_nonzero_flag_keeps_and_an_odd_flag_address(dev):
    off, ids, codes = _index(257, 16)
    rs = np.random.RandomState(2)
    keep = (rs.rand(len(ids)) < 0.5).astype(np.uint8) * rs.randint(1, 256, len(ids)).astype(np.uint8)
    new_off = rr.offsets(np.array([(keep[off[l]:off[l + 1]] != 0).sum() for l in range(257)], np.int64))
    want = rr.compact(off, ids, codes, keep, new_off, rows=int(new_off[-1]) + GUARD, fill=FILL)
    got = _compact(dev, off, ids, codes, keep, new_off)
    assert got[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the flags at an address that is no multiple of four
    odd = torch.zeros(len(ids) + 8, dtype=torch.uint8, device=dev)
    odd[3:3 + len(ids)] = up(keep, dev)
    got = _compact(dev, off, ids, codes, keep, new_off, over=dict(keep=odd.data_ptr() + 3))
    assert got[2] == 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("delta", [-1, 1])
def test_n_bad_counts_a_wrong_slot_and_the_neighbours_are_intact(dev, delta):
    """new_off gives ONE list a slot one row too short / too long (the lists behind it shift): that list is counted once, writes
    inside its slot only, and every other list holds exactly its survivors"""
    off, ids, codes = _index(257, 64)
    w_keep, w_lk = rr.keep_flags(ids, off, rr.normalize_ranges(ids=ids[::3]))
    l = int(np.argmax(off[1:] - off[:-1] == 4097))
    new_off = rr.offsets(w_lk)
    wrong = new_off.copy()
    wrong[l + 1:] += delta
    rows = int(wrong[-1]) + GUARD
    want = rr.compact(off, ids, codes, w_keep, wrong, rows=rows, fill=FILL)
    got = _compact(dev, off, ids, codes, w_keep, wrong)
    assert got[2] == want[2] == 1
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    good = rr.compact(off, ids, codes, w_keep, new_off)
    for n in (l - 1, l + 1):                                              # the neighbours' rows, read at their own slots
        assert np.array_equal(got[0][wrong[n]:wrong[n + 1]], good[0][new_off[n]:new_off[n + 1]])
        assert np.array_equal(got[1][wrong[n]:wrong[n + 1]], good[1][new_off[n]:new_off[n + 1]])
    if delta > 0:                                                         # the slot's spare row was left alone
        assert got[0][wrong[l + 1] - 1] == FILL and (got[1][wrong[l + 1] - 1] == FILL).all()


def test_unsorted_ranges_stay_inside_the_arrays(dev):
    """ranges that break the precondition: the flags are unspecified, but they are flags, and nothing else is written"""
    off, ids, _ = _index(3, 16)
    rs = np.random.RandomState(4)
    lo = rs.randint(-2000, 1 << 40, 500).astype(np.int64)
    ranges = np.stack([lo, lo - rs.randint(-50, 50, 500)], 1)
    keep, list_keep = _flags(dev, off, ids, ranges)
    assert set(np.unique(keep)) <= {0, 1}
    assert np.array_equal(list_keep, [keep[off[l]:off[l + 1]].sum() for l in range(3)])


def test_refusals_write_nothing(dev):
    off, ids, codes = _index(3, 16)
    w_keep, w_lk = rr.keep_flags(ids, off, rr.normalize_ranges(ids=ids[::2]))
    new_off = rr.offsets(w_lk)
    ranges = rr.normalize_ranges(ids=ids[::2])
    for kw in (dict(N=-1), dict(nlist=-1), dict(n_ranges=-1), dict(nlist=0), dict(ids=None), dict(list_off=None), dict(keep=None),
               dict(ranges=None)):
        with pytest.raises(_lib.GnnlmError):
            _flags(dev, off, ids, ranges, over=kw)
        k, lk = _flags.last
        assert (k == FILL).all() and (lk == -7).all(), kw
    for kw in (dict(M=24), dict(M=8), dict(M=0), dict(N0=-1), dict(nlist=-1), dict(nlist=0), dict(list_off_old=None), dict(ids_old=None),
               dict(codes_old=None), dict(keep=None), dict(new_off=None), dict(ids=None), dict(codes=None), dict(workspace=None),
               dict(workspace_bytes=8), dict(codes_old=lambda c: c.codes_old + 8), dict(codes=lambda c: c.codes + 4),
               dict(workspace=lambda c: c.workspace + 4), dict(codes=lambda c: c.codes_old), dict(ids=lambda c: c.ids_old)):
        with pytest.raises(_lib.GnnlmError):
            _compact(dev, off, ids, codes, w_keep, new_off, over=kw)
        gi, gc, bad = _compact.last
        assert (gc == FILL).all() and (gi == FILL).all() and bad == 0, kw


def test_empty_problems_are_accepted(dev):
    off, ids, codes = _index(3, 16)
    # N = 0 over three lists: the counts are written (zero), nothing else; the compaction touches nothing
    e_off = np.zeros(4, np.int64)
    keep, list_keep = _flags(dev, e_off, ids[:0], rr.normalize_ranges(ids=[1, 2]))
    assert keep.size == 0 and np.array_equal(list_keep, [0, 0, 0])
    gi, gc, bad = _compact(dev, e_off, ids[:0], codes[:0], keep, e_off)
    assert (gc == FILL).all() and (gi == FILL).all() and bad == 0
    # no lists at all, with every pointer NULL
    f = _lib.gnnlm_ivfpq_keep_flags_t()
    _lib.call_desc("gnnlm_ivfpq_keep_flags", f)
    c = _lib.gnnlm_ivfpq_list_compact_t()
    c.M = 16
    _lib.call_desc("gnnlm_ivfpq_list_compact", c)
    torch.cuda.synchronize()
    assert ctypes.sizeof(c) > 0
