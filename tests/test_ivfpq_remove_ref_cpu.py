"""Removing keys from an IVF-PQ index and merging two, without a GPU: the numpy restatement (tests/ivfpq_remove_ref.py) pinned
against a plain membership loop and against the ADD restatement (tests/ivfpq_add_ref.py) -- compact(merge(layout(A), B), ids of
B) == layout(A) and merge_lists(layout(A), layout(B)) == add of B onto A, bit for bit -- then ``ivfpq_train.normalize_ranges`` on CPU
tensors, the ``edit_index`` parser and its host-only refusals, and the ABI additions."""
import ctypes
import re

import numpy as np
import pytest
import torch

import ivfpq_add_ref as ar
import ivfpq_remove_ref as rr


def _rows(rs, nlist, M, n, id_lo=0, id_hi=1 << 20):
    """n rows given in id order: (assign, ids, codes) with distinct random ids"""
    ids = rs.choice(np.arange(id_lo, id_hi), size=n, replace=False).astype(np.int64)
    return rs.randint(0, nlist, n).astype(np.int64), ids, rs.randint(0, 256, (n, M)).astype(np.uint8)


def test_flags_equal_a_membership_loop():
    rs = np.random.RandomState(0)
    ids = rs.permutation(np.arange(-20, 60)).astype(np.int64)
    off = np.array([0, 0, 7, 7, 30, 79, 80, 80], np.int64)
    for ranges in ([], [(3, 4)], [(-25, -18), (0, 1), (10, 20), (59, 70)], [(-100, 100)], [(100, 200)], [(5, 6), (6, 7), (8, 30)]):
        rg = np.asarray(ranges, np.int64).reshape(-1, 2)
        keep, list_keep = rr.keep_flags(ids, off, rg)
        want = [0 if any(lo <= int(i) < hi for lo, hi in ranges) else 1 for i in ids]
        assert keep.dtype == np.uint8 and keep.tolist() == want
        assert list_keep.tolist() == [sum(want[off[l]:off[l + 1]]) for l in range(len(off) - 1)]
        assert rr.offsets(list_keep)[-1] == sum(want)


def test_normalize_ranges_restatement():
    assert rr.normalize_ranges(ids=[5, 3, 4, 4, 9]).tolist() == [[3, 6], [9, 10]]
    assert rr.normalize_ranges(ranges=[(10, 20), (0, 5), (5, 7), (15, 30), (40, 41)]).tolist() == [[0, 7], [10, 30], [40, 41]]
    assert rr.normalize_ranges(ids=[7, 100], ranges=[(0, 7)]).tolist() == [[0, 8], [100, 101]]
    assert rr.normalize_ranges().shape == (0, 2) and rr.normalize_ranges(ids=[]).shape == (0, 2)
    with pytest.raises(ValueError):
        rr.normalize_ranges(ranges=[(3, 3)])


@pytest.mark.parametrize("nlist,M,nA,nB", [(1, 16, 40, 13), (7, 16, 300, 200), (257, 64, 500, 700), (5, 16, 0, 50), (5, 16, 50, 0)])
def test_remove_undoes_add_and_merge_equals_add(nlist, M, nA, nB):
    rs = np.random.RandomState(nlist + nA + nB)
    asg, ids, codes = _rows(rs, nlist, M, nA + nB)
    A, B = slice(0, nA), slice(nA, nA + nB)
    lay_a = ar.layout(asg[A], ids[A], codes[A], nlist)
    # add B onto layout(A): the add restatement's placement and merge
    new_off, dest = ar.place(asg[B], lay_a[0])
    ids_ab, codes_ab, bad = ar.merge(*lay_a, dest, ids[B], codes[B], new_off)
    assert bad == 0
    # ... removing B's ids (shuffled, as single ids) gives layout(A) back, bit for bit
    got = rr.remove(new_off, ids_ab, codes_ab, rr.normalize_ranges(ids=rs.permutation(ids[B])))
    for g, w in zip(got, lay_a):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    # ... and merging the two layouts is that add
    lay_b = ar.layout(asg[B], ids[B], codes[B], nlist)
    got = rr.merge_lists(*lay_a, *lay_b)
    for g, w in zip(got, (new_off, ids_ab, codes_ab)):
        assert g.dtype == w.dtype and np.array_equal(g, w)


def test_compact_counts_and_contains_an_inconsistent_list():
    rs = np.random.RandomState(3)
    asg, ids, codes = _rows(rs, 4, 16, 60)
    off, lids, lcodes = ar.layout(asg, ids, codes, 4)
    keep, list_keep = rr.keep_flags(lids, off, rr.normalize_ranges(ids=ids[::3]))
    new_off = rr.offsets(list_keep)
    want = rr.compact(off, lids, lcodes, keep, new_off, fill=0xAB)
    assert want[2] == 0
    short = new_off.copy()
    short[2:] -= 1                                                         # list 1 gets one row too few: its last survivor has no place
    got = rr.compact(off, lids, lcodes, keep, short, fill=0xAB)
    assert got[2] == 1
    assert np.array_equal(got[0][:short[2]], want[0][:new_off[2] - 1]) and np.array_equal(got[0][short[2]:], want[0][new_off[2]:])


def test_train_normalize_ranges_on_cpu_tensors():
    from gnnlm_amd import ivfpq_train
    rs = np.random.RandomState(5)
    nr = lambda **kw: ivfpq_train.normalize_ranges(device="cpu", **kw)
    cases = [dict(ids=np.array([5, 3, 4, 4, 9])),                                           # unsorted, duplicates
             dict(ids=torch.tensor([7, 100, -3, -2]), ranges=[(0, 7)]),                      # ids touching a range, negative ids
             dict(ranges=[(10, 20), (0, 5), (5, 7), (15, 30), (40, 41)]),                    # touching and overlapping
             dict(ranges=np.array([[0, 100], [10, 20], [30, 40], [100, 101]])),              # ranges inside a range
             dict(ids=rs.randint(-50, 50, 200), ranges=[(int(a), int(a) + int(b)) for a, b in zip(rs.randint(-80, 80, 20), rs.randint(1, 9, 20))]),
             dict(ids=np.array([1 << 40, (1 << 40) + 1], np.int64)),
             dict(), dict(ids=np.zeros(0, np.int64)), dict(ranges=[])]
    for kw in cases:
        got = nr(**kw)
        want = rr.normalize_ranges(**{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        assert got.dtype == torch.int64 and got.shape == want.shape and got.is_contiguous() and np.array_equal(got.numpy(), want)
        assert bool((got[:, 0] < got[:, 1]).all()) and bool((got[1:, 0] > got[:-1, 1]).all())
    for bad in ([(3, 3)], [(0, 5), (9, 2)]):
        with pytest.raises(ValueError):
            nr(ranges=bad)


def test_edit_index_parser_and_refusals(tmp_path):
    from gnnlm_amd import edit_index
    assert edit_index.parse_ranges("100:200,5000:5100") == [(100, 200), (5000, 5100)]
    assert edit_index.parse_ranges(" 7:8 , -5:-1,") == [(7, 8), (-5, -1)] and edit_index.parse_ranges("") == []
    for bad in ("5", "5:", "a:b", "9:3", "4:4", "1:2:3", "1-2"):
        with pytest.raises(ValueError):
            edit_index.parse_ranges(bad)
    src, out = str(tmp_path / "in.gnnlm.npz"), str(tmp_path / "out.gnnlm.npz")
    open(src, "wb").close()
    parse = lambda *a: edit_index.get_parser().parse_args(["--index-file", src] + list(a))
    a = parse("--out", out, "--remove-ranges", "1:2", "--merge", "x.npz", "y.npz", "--remove-ids-file", "ids.npy", "--cuda", "1")
    assert (a.merge, a.remove_ids_file, a.cuda) == (["x.npz", "y.npz"], "ids.npy", 1) and edit_index.check_args(a) == [(1, 2)]
    # host-only refusals, raised by main before any device work (the input file is empty: reading it would fail differently)
    for argv, what in ((("--out", out), "nothing to do"),
                       (("--out", src, "--remove-ranges", "1:2"), "input"),
                       (("--out", str(tmp_path / "." / "in.gnnlm.npz"), "--remove-ranges", "1:2"), "input"),
                       (("--out", out, "--merge", out), "input"),
                       (("--out", out, "--remove-ranges", "5:1"), "lo:hi"),
                       (("--out", out, "--remove-ranges", "1:2,x"), "lo:hi"),
                       (("--out", str(tmp_path / "out.bin"), "--remove-ranges", "1:2"), ".gnnlm.npz")):
        with pytest.raises(ValueError, match=re.escape(what)):
            edit_index.main(parse(*argv))
    assert "run_index_build" in edit_index.__doc__ and "resume" in edit_index.__doc__


def test_abi_additions():
    from gnnlm_amd import _lib
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", text) and _lib.ABI_VERSION == 12        # additions only
    syms = _lib.exported_symbols()
    L = _lib.lib()
    for name in ("gnnlm_ivfpq_keep_flags", "gnnlm_ivfpq_list_compact", "gnnlm_ivfpq_list_compact_workspace_bytes"):
        assert name in syms and hasattr(L, name)
    for name in ("gnnlm_ivfpq_keep_flags_t", "gnnlm_ivfpq_list_compact_t"):
        assert L.gnnlm_sizeof(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0
    assert [f[0] for f in _lib.STRUCTS["gnnlm_ivfpq_keep_flags_t"]._fields_] == [
        "ids", "N", "list_off", "nlist", "ranges", "n_ranges", "keep", "list_keep"]
    assert [f[0] for f in _lib.STRUCTS["gnnlm_ivfpq_list_compact_t"]._fields_] == [
        "list_off_old", "nlist", "N0", "ids_old", "codes_old", "M", "keep", "new_off", "ids", "codes", "n_bad", "workspace", "workspace_bytes"]
    # the workspace: one count per chunk of rows and one per list boundary; nothing for an empty problem
    ws = L.gnnlm_ivfpq_list_compact_workspace_bytes
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(1, 1) == 8 * 3 and ws(1 << 33, 1 << 20) >= 8 * ((1 << 20) + 1)
    assert ws(1 << 33, 1 << 20) < (1 << 33) // 64                             # far below one byte per key
    # refusals are decided on the host, before anything is launched
    f = _lib.gnnlm_ivfpq_keep_flags_t()
    f.N = -1
    assert L.gnnlm_ivfpq_keep_flags(ctypes.byref(f), None) == -22 and L.gnnlm_ivfpq_keep_flags(None, None) == -22
    f.N, f.nlist = 4, 0
    assert L.gnnlm_ivfpq_keep_flags(ctypes.byref(f), None) == -22
    c = _lib.gnnlm_ivfpq_list_compact_t()
    c.M, c.nlist, c.N0 = 24, 1, 1
    assert L.gnnlm_ivfpq_list_compact(ctypes.byref(c), None) == -22 and b"M % 16" in L.gnnlm_last_error()
    c.M = 16
    assert L.gnnlm_ivfpq_list_compact(ctypes.byref(c), None) == -22 and L.gnnlm_ivfpq_list_compact(None, None) == -22
    # an empty problem is accepted and launches nothing
    c.N0 = c.nlist = 0
    assert L.gnnlm_ivfpq_list_compact(ctypes.byref(c), None) == 0
    f.N = f.nlist = 0
    assert L.gnnlm_ivfpq_keep_flags(ctypes.byref(f), None) == 0
