"""numpy restatement of REMOVING keys from an IVF-PQ index and of MERGING two (include/gnnlm.h: gnnlm_ivfpq_keep_flags,
gnnlm_ivfpq_list_compact; gnn-lm_amd/ivfpq_train.py: normalize_ranges, remove_rows, merge_lists) -- TEST INFRASTRUCTURE, pinned by
tests/test_ivfpq_remove_ref_cpu.py.  Everything here is integer work: the device results must equal it bit for bit.

  normalize_ranges  ids and (lo, hi) pairs -> sorted, disjoint, non-touching half-open ranges
  keep_flags        keep[s] = no range holds ids[s] (np.searchsorted), list_keep = survivors per list
  compact           the survivors of every list (a boolean mask per list) at new_off[l] .., clipped to the list's own slot
  merge_lists       per list A's rows, then B's"""
import numpy as np


def normalize_ranges(ids=None, ranges=None):
    rows = []
    if ranges is not None:
        for lo, hi in np.asarray(ranges, np.int64).reshape(-1, 2):
            if lo >= hi:
                raise ValueError("lo >= hi")
            rows.append((int(lo), int(hi)))
    if ids is not None:
        rows += [(int(i), int(i) + 1) for i in np.asarray(ids, np.int64).reshape(-1)]
    out = []
    for lo, hi in sorted(rows):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return np.asarray(out, np.int64).reshape(-1, 2)


def keep_flags(ids, list_off, ranges):
    """-> (keep [N] u8, list_keep [nlist] i64); ranges [n, 2] sorted by lo, disjoint"""
    ids, off, ranges = np.asarray(ids, np.int64), np.asarray(list_off, np.int64), np.asarray(ranges, np.int64).reshape(-1, 2)
    j = np.searchsorted(ranges[:, 0], ids, side="right") - 1                # the last range that starts at or below the id
    hit = (j >= 0) & (ids < ranges[np.maximum(j, 0), 1]) if len(ranges) else np.zeros(len(ids), bool)
    keep = (~hit).astype(np.uint8)
    list_keep = np.array([keep[off[l]:off[l + 1]].sum() for l in range(len(off) - 1)], np.int64)
    return keep, list_keep


def offsets(list_keep):
    off = np.zeros(len(list_keep) + 1, np.int64)
    off[1:] = np.cumsum(list_keep)
    return off


def compact(list_off_old, ids_old, codes_old, keep, new_off, rows=None, fill=0):
    """-> (ids [rows], codes [rows, M], n_bad): rows nothing lands on keep `fill` (rows: the buffers' length, default new_off[-1]).
    A list whose survivors are not new_off[l + 1] - new_off[l] is counted and writes its first survivors inside its own slot only
    (and below new_off[-1])."""
    off, new_off = np.asarray(list_off_old, np.int64), np.asarray(new_off, np.int64)
    rows = int(new_off[-1]) if rows is None else rows
    ids = np.full(rows, fill, np.int64)
    codes = np.full((rows, codes_old.shape[1]), fill, np.uint8)
    bad = 0
    for l in range(len(off) - 1):
        m = np.asarray(keep[off[l]:off[l + 1]]) != 0
        si, sc = ids_old[off[l]:off[l + 1]][m], codes_old[off[l]:off[l + 1]][m]
        slot = int(new_off[l + 1] - new_off[l])
        bad += int(len(si) != slot)
        n = max(0, min(len(si), slot, int(new_off[-1] - new_off[l])))
        ids[new_off[l]:new_off[l] + n], codes[new_off[l]:new_off[l] + n] = si[:n], sc[:n]
    return ids, codes, bad


def remove(list_off, list_ids, list_codes, ranges):
    keep, list_keep = keep_flags(list_ids, list_off, ranges)
    new_off = offsets(list_keep)
    ids, codes, bad = compact(list_off, list_ids, list_codes, keep, new_off)
    assert bad == 0
    return new_off, ids, codes


def merge_lists(off_a, ids_a, codes_a, off_b, ids_b, codes_b):
    nlist = len(off_a) - 1
    new_off = offsets((off_a[1:] - off_a[:-1]) + (off_b[1:] - off_b[:-1]))
    ids = np.concatenate([np.concatenate([ids_a[off_a[l]:off_a[l + 1]], ids_b[off_b[l]:off_b[l + 1]]]) for l in range(nlist)]) \
        if nlist else np.zeros(0, np.int64)
    codes = np.concatenate([np.concatenate([codes_a[off_a[l]:off_a[l + 1]], codes_b[off_b[l]:off_b[l + 1]]]) for l in range(nlist)]) \
        if nlist else codes_a[:0]
    return new_off, ids.astype(np.int64), codes
