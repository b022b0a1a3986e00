"""IVF-PQ index searched on the GPU -- the on-device replacement of the reference's faiss CPU search
(``knn/knn_model.py:87-101``: ``index.search`` on ``faiss_store.cosine`` = ``OPQ64_1024,IVF4096,PQ64``, nprobe 32,
``gnnlm_scripts/wiki103/find_knn.sh:8-13``; built by ``knn/index_builder.py``).

The algorithm is faiss's published IVFADC with residual codes and an OPQ pre-rotation, inner-product metric:

    x' = R x                       (cosine index: x is L2-normalised first, index_builder.py:90-95,118)
    list(x) = argmax_l <x', c_l>   residual r = x' - c_list,  code_m = argmin_c |r_m - p_mc|^2
    score(q, x) = <q', c_list(x)> + sum_m <q'_m, p_{m, code_m(x)}>         (ADC, look-up table per query)
    search: the nprobe lists with the largest <q', c_l>, then the k best scores among their members.

Search path (everything on the device, nothing [n, N]-sized): rotation, coarse scores and look-up tables on the f32
MFMA GEMM (``gnnlm_gemm_nt``), probe selection and k-selection by ``gnnlm_ivfpq_select_probes`` / ``gnnlm_ivfpq_select_final``
(``gnnlm_topk_merge`` for the float32 scan's rounds and for shapes beyond their limits), the list scan by
``gnnlm_ivfpq_scan`` in two rounds -- the best ``dense_probes`` lists of every query are scored in full and give its
k-th-best threshold, the remaining lists only emit scores above that threshold.

At M = 64 (the reference's PQ64) the thresholded round is a FILTER on the int8 matrix cores followed by an exact re-score
(``csrc/ivfpq8_scan.hip``: 8-bit tables with a guaranteed one-sided bound, eight queries of a list per workgroup, the
sums taken by ``v_smfmac_i32_16x16x128_i8`` (round 3: ``v_mfma_i32_16x16x64_i8``); survivors re-scored in float32 in the summation order of the float32 scan), so
candidates and scores are those of the one-pass float32 scan -- ``IVFPQIndex(..., scan="f32")`` selects that scan.
With ``attach_vals`` the index carries each key's label next to its id (one 8-byte payload per key), and the search
returns ``vals[ids]`` with the neighbours: the label gather of knn/knn_model.py:198 disappears.

Host path of one search ("The search's host path"): the constructor names the index's ROUTE once (``choose_route``:
"int8" / "packed" / "rowmajor", with the L2 term in use); every call turns its numbers into one ``SearchPlan`` (``plan_search``:
probes, capacities, block size, sampled rank, who splits the payloads); every query block fills one ``_Block`` of buffers and runs
its route's rounds; the call's ``_Outcome`` waits in a ``_PendingSearch`` until ``_finish`` has looked at the survivor counts and
repaired what overflowed.  One private function fills each kernel descriptor.  ``IVFPQIndex.build`` is the offline producer
(``ivfpq_train.py``); ``IVFPQIndex.train`` + ``add`` are its two halves: an index, however it was made, takes new keys without retraining.

PARITY UNPINNED against faiss itself (not in the image, no version pinned): the pin is the numpy restatement
``oracle/ivfpq.py`` over the SAME index arrays (tests/test_knn_search_gpu.py)."""
import contextlib
import ctypes
import os
from collections import namedtuple
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib, ivfpq_train, ops


class _LazyStats(dict):
    """Work counters of a search whose device-side terms are only reduced when somebody reads them: a search enqueues no
    bookkeeping kernels for numbers that only bench.py and the tests look at (``add`` keeps the tensors and a thunk)."""

    def add(self, key, thunk):
        dict.setdefault(self, key, 0)
        self.__dict__.setdefault("_pending", {}).setdefault(key, []).append(thunk)

    def set(self, key, value):
        """a number the host knows already"""
        dict.__setitem__(self, key, value)

    def _resolve(self, key):
        pend = self.__dict__.get("_pending", {}).pop(key, None)
        if pend:
            dict.__setitem__(self, key, dict.__getitem__(self, key) + sum(t() for t in pend))

    def __getitem__(self, key):
        self._resolve(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        return self[key] if key in self else default

    def items(self):
        return [(k, self[k]) for k in list(self.keys())]


def choose_route(M, ntotal, max_list, nlist, scan=None, metric="ip", list_term_bytes=4 << 30):
    """The kernels an index is searched with, decided once from the constructor's numbers -> (route, L2 term | None).
    route "int8": M = 64, the int8-MFMA filter + exact re-score over tiles of 16 code rows (csrc/ivfpq8_scan.hip, ivfpq8_rescore.hip);
    "packed": M = 32 / 64, the float32 scan over its own image of the code rows (blocks of 64 rows, bytes in rotated order) and
    tables in [half][code][sub-quantizer] order -- look-ups without LDS bank conflicts (csrc/ivfpq.hip); scan="f32" asks for it at
    M = 64 too (tests compare the int8 search with it);  "rowmajor": one table per (query, list) task over the codes as stored.
    L2 term (see ``IVFPQIndex.__init__``): "list_term", "key_term", or None (inner product, or an L2 index without keys)."""
    term = None
    if metric == "l2":
        fits = nlist * M * 1024 <= list_term_bytes
        if fits and (M != 64 or scan == "rowmajor"):
            term = "list_term"
        elif ntotal:
            term = "key_term"
        scan = "f32" if M == 64 and scan != "rowmajor" else "rowmajor"
    if scan == "rowmajor":
        return "rowmajor", term
    # (a survivor record packs the row inside its list into 19 bits and the list into 18: longer / more lists take the float32 scan)
    if M == 64 and ntotal and ntotal < (1 << 32) and scan != "f32" and max_list < (1 << IVFPQIndex.SURV_ROW_BITS) and nlist <= (1 << IVFPQIndex.SURV_LIST_BITS):
        return "int8", term
    return ("packed" if M in (32, 64) and ntotal else "rowmajor"), term


def choose_coarse(route, nlist, coarse=None):
    """How an index takes its coarse step (the nprobe best lists of a query), decided once from the constructor's numbers -> "dense":
    the [queries, nlist] scores on ``gnnlm_gemm_nt``, then the probe selection over them; "fused": ``gnnlm_ivfpq_coarse_probes``
    (csrc/ivfpq_coarse.hip), scores and selection in one kernel, no score matrix -- the float32 routes from
    ``ivfpq_train.COARSE_FUSED_MIN_LISTS`` lists on.  The int8 route reads the coarse scores again in its scan and stays dense.
    ``coarse`` = "dense" / "fused" forces a route; the environment's GNNLM_IVF_COARSE does the same for the float32 routes (A/B runs)."""
    if coarse not in (None, "dense", "fused"):
        raise ValueError(f"IVFPQIndex: coarse is 'dense' or 'fused', got {coarse!r}")
    if coarse is not None:
        return coarse
    if route == "int8":
        return "dense"
    env = os.environ.get("GNNLM_IVF_COARSE")
    if env:
        if env not in ("dense", "fused"):
            raise ValueError(f"GNNLM_IVF_COARSE is 'dense' or 'fused', got {env!r}")
        return env
    return "fused" if nlist >= ivfpq_train.COARSE_FUSED_MIN_LISTS else "dense"


# What a plan depends on besides the call's own arguments: the index's route and sizes (score_bytes: the budget of the dense round's
# score rows per query block), its sampling settings as they are now (``_finish`` may have changed them), and the two switches of the
# environment as they are now (select: GNNLM_IVF_SELECT != "0"; env_query_block: GNNLM_IVF_QUERY_BLOCK)
SearchNumbers = namedtuple("SearchNumbers", "route nprobe nlist ntotal max_list score_bytes has_vals threshold_sample "
                                            "sample_min_keys_per_k sample_sigmas select env_query_block")
# Every per-call quantity of one pass over a batch of queries, by the rules of ``plan_search``: lists probed per query, of which the best
# `dense` give the threshold; records per query the thresholded round may emit (int8: the filter's survivors) and candidate columns;
# queries per block; the int8 threshold pass histograms every S-th tile of 16 keys and takes the bound of rank `rank` of that sample;
# fold: the final selection stores (id, label) itself, no split pass over [n, k]
SearchPlan = namedtuple("SearchPlan", "k nprobe dense cap ccap query_block qb S rank fold select")


def plan_search(ix, k, dense_probes, cap, query_block=None, fold=None):
    """Numbers in, numbers out (no tensors).  ``fold`` not None: decided by the caller (rows searched again come back in the state
    of the pass they belong to, split once or not at all)."""
    int8 = ix.route == "int8"
    nprobe = min(ix.nprobe, ix.nlist)
    dense = max(1, min(dense_probes, nprobe))
    # (the int8 path: `cap` bounds a query's SURVIVORS of the filter; what scores above the refined threshold afterwards is a fraction of them
    # and gets 16384 columns at most -- the width the one-chunk k-selection takes)
    ccap = min(cap, 16384) if int8 else cap
    if query_block is None:
        # (the int8 filter groups 8 queries per list: the more queries a block holds, the fuller its groups and the longer a list's bytes
        # stay in the XCD's L2 -- per 8192 queries 12.2 ms in blocks of 8192, 11.4 of 16384, 11.0 of 32768; ~18 GB of temporaries at 32768)
        query_block = ix.env_query_block if int8 else 1024
    # the dense round's score rows: query_block * dense * max_list floats, bounded (a skewed index has long lists)
    qb = query_block if int8 else max(1, min(query_block, ix.score_bytes // max(1, 4 * dense * max(ix.max_list, 1))))
    # The threshold pass histograms a SAMPLE of its lists' keys (every S-th tile of 16) when they hold plenty of them: tau is then the
    # bound of rank k / S + 4.5 sigma of the sample (sigma = sqrt(k (S - 1)) / S: the k best land in the sample binomially), i.e. with
    # probability ~1e-5 per query fewer than k keys score above it.  Nothing is taken on trust: a query with fewer than k candidates
    # above its threshold is reported like an overflowing one and searched again with every probed list in an exact threshold pass.
    S = ix.threshold_sample if (dense < nprobe and ix.ntotal / max(ix.nlist, 1) * dense >= ix.sample_min_keys_per_k * k) else 1
    rank = k if S == 1 else max(1, min(k, -(-k // S) + int(np.ceil(ix.sample_sigmas * np.sqrt(k * (S - 1)) / S))))
    if fold is None:
        fold = bool(ix.has_vals and int8 and k <= 1024 and ix.select)
    return SearchPlan(k, nprobe, dense, cap, ccap, query_block, qb, S, rank, fold, ix.select)


# The buffers every route's rounds work on, for one block of queries (``IVFPQIndex._block_begin``): qr [nq, d] = R q; cs [nq, nlist] =
# <q', c_l>; pv, pi [nq, nprobe] the probed lists' bias and ids, best first (-1: none); lut [nq, M * 256] the ADC tables and, on the int8
# route, tables = (qlut [nq, 2, 256, 32] u8, qmeta [nq, 4] f32), their byte image; cv, ci [nq, ccap] the scores and payloads of the
# thresholded round's candidates, cc [nq] how many (zeroed).  With the fused coarse step (``choose_coarse``) cs is None: no such matrix exists
_Block = namedtuple("_Block", "qr cs pv pi lut tables cv ci cc")


class _Outcome(NamedTuple):
    """What one pass over a batch (or a block of it: ``rows``) leaves behind."""
    val: torch.Tensor                # [n, k] scores, descending
    idx: torch.Tensor                # [n, k] payloads as the index carries them, or ids if `split`
    labels: Optional[torch.Tensor]   # [n, k] int32 if `split` and the caller wants the labels
    split: bool                      # the final selection has split the payloads already (``_deliver`` must not)
    over: Optional[torch.Tensor] = None   # [n] survivor counts to hold against the capacity (None: no thresholded round ran)

    def rows(self, lo, hi):
        return self._replace(val=self.val[lo:hi], idx=self.idx[lo:hi], labels=None if self.labels is None else self.labels[lo:hi])


class _PendingSearch:
    """Handle of ``IVFPQIndex.search_begin``."""

    def __init__(self, index, q, k, query_block, return_vals):
        self.index, self.q, self.k, self.query_block, self.return_vals = index, q, k, query_block, return_vals
        # of the latest pass over the whole call (``IVFPQIndex._run``): its work counters (index.stats once the search has finished),
        # the survivor capacity its buffers were allocated with, its outcome
        self.stats = self.cap = self.out = None
        self.worst = self.ev = None                      # the first pass's worst survivor count on its way to pinned memory, the event behind it
        self._result = None

    def result(self):
        if self._result is None:
            self._result = self.index._finish(self)
        return self._result


class IVFPQIndex:
    """faiss ``search`` contract: ``search(queries [n, d] f32, k) -> (scores [n, k] descending, ids [n, k], -1 padded)``."""

    UNDERFLOW = 1 << 30      # "survivor count" of a query whose sampled threshold left fewer than k candidates: searched again like an overflow
    COLUMNS = (1 << 30) - 1  # ... of a query with more candidates than the selection has columns (a larger survivor capacity would not help it)
    LABEL_BITS = 24                                                          # payload = id << 24 | label (ids < 2^39, labels < 2^24)
    # What the int8 search's kernels expect of the buffers allocated here: csrc/ivfpq8_layout.h by value (tests/test_ivfpq8_layout_cpu.py
    # holds the two sides together)
    QG = 8                       # queries per group of the scan's task table
    HIST_BINS = 1024             # threshold pass: counters per (query, list) histogram
    CNT_STRIDE = 16              # int32 per survivor counter: one 64-byte line each (column 0 counts)
    WORK_CTR_SHAPE = (8, 16)     # the persistent workgroups' group counters: one 64-byte line per XCD
    QLUT_SHAPE = (2, 256, 32)    # a query's byte table [half][code][slot]
    QMETA = 4                    # ... and its {delta, sum_lo, absmax, 0}
    SURV_ROW_BITS, SURV_LIST_BITS = 19, 18   # a survivor record holds the row inside its list and the list

    @classmethod
    def n_groups_cap(cls, nq, P, nlist):
        """rows gnnlm_ivfpq_build_groups needs for nq queries with P probes each: every list's last group may be partly filled"""
        return nq * P // cls.QG + nlist + 1

    def __init__(self, R, coarse, pq, list_off, list_ids, list_codes, nprobe=32, cosine=True, dense_probes=None, cand_cap=None,
                 score_bytes=6 << 30, scan=None, metric="ip", list_term_bytes=4 << 30, coarse_route=None):
        self.R, self.coarse, self.pq = R, coarse, pq                         # [d, d], [nlist, d], [M, 256, dsub]  f32
        self.list_off, self.list_ids, self.list_codes = list_off, list_ids, list_codes   # i64 [nlist+1], i64 [N], u8 [N, M]
        self.nprobe, self.cosine, self.dense_probes, self.cand_cap = nprobe, cosine, dense_probes, cand_cap
        self._given = dict(dense_probes=dense_probes, cand_cap=cand_cap, scan=scan, list_term_bytes=list_term_bytes, coarse_route=coarse_route)   # as passed (``add``)
        self.threshold_sample = 4                # every S-th tile of the threshold lists is histogrammed (1: all of them -- see plan_search)
        self.sample_min_keys_per_k = 64          # ... when the threshold lists hold at least this many keys per neighbour asked for
        self.sample_sigmas = 4.5                 # margin of the sample's rank (tests lower it to force the verification to fail)
        self.sample_fail_frac = 0.01             # more failing queries than this in a batch: the index stops sampling
        self.score_bytes = score_bytes                                       # budget of the dense round's score rows per query block
        self.payload, self.has_vals, self.val_last = list_ids, False, 0      # what a candidate carries through the selection
        self.device = R.device
        if metric not in ("ip", "l2") or (metric == "l2" and cosine):
            raise ValueError("IVFPQIndex: metric is 'ip' (cosine: inner product of normalised vectors) or 'l2'")
        self.metric = metric
        self.d, self.nlist = coarse.shape[1], coarse.shape[0]
        self.M, _, self.dsub = pq.shape
        self.ntotal = list_ids.shape[0]
        self.list_len = list_off[1:] - list_off[:-1]
        self.max_list = int(self.list_len.max().item()) if self.nlist else 0
        self.route, term = choose_route(self.M, self.ntotal, self.max_list, self.nlist, scan, metric, list_term_bytes)
        # (the argument is `coarse_route`: `coarse` names the centroids)
        self.coarse_route = choose_coarse(self.route, self.nlist, coarse_route)
        if self.coarse_route == "fused" and (self.route == "int8" or self.d % 4):
            if coarse_route == "fused":
                raise ValueError("IVFPQIndex: coarse_route='fused' needs a float32 route (scan='f32' / 'rowmajor') and d % 4 == 0")
            self.coarse_route = "dense"
        self.packed_codes = self.tiles = self.list_term = self.key_term = None
        if metric == "l2":
            # squared distances with residual codes: |q' - c_l - r|^2 = |q' - c_l|^2 + sum_m (T[l][m][code] - 2 <q'_m, p_mc>) with the
            # per-list table T[l][m][c] = |p_mc|^2 + 2 <c_l,m, p_mc> (faiss IndexIVFPQ's precomputed table).  A key's M entries of T add up
            # to a constant of the key, key_term = |c_l + r|^2 - |c_l|^2 (gnnlm_ivfpq_key_terms): with that one float per key the tables
            # are the query's own, as for the inner product.
            #   M = 64 (the kNN-LM shape): key_term + the packed float32 scan, two rounds (scan="rowmajor": the per-list table below)
            #   T beyond list_term_bytes (nlist * M KiB: many lists): key_term + the row-major scan
            #   otherwise: T itself; the row-major scan adds it to the query's table while it fills LDS (gnnlm_ivfpq_scan, list_term)
            self.coarse_n2 = (coarse ** 2).sum(1).contiguous()
            if term == "list_term":
                cross = torch.einsum("lmd,mcd->lmc", coarse.reshape(self.nlist, self.M, self.dsub), pq)
                self.list_term = ((pq ** 2).sum(2)[None] + 2.0 * cross).reshape(self.nlist, self.M * 256).contiguous()
            elif term == "key_term":
                self.key_term = ops.ivfpq_key_terms(list_codes, list_off, coarse, pq)
        if self.route == "int8":
            self.tiles = ops.ivfpq_pack_tiles(self.list_codes)
        elif self.route == "packed":
            self.packed_codes = torch.empty(-(-self.ntotal // 64) * 64 * self.M, dtype=torch.uint8, device=self.device)
            _lib.call("gnnlm_ivfpq_pack_codes", _lib.ptr(self.list_codes), self.ntotal, self.M, _lib.ptr(self.packed_codes), _lib.stream())
        # lists per query behind the threshold: the float32 dense round scores 2 in full; the int8 threshold pass is cheap and its
        # bound a little loose, 6 lists give the tighter threshold (fewer survivors to re-score) for less time
        if self.dense_probes is None:
            self.dense_probes = 6 if self.route == "int8" else 2
        # records per query: the int8 filter's SURVIVORS (8 bytes each; a sampled threshold lets ~8 k of them through on average and twice that
        # where list lengths vary: 32768 keeps the re-searches of overflowing queries rare), the float32 scan's candidates
        if self.cand_cap is None:
            self.cand_cap = 32768 if self.route == "int8" else 16384
        self.refine_tau = True                   # the threshold refinement inside the re-score's launch (False: the re-score alone, tests)
        self.keep_candidates, self.last_candidates = False, None             # tests / debugging: (cv, ci, cc, tau) of the last block's thresholded round
        self._side_streams = {}                                              # raw stream -> its side stream
        self._worst_host, self._worst_next = None, 0                         # pinned landing slots (``_landing_slot``), pinned with the first search
        self.stats = {}                                                      # device-side work counters of the last search that finished (bench.py)

    def attach_vals(self, vals):
        """Carry the keys' labels with the index: payload[r] = id << 24 | vals[id] for the key at list position r (the reference
        reads ``self.vals[knns]`` after the search, knn/knn_model.py:198: k random 4-byte reads per query).  ``vals``: the
        datastore's label table on the device ([N] or [N, 1], int16 / int32); -1 ids of the result read ``vals[-1]`` as numpy's
        wrap-around does there."""
        v = vals.reshape(-1).to(self.device)
        if self.ntotal == 0:
            return self
        if int(v.max().item()) >= (1 << self.LABEL_BITS) or int(v.min().item()) < 0 or int(self.list_ids.max().item()) >= (1 << (63 - self.LABEL_BITS)):
            raise ValueError("attach_vals: labels must fit 24 bits and key ids 39 bits")
        self.payload = (self.list_ids << self.LABEL_BITS) | v[self.list_ids].to(torch.int64)
        self.has_vals, self.val_last = True, int(v[-1].item())
        return self

    @classmethod
    def build(cls, keys, nlist, M, device="cuda", cosine=True, nprobe=32, iters=10, train_size=262144, seed=0, chunk=1 << 18,
              opq_iters=0, metric="ip", d_out=None, **kw):
        """The offline producer: train and add every key (``ivfpq_train.build_arrays``), then the index over those arrays.
        ``d_out`` < d: a reducing rotation R [d_out, d] (the ``OPQ16_64`` block of the One Billion Word recipe)."""
        arrays = ivfpq_train.build_arrays(keys, nlist, M, device, cosine, iters, train_size, seed, chunk, opq_iters, metric, d_out)
        return cls(*arrays, nprobe=nprobe, cosine=cosine, metric=metric, **kw)

    @classmethod
    def train(cls, keys, nlist, M, device="cuda", cosine=True, nprobe=32, iters=10, train_size=262144, seed=0, opq_iters=0, metric="ip",
              chunk=1 << 18, d_out=None, **kw):
        """A trained index without keys (``ntotal == 0``; the reference's ``IndexBuilder.train`` and its ``faiss_store.trained.*``
        file, knn/index_builder.py:66-95): it saves, loads and takes keys with ``add``; searching it is not supported."""
        device = torch.device(device)
        R, coarse, pq = ivfpq_train.train(keys, nlist, M, device, cosine, iters, train_size, seed, chunk, opq_iters, metric, d_out)
        return cls(R, coarse, pq, *ivfpq_train.empty_lists(nlist, M, device), nprobe=nprobe, cosine=cosine, metric=metric, **kw)

    def add(self, keys, ids=None, chunk=1 << 18):
        """A NEW index that holds this one's keys and ``keys`` [n, d] (numpy array, memmap or torch tensor, fp16 / f32, read chunk by
        chunk) under ``ids`` (default ntotal .. ntotal + n - 1: the reference's ``add_with_ids(keys, np.arange(start, end))``,
        knn/index_builder.py:97-109), with this one's settings; nothing is retrained and this index is left as it is.  New keys go
        behind the old keys of their lists (``ivfpq_train.add_rows``).  Labels are not carried over: ``attach_vals`` with the grown
        table."""
        n = keys.shape[0]
        if keys.ndim != 2 or keys.shape[1] != self.R.shape[1]:
            raise ValueError(f"add: keys [n, {self.R.shape[1]}], got {tuple(keys.shape)}")
        if ids is None:
            ids = torch.arange(self.ntotal, self.ntotal + n, dtype=torch.int64, device=self.device)
        else:
            ids = torch.as_tensor(ids if isinstance(ids, torch.Tensor) else np.asarray(ids)).to(self.device, torch.int64).contiguous()
            if ids.shape != (n,):
                raise ValueError("add: one id per key")
        arrays = ivfpq_train.add_rows(self.R, self.coarse, self.pq, self.list_off, self.list_ids, self.list_codes, keys, ids,
                                      self.cosine, self.metric, chunk, self._given["coarse_route"])
        return self._with_lists(arrays)

    def _with_lists(self, arrays):
        """a NEW index over (list_off, list_ids, list_codes) with this one's trained part and settings: the constructor derives the
        tiles, packed codes and key terms again"""
        return type(self)(self.R, self.coarse, self.pq, *arrays, nprobe=self.nprobe, cosine=self.cosine, score_bytes=self.score_bytes,
                          metric=self.metric, **self._given)

    def remove(self, ids=None, ranges=None):
        """A NEW index without the keys whose ids are among ``ids`` (numpy / torch, any order, duplicates allowed) or inside one of
        ``ranges`` (half-open (lo, hi) pairs: a document is one range) -- faiss's ``remove_ids``; this index is left as it is.  Ids
        are datastore rows: the ids of the remaining keys and the label table do not change, ids the index does not hold are no
        error, ``self.ntotal - new.ntotal`` keys were removed.  The result is, bit for bit, what ``add`` of the surviving keys in
        their order would have built (``ivfpq_train.remove_rows``).  Removing everything gives the ``ntotal == 0`` state of
        ``train``.  Labels are not carried over: ``attach_vals`` again."""
        rg = ivfpq_train.normalize_ranges(ids, ranges, self.device)
        return self._with_lists(ivfpq_train.remove_rows(self.list_off, self.list_ids, self.list_codes, rg))

    def merge(self, other):
        """A NEW index that holds this one's keys and ``other``'s (faiss's ``merge_from``): per list this one's rows, then the
        other's -- what ``self.add(other's keys, other's ids)`` builds, without encoding anything.  Both must share one trained part
        (``R``, ``coarse``, ``pq`` equal, the same ``cosine`` / ``metric``) and one device, else ``ValueError``.  As in ``add``,
        ids present in both are NOT checked: such a key is then held twice.  Labels are not carried over: ``attach_vals`` again."""
        if not isinstance(other, IVFPQIndex) or other.device != self.device:
            raise ValueError("merge: both indexes live on one device")
        if (self.cosine, self.metric) != (other.cosine, other.metric):
            raise ValueError("merge: the indexes differ in cosine / metric")
        for name in ("R", "coarse", "pq"):
            a, b = getattr(self, name), getattr(other, name)
            if a.shape != b.shape or not torch.equal(a, b):
                raise ValueError(f"merge: the indexes were trained differently ({name} differs)")
        return self._with_lists(ivfpq_train.merge_lists(self.list_off, self.list_ids, self.list_codes,
                                                        other.list_off, other.list_ids, other.list_codes))

    def replace(self, keys, ids):
        """``remove(ids=ids).add(keys, ids)``: new keys under ids the index may already hold (a corrected document)"""
        return self.remove(ids=ids).add(keys, ids)

    def save(self, path):
        arrays = dict(R=self.R, coarse=self.coarse, pq=self.pq, list_off=self.list_off, list_ids=self.list_ids, list_codes=self.list_codes)
        np.savez(path, **{k: t.cpu().numpy() for k, t in arrays.items()}, meta=np.array([self.nprobe, int(self.cosine), int(self.metric == "l2")]))

    @classmethod
    def load(cls, path, device="cuda", **kw):
        z = np.load(path)
        t = lambda k: torch.from_numpy(z[k]).to(device)
        kw.setdefault("nprobe", int(z["meta"][0]))
        kw.setdefault("metric", "l2" if len(z["meta"]) > 2 and z["meta"][2] else "ip")
        return cls(t("R"), t("coarse"), t("pq"), t("list_off"), t("list_ids"), t("list_codes"), cosine=bool(z["meta"][1]), **kw)

    @classmethod
    def from_faiss_file(cls, path, device="cuda", cosine=True, **kw):
        """The reference's own index file (``faiss.write_index`` of ``OPQ64_1024,IVF4096,PQ64``, knn/index_builder.py:79-150;
        ``--index-file``) read without faiss (faiss_io.read_ivfpq_index) -- inner-product indexes with residual codes."""
        from . import faiss_io
        z = faiss_io.read_ivfpq_index(path)
        if z["metric"] != z["coarse_metric"] or not z["by_residual"]:
            raise ValueError(f"{path}: the on-device search covers IVF-PQ with residual codes whose coarse quantizer has the index's "
                             f"metric (what knn/index_builder.py builds), found metric={z['metric']} coarse={z['coarse_metric']} "
                             f"by_residual={z['by_residual']}")
        kw.setdefault("metric", z["metric"])
        if z["metric"] == "l2":
            cosine = False
        d = z["coarse"].shape[1]
        R = z["R"] if z["R"] is not None else np.eye(d, dtype=np.float32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        kw.setdefault("nprobe", z["nprobe"])
        return cls(t(R), t(z["coarse"]), t(z["pq"]), t(z["list_off"]), t(z["list_ids"]), t(z["list_codes"]), cosine=cosine, **kw)

    # ------------------------------------------------------------------------------------------ a search: begin, finish, repair
    def search(self, queries, k):
        d, i = self.search_device(torch.as_tensor(np.asarray(queries)), k)
        return d.cpu().numpy(), i.cpu().numpy()

    def search_device(self, q, k, query_block=None, return_vals=False):
        """The search, on device tensors: (scores [n, k] descending, ids [n, k], -1 padded[, vals [n, k] int32 with
        ``attach_vals``]).  The thresholded round keeps at most ``cand_cap`` survivors per query; the survivor counts are read
        back once per call (the only host sync).  Queries with more (a query whose dense lists hold fewer than k keys has no
        threshold) are searched again on their own with every probed list scored in full; if many overflow, the capacity is
        doubled for good and the call repeated."""
        return self.search_begin(q, k, query_block, return_vals).result()

    def search_begin(self, q, k, query_block=None, return_vals=False):
        """Enqueue the search and return a handle; ``handle.result()`` waits for the SEARCH only (an event behind its last kernel, the
        worst survivor count on its way to pinned memory) and returns what ``search_device`` returns.  Work enqueued between the two
        calls (the language model's softmax, which does not depend on the neighbours) keeps the device busy while the host looks at
        the count and enqueues what follows: no pipeline bubble behind the search's one host round trip."""
        h = _PendingSearch(self, q.to(self.device, torch.float32).contiguous(), k, query_block, return_vals)
        self._run(h, self.cand_cap)
        if h.out.over is not None:
            h.worst = self._landing_slot()
            h.worst.copy_(h.out.over.max().reshape(1), non_blocking=True)
            h.ev = torch.cuda.Event()
            h.ev.record()
        return h

    def _landing_slot(self):
        """one of 8 pinned ints, one per search in flight (a ring)"""
        if self._worst_host is None:
            self._worst_host = torch.empty(8, dtype=torch.int32).pin_memory()
        slot = self._worst_host[self._worst_next:self._worst_next + 1]
        self._worst_next = (self._worst_next + 1) % 8
        return slot

    def _plan(self, k, dense_probes, cap, query_block=None, fold=None):
        ix = SearchNumbers(self.route, self.nprobe, self.nlist, self.ntotal, self.max_list, self.score_bytes, self.has_vals,
                           self.threshold_sample, self.sample_min_keys_per_k, self.sample_sigmas,
                           # GNNLM_IVF_SELECT=0: the selections by gnnlm_topk_merge and the split pass of their own, as before csrc/ivfpq_select.hip (A/B runs)
                           os.environ.get("GNNLM_IVF_SELECT", "1") != "0", int(os.environ.get("GNNLM_IVF_QUERY_BLOCK", "32768")))
        return plan_search(ix, k, dense_probes, cap, query_block, fold)

    def _run(self, h, cap):
        """One pass over the whole call with `cap` records per query (not self.cand_cap: another search in flight may have raised it
        since), under the index's settings as they are now; the handle's counters describe this pass alone."""
        h.cap, h.stats = cap, _LazyStats(pairs=0, survivors=0, candidates=0, queries=h.q.shape[0], M=self.M, requeried=0)
        h.out = self._search_once(h.q, self._plan(h.k, self.dense_probes, cap, h.query_block), h.stats, h.return_vals)

    def _finish(self, h):
        n = h.q.shape[0]
        while h.out.over is not None:
            if h.ev is not None:
                h.ev.synchronize()
                if int(h.worst[0]) <= h.cap:
                    break
                h.ev = None
            over = h.out.over
            bad = (over > h.cap).nonzero().reshape(-1)                        # host sync
            if bad.numel() == 0:
                break
            n_under = int((over[bad] >= self.UNDERFLOW).sum().item())
            n_cols = int((over[bad] == self.COLUMNS).sum().item())            # too many CANDIDATES for the selection's columns: searched again one by one
            if n_under > self.sample_fail_frac * n and self.threshold_sample > 1:   # the sample does not stand for its lists on this data: stop sampling
                self.threshold_sample = 1
                self._run(h, h.cap)
            elif (bad.numel() - n_under - n_cols) * 8 > n and h.cap < (1 << 18):
                self.cand_cap = max(self.cand_cap, 2 * h.cap)
                self._run(h, 2 * h.cap)
            else:
                self._search_rows_again(h, bad)
                break
        self.stats = h.stats
        return self._deliver(h)

    def _search_rows_again(self, h, bad):
        """Rows `bad` of the handle's outcome, searched on their own with every probed list in the threshold / dense round and written
        over their rows (the counters describe the main pass: the re-search's go to a throw-away set)."""
        out, sub, cap = h.out, h.q[bad].contiguous(), h.cap
        while True:
            again = self._search_once(sub, self._plan(h.k, self.nprobe, cap, h.query_block, fold=out.split), _LazyStats(), h.return_vals)
            if again.over is None or int(again.over.max().item()) <= cap:
                break
            if cap >= (1 << 22):                                              # survivors beyond the capacity would be dropped silently
                raise _lib.GnnlmError(f"ivfpq search: {int(again.over.max().item())} survivors of one query exceed the largest candidate "
                                      f"capacity ({cap}); lower k / nprobe or search this index with scan='f32'")
            cap *= 2
        out.val[bad], out.idx[bad] = again.val, again.idx
        if out.labels is not None:
            out.labels[bad] = again.labels
        h.stats.set("requeried", int(bad.numel()))

    def _deliver(self, h):
        """the outcome as ``search_device`` returns it: distances for L2, payloads split into (id, label) if nobody has yet"""
        val, idx, rv = h.out.val, h.out.idx, h.return_vals
        if self.metric == "l2":
            val = -val                                                        # scores are -distance: squared distances, ascending, +inf padded
        if not self.has_vals:
            return (val, idx, None) if rv else (val, idx)
        if h.out.split:                                                       # the final selection stored (id, label) itself: no pass over [n, k]
            return (val, idx, h.out.labels) if rv else (val, idx)
        # payload -> (id in place, label): one pass (gnnlm_ivfpq_split_payload) instead of five elementwise torch kernels over [n, k]
        vals = torch.empty(idx.shape, dtype=torch.int32, device=idx.device) if rv else None
        _lib.call("gnnlm_ivfpq_split_payload", _lib.ptr(idx), idx.numel(), self.LABEL_BITS, self.val_last, _lib.ptr(vals), _lib.stream())
        return (val, idx, vals) if rv else (val, idx)

    # ------------------------------------------------------------------------------------------ one pass: blocks of queries
    def _search_once(self, q, plan, stats, return_vals=False):
        n, dev = q.shape[0], self.device
        val = torch.empty(n, plan.k, device=dev, dtype=torch.float32)
        idx = torch.empty(n, plan.k, device=dev, dtype=torch.int64)
        labels = torch.empty(n, plan.k, dtype=torch.int32, device=dev) if plan.fold and return_vals else None
        out, over = _Outcome(val, idx, labels, plan.fold), None
        block = self._block_int8 if self.route == "int8" else self._block_f32
        # the fused coarse step takes the whole batch at once (nothing of it is [queries, nlist]-sized, and a workgroup's first chunks
        # of a slab are its dearest: one call over 8192 queries takes half the time of eight over 1024)
        pre = self._coarse_fused(plan, q) if self.coarse_route == "fused" else None
        for q0 in range(0, n, plan.qb):
            blk = self._block_begin(plan, q[q0:q0 + plan.qb], stats, None if pre is None else tuple(t[q0:q0 + plan.qb] for t in pre))
            o = block(plan, blk, out.rows(q0, q0 + plan.qb), stats)
            if o is not None:
                over = o if over is None else torch.cat([over, o])
        return out._replace(over=over)

    def _coarse_fused(self, plan, q):
        """rotation and coarse step of a whole batch without its [n, nlist] scores -> (qr [n, d], pv, pi [n, nprobe]) as a block holds them"""
        qr = ops.gemm_nt(q, self.R)
        pv = torch.empty(q.shape[0], plan.nprobe, device=self.device, dtype=torch.float32)
        pi = torch.empty(q.shape[0], plan.nprobe, device=self.device, dtype=torch.int64)
        ops.ivfpq_coarse_probes(qr, self.coarse, pv, pi, -0.5 * self.coarse_n2 if self.metric == "l2" else None)
        if self.metric == "l2":
            pv = (2.0 * pv - (qr ** 2).sum(1, keepdim=True)).contiguous()      # the list's bias: -|q' - c_l|^2
        return qr, pv, pi

    def _block_begin(self, plan, qs, stats, pre=None):
        """``pre``: the block's rows of ``_coarse_fused`` (the fused coarse route); None: rotation and coarse step of this block here"""
        dev, nq = self.device, qs.shape[0]
        qr = ops.gemm_nt(qs, self.R) if pre is None else pre[0]                 # q' = R q
        # the ADC tables (a store-bound batched GEMM, 2 KB per query and sub-quantizer) and their 8-bit images depend on q' alone: they
        # are built on a side stream beside the coarse scores / probe selection / task table of this stream
        lut, tables, side = self._tables_begin(qr)
        # <q', c_l> and the nprobe best lists, best first; the fused coarse step has done both without the [nq, nlist] matrix
        if pre is not None:
            cs, pv, pi = None, pre[1], pre[2]
        elif self.coarse_route == "fused":
            cs, (_, pv, pi) = None, self._coarse_fused(plan, qs)
        else:
            cs = ops.gemm_nt(qr, self.coarse)
            pv = torch.empty(nq, plan.nprobe, device=dev, dtype=torch.float32)
            pi = torch.empty(nq, plan.nprobe, device=dev, dtype=torch.int64)
            if self.metric == "l2":                                             # the nprobe NEAREST lists: argmax <q', c> - |c|^2 / 2
                self._select_probes(plan, cs, pv, pi, col_bias=-0.5 * self.coarse_n2)
                pv = (2.0 * pv - (qr ** 2).sum(1, keepdim=True)).contiguous()  # the list's bias: -|q' - c_l|^2
            else:
                self._select_probes(plan, cs, pv, pi)                           # the nprobe best lists, best first
        stats.add("pairs", lambda pi=pi: self.list_len[pi.clamp(min=0)].masked_fill(pi < 0, 0).sum().double())
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)                       # (lut / tables were allocated on THIS stream: no record_stream needed)
        cv = torch.empty(nq, plan.ccap, device=dev, dtype=torch.float32)
        ci = torch.empty(nq, plan.ccap, device=dev, dtype=torch.int64)
        cc = torch.zeros(nq, device=dev, dtype=torch.int32)
        return _Block(qr, cs, pv, pi, lut, tables, cv, ci, cc)

    def _block_f32(self, plan, blk, out, stats):
        """The float32 scan ("packed" / "rowmajor"), two rounds; -> the candidate counts of round 2 (None: every list was dense)."""
        dev, nq, k, dense = self.device, blk.pv.shape[0], plan.k, plan.dense
        bv, bi, pi = out.val, out.idx, blk.pi
        lut_s = blk.lut
        if self.route == "packed":
            lut_s = torch.empty_like(blk.lut)
            _lib.call("gnnlm_ivfpq_pack_lut", _lib.ptr(blk.lut), blk.lut.stride(0), nq, self.M, _lib.ptr(lut_s), _lib.stream())
        # round 1: the best `dense` lists of every query, every score
        ov = torch.empty(nq, dense * self.max_list, device=dev, dtype=torch.float32)
        self._scan(lut_s, blk, 0, dense, out=ov)
        ops.topk_merge(ov, bv, bi, largest=True, init=True)                     # ids = columns of ov
        # the columns kept -> payloads: column = probe slot * max_list + position in the list (-inf: beyond a list)
        lst = torch.gather(pi, 1, torch.div(bi, self.max_list, rounding_mode="floor").clamp_(0, dense - 1))
        pos = self.list_off[lst.clamp(min=0)] + bi % self.max_list
        bi.copy_(torch.where(torch.isinf(bv) | (lst < 0), torch.full_like(bi, -1), self.payload[pos.clamp_(0, max(self.ntotal - 1, 0))]))
        if plan.nprobe <= dense:
            return None
        # round 2: the other lists only emit scores above the query's k-th best so far
        tau = torch.where(bi[:, k - 1] >= 0, bv[:, k - 1], torch.full_like(bv[:, k - 1], float("-inf"))).contiguous()
        self._scan(lut_s, blk, dense, plan.nprobe, filt=(tau, plan.cap))
        stats.add("candidates", lambda cc=blk.cc: cc.sum().double())
        if self.keep_candidates:
            self.last_candidates = (blk.cv, blk.ci, blk.cc, tau)
        ops.topk_merge(blk.cv, bv, bi, ids=blk.ci, largest=True, init=False, row_ncols=blk.cc.clamp(max=plan.cap))
        return blk.cc

    def _block_int8(self, plan, blk, out, stats):
        """M = 64: everything on the int8 matrix cores (csrc/ivfpq8_prep.hip, ivfpq8_scan.hip, ivfpq8_rescore.hip).  (1) threshold pass: histograms of the integer sums of the
        first `dense` lists (a sample of them: plan.S) -> a lower bound tau of the query's k-th best score (no per-key output, no
        selection); (2) filter: every probed list, keys whose integer sum can reach tau; (3) exact float32 scores of the survivors,
        score > tau -> candidates; (4) one k-selection over the candidates.  -> the survivor counts to hold against plan.cap."""
        dev, nq, pi, cc = self.device, blk.pv.shape[0], blk.pi, blk.cc
        hist = torch.empty(nq, plan.dense, self.HIST_BINS, device=dev, dtype=torch.int32)   # per (query, list): sum_u >> 4 counted on the device
        self._scan8(blk.tables, blk.cs, self._groups(pi[:, :plan.dense], seg=self.HIST_BINS), hist=hist, stride=plan.S)
        tau = self._tau(plan, blk, hist)
        surv = torch.empty(nq, plan.cap, 2, device=dev, dtype=torch.int32)
        sc16 = torch.zeros(nq, self.CNT_STRIDE, device=dev, dtype=torch.int32)   # one 64-byte line per counter (column 0)
        g2 = self._groups(pi)
        stats.add("groups", lambda g=g2[2]: g[0].double())
        self._scan8(blk.tables, blk.cs, g2, filt=(tau, surv, sc16))
        sc = sc16[:, 0]
        self._rescore(plan, blk, (tau, surv, sc16), stats)
        stats.add("survivors", lambda sc=sc: sc.sum().double())
        stats.add("candidates", lambda cc=cc: cc.sum().double())
        if self.keep_candidates:
            self.last_candidates = (blk.cv, blk.ci, cc, tau)
        self._select_final(plan, blk, out)
        over = sc                                                             # every candidate is a survivor: sc >= cc
        if plan.ccap < plan.cap:                                              # more candidates than columns: an overflow like any other
            over = torch.where(cc > plan.ccap, torch.full_like(sc, self.COLUMNS), over)
        if plan.S > 1:                                                        # the sampled threshold's proof: k candidates above it (or every key there is)
            avail = self.list_len[pi.clamp(min=0)].masked_fill(pi < 0, 0).sum(1)
            short = cc.to(torch.int64) < avail.clamp(max=plan.k)
            stats.add("underflow", lambda short=short: short.sum().double())
            over = torch.where(short, torch.full_like(sc, self.UNDERFLOW), over)
        return over

    # ------------------------------------------------------------------------------------------ one function per descriptor
    def _select_probes(self, plan, cs, pv, pi, col_bias=None):
        """the nprobe best lists of every query, best first (csrc/ivfpq_select.hip); shapes it does not take go to gnnlm_topk_merge"""
        ops.ivfpq_select_probes(cs, pv, pi, col_bias, plan.select)

    def _tables_begin(self, qr):
        """lut[q][m][c] = <q'_m, p_mc> (M small GEMMs) and, for the int8 filter, its byte image: enqueued on a side stream of the
        current one when the filter will run (the caller joins before the first consumer).  -> (lut, (qlut, qmeta) | None, side | None)"""
        nq, dev = qr.shape[0], self.device
        lut = torch.empty(nq, self.M * 256, device=dev, dtype=torch.float32)
        tables = side = None
        if self.route == "int8":
            tables = (torch.empty(nq, *self.QLUT_SHAPE, dtype=torch.uint8, device=dev), torch.empty(nq, self.QMETA, dtype=torch.float32, device=dev))
            if not torch.cuda.is_current_stream_capturing():
                cur = torch.cuda.current_stream()
                side = self._side_streams.get(cur.cuda_stream)
                if side is None:
                    side = self._side_streams[cur.cuda_stream] = torch.cuda.Stream(device=dev)
                side.wait_stream(cur)
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            if tables is not None and self.dsub in (4, 8, 16, 32):
                t = _lib.gnnlm_ivfpq_tables_t()
                t.qr, t.ld_qr, t.n, t.pq, t.M, t.dsub = qr.data_ptr(), qr.stride(0), nq, self.pq.data_ptr(), self.M, self.dsub
                t.lut, t.ld_lut, t.qlut, t.qmeta = lut.data_ptr(), lut.stride(0), tables[0].data_ptr(), tables[1].data_ptr()
                _lib.call_desc("gnnlm_ivfpq_tables", t)
                return lut, tables, side
            g = _lib.gnnlm_gemm_t()
            g.A, g.lda, g.W, g.ldw, g.C, g.ldc = qr.data_ptr(), qr.stride(0), self.pq.data_ptr(), self.dsub, lut.data_ptr(), self.M * 256
            g.M, g.N, g.K, g.batch1 = nq, 256, self.dsub, self.M
            g.sA1, g.sW1, g.sC1 = self.dsub, 256 * self.dsub, 256
            _lib.call_desc("gnnlm_gemm_nt", g)
            if tables is not None:
                _lib.call("gnnlm_ivfpq_quantize_lut", _lib.ptr(lut), lut.stride(0), nq, self.M, _lib.ptr(tables[0]), _lib.ptr(tables[1]), _lib.stream())
        return lut, tables, side

    def _scan(self, lut, blk, p_lo, p_hi, out=None, filt=None):
        """gnnlm_ivfpq_scan over probe slots p_lo..p_hi of a block.  ``out``: every score, [nq, (p_hi - p_lo) * max_list];
        ``filt`` = (tau, cap): scores above tau into the block's candidate buffers."""
        pl = blk.pi[:, p_lo:p_hi]
        # tasks grouped by list (bookkeeping on the device, no host round trip): concurrent workgroups share code rows
        order = torch.sort(pl.reshape(-1), stable=True).indices
        task_q = torch.div(order, p_hi - p_lo, rounding_mode="floor").to(torch.int32)
        task_p = (order % (p_hi - p_lo) + p_lo).to(torch.int32)
        s = _lib.gnnlm_ivfpq_scan_t()
        s.codes, s.ids, s.list_off, s.M = self.list_codes.data_ptr(), self.payload.data_ptr(), self.list_off.data_ptr(), self.M
        if self.route == "packed":
            s.codes, s.packed = self.packed_codes.data_ptr(), 1                 # `lut` is then the packed table set
        s.lut, s.ld_lut = lut.data_ptr(), lut.stride(0)
        s.probe_list, s.probe_bias, s.ld_probe = blk.pi.data_ptr(), blk.pv.data_ptr(), blk.pi.stride(0)
        s.task_q, s.task_p, s.n_tasks = task_q.data_ptr(), task_p.data_ptr(), order.numel()
        if self.list_term is not None:
            s.list_term, s.ld_list_term = self.list_term.data_ptr(), self.list_term.stride(0)
        if self.key_term is not None:
            s.key_term = self.key_term.data_ptr()
        if filt is None:
            s.out_val, s.ld_out, s.p0, s.seg = out.data_ptr(), out.stride(0), p_lo, self.max_list       # scores only (out_id NULL)
        else:
            s.tau, s.cand_val, s.cand_id, s.cand_cnt, s.cap = filt[0].data_ptr(), blk.cv.data_ptr(), blk.ci.data_ptr(), blk.cc.data_ptr(), filt[1]
        _lib.call_desc("gnnlm_ivfpq_scan", s)

    def _groups(self, pl, seg=None):
        """The scan's task table on the device (gnnlm_ivfpq_build_groups: histogram, prefix, scatter -- four small launches instead
        of the ~25 of ``tests/ivfpq_groups_ref.py``, the torch reference of the same table); same tuple."""
        nq, P = pl.shape
        dev = pl.device
        G = self.n_groups_cap(nq, P, self.nlist)
        grp_list = torch.empty(G, dtype=torch.int32, device=dev)
        grp_q = torch.empty(G, self.QG, dtype=torch.int32, device=dev)
        grp_out = torch.empty(G, self.QG, dtype=torch.int64, device=dev) if seg is not None else None
        n_groups = torch.empty(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(2 * (self.nlist + 1), dtype=torch.int32, device=dev)
        _lib.call("gnnlm_ivfpq_build_groups", ctypes.c_void_p(pl.data_ptr()), pl.stride(0), nq, P, self.nlist, seg or 0, _lib.ptr(grp_list),
                  _lib.ptr(grp_q), _lib.ptr(grp_out), _lib.ptr(n_groups), _lib.ptr(scratch), _lib.stream())
        return (grp_list, grp_q, n_groups, G) if seg is None else (grp_list, grp_q, n_groups, G, grp_out)

    def _scan8(self, tables, cs, groups, hist=None, stride=1, filt=None):
        """gnnlm_ivfpq_scan8 over a task table (``_groups``).  ``hist`` (groups with segment offsets): the threshold pass, every
        `stride`-th tile; ``filt`` = (tau, surv, counters): the filter."""
        d = _lib.gnnlm_ivfpq_scan8_t()
        d.sums_stride = stride
        d.tiles, d.list_off, d.M = self.tiles.data_ptr(), self.list_off.data_ptr(), self.M
        d.nlist, d.max_list = self.nlist, self.max_list
        d.qlut, d.qmeta, d.coarse, d.ld_coarse = tables[0].data_ptr(), tables[1].data_ptr(), cs.data_ptr(), cs.stride(0)
        d.grp_list, d.grp_q, d.n_groups, d.max_groups = groups[0].data_ptr(), groups[1].data_ptr(), groups[2].data_ptr(), groups[3]
        ctr = torch.zeros(*self.WORK_CTR_SHAPE, device=self.device, dtype=torch.int32)   # the persistent workgroups' work counters (one per XCD)
        d.work_ctr = ctr.data_ptr()
        if hist is not None:
            d.out_hist, d.grp_out = hist.data_ptr(), groups[4].data_ptr()
        else:
            tau, surv, cnt = filt
            d.tau, d.surv, d.surv_cnt, d.cap = tau.data_ptr(), surv.data_ptr(), cnt.data_ptr(), surv.shape[1]
        _lib.call_desc("gnnlm_ivfpq_scan8", d)

    def _tau(self, plan, blk, hist):
        """histograms of the threshold lists -> tau [nq], the bound of rank plan.rank among the keys counted"""
        tau = torch.empty(hist.shape[0], device=self.device, dtype=torch.float32)
        t = _lib.gnnlm_ivfpq_tau_t()
        t.hist, t.D = hist.data_ptr(), plan.dense
        t.probe_list, t.probe_bias, t.ld_probe = blk.pi.data_ptr(), blk.pv.data_ptr(), blk.pi.stride(0)
        t.qmeta, t.n, t.k, t.tau = blk.tables[1].data_ptr(), hist.shape[0], plan.rank, tau.data_ptr()
        _lib.call_desc("gnnlm_ivfpq_tau", t)
        return tau

    def _rescore(self, plan, blk, filt, stats):
        """exact float32 scores of the filter's survivors; those above tau become the block's candidates"""
        tau, surv, sc16 = filt
        r = _lib.gnnlm_ivfpq_rescore_t()
        r.codes, r.payload, r.M = self.list_codes.data_ptr(), self.payload.data_ptr(), self.M
        r.lut, r.ld_lut, r.coarse, r.ld_coarse, r.tau = blk.lut.data_ptr(), blk.lut.stride(0), blk.cs.data_ptr(), blk.cs.stride(0), tau.data_ptr()
        r.surv, r.surv_cnt, r.cap, r.n = surv.data_ptr(), sc16.data_ptr(), plan.cap, sc16.shape[0]
        r.cand_val, r.cand_id, r.cand_cnt, r.cand_cap = blk.cv.data_ptr(), blk.ci.data_ptr(), blk.cc.data_ptr(), plan.ccap
        if self.refine_tau:
            # inside the re-score's launch: a tighter threshold from the survivors' own integer sums (all lists, un-binned), and only
            # the survivors that can beat it are re-scored
            rc16 = torch.empty_like(sc16)
            r.qmeta, r.k, r.out_cnt = blk.tables[1].data_ptr(), plan.k, rc16.data_ptr()
            stats.add("rescored", lambda rc=rc16: rc[:, 0].sum().double())
        _lib.call_desc("gnnlm_ivfpq_rescore", r)

    def _select_final(self, plan, blk, out):
        """the k best candidates of every query into the outcome's rows: ranked inside value bins (csrc/ivfpq_select.hip), with
        ``out.split`` the payloads leave as (id, label); k beyond 1024 and GNNLM_IVF_SELECT=0 go to gnnlm_topk_merge"""
        cv, ci, ccap = blk.cv, blk.ci, plan.ccap
        if not (plan.k <= 1024 and (out.split or plan.select)):
            return ops.topk_merge(cv, out.val, out.idx, ids=ci, largest=True, init=True, row_ncols=blk.cc.clamp(max=ccap))
        rn = blk.cc.clamp(max=ccap)
        f = _lib.gnnlm_ivfpq_select_final_t()
        f.cand_val, f.ld_val, f.cand_id, f.ld_id = cv.data_ptr(), cv.stride(0), ci.data_ptr(), ci.stride(0)
        f.row_ncols, f.n, f.cap, f.k, f.out_val, f.out_id = rn.data_ptr(), cv.shape[0], ccap, plan.k, out.val.data_ptr(), out.idx.data_ptr()
        if out.split:
            f.label_bits, f.val_last = self.LABEL_BITS, self.val_last
            if out.labels is not None:
                f.out_vals = out.labels.data_ptr()
        _lib.call_desc("gnnlm_ivfpq_select_final", f)
