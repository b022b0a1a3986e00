"""gnnlm_ivfpq_scan at the descriptor level (include/gnnlm.h: gnnlm_ivfpq_scan_t): both code layouts, both modes, the three score
formulas, every M the entry point dispatches differently -- against the float64 restatement of tests/ivfpq_scan_ref.py.
Descriptors are filled by hand and passed to ``_lib.call_desc``; no index is built, the tables are random arrays.

Two bars only: ``ref.bar(M, mag) = (M + 3) * 2^-24 * mag`` (derived in ivfpq_scan_ref.py) for every score against the reference,
and exact equality for everything else (ids, counts, padding, sentinels, bit patterns of the kernel against itself).

Data (ref.make_data): lists of 0, 1, 63, 64, 65, 129, 0, 7, 1100 and 2300 rows, 5 queries, 4 probe slots; the task tables
(ref.task_table over ref.PROBES) hold a -1 slot, pairs of tasks inside one list and across a list boundary, an odd task count and
one that is no multiple of 16 (padded workgroups of the packed kernel's 8-way grid)."""
import functools

import numpy as np
import pytest
import torch

import ivfpq_scan_ref as ref

pytestmark = pytest.mark.gpu

SENT_F_BITS = 0x7FC0BEEF                                                      # a NaN with a payload of its own: compared as bits
SENT_I = -0x0123456789ABCDEF
CASES = [("rowmajor", M, f) for M in (16, 32, 64, 128) for f in ref.FORMULAS] + \
        [("packed", M, f) for M in (32, 64) for f in ("ip", "key_term")]
CASE_IDS = [f"{l}-M{M}-{f}" for l, M, f in CASES]
DENSE_SLOTS = (1, 4)                                                          # p0 = 1, three slots, 15 tasks
ALL_SLOTS = (0, 4)                                                            # 20 tasks


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def host(M):
    return ref.make_data(M)


@functools.lru_cache(maxsize=None)
def task_scores(M, formula):
    """{(q, slot): (scores, mag, rows)} of the reference, computed once."""
    D = host(M)
    return {(q, p): ref.scan_ref(D["codes"], D["list_off"], D["lut"], D["probe_list"], D["probe_bias"], q, p, **ref.formula_terms(D, formula))
            for q in range(D["n"]) for p in range(D["P"])}


def query_scores(M, formula, q, slots):
    parts = [task_scores(M, formula)[(q, p)] for p in range(*slots)]
    return tuple(np.concatenate(x) for x in zip(*parts))


def sentinel_f(shape, dev):
    return torch.from_numpy(np.full(shape, SENT_F_BITS, dtype=np.uint32).view(np.float32)).to(dev)


def sentinel_i(shape, dev):
    return torch.full(shape, SENT_I, dtype=torch.int64, device=dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pack_codes_dev(codes_d, N, M, guard=0):
    from gnnlm_amd import _lib
    size = (N + 63) // 64 * 64 * M
    out = torch.full((size + guard,), 0xAB, dtype=torch.uint8, device=codes_d.device)
    _lib.call("gnnlm_ivfpq_pack_codes", _lib.ptr(codes_d), N, M, _lib.ptr(out), _lib.stream())
    return out


def pack_lut_dev(lut_d, ld, n, M):
    from gnnlm_amd import _lib
    out = torch.empty(n, M * 256, dtype=torch.float32, device=lut_d.device)
    _lib.call("gnnlm_ivfpq_pack_lut", _lib.ptr(lut_d), ld, n, M, _lib.ptr(out), _lib.stream())
    return out


_DEV = {}


def device_data(M, dev):
    """The data set of one M on the device (once per module); the packed image and tables come from the pack kernels."""
    if M not in _DEV:
        D = host(M)
        T = {k: torch.from_numpy(np.ascontiguousarray(D[k])).to(dev) for k in
             ("codes", "ids", "list_off", "lut", "probe_list", "probe_bias", "list_term", "key_term")}
        T["lut"] = T["lut"].reshape(D["n"], M * 256)
        T["list_term"] = T["list_term"].reshape(D["nlist"], M * 256)
        if M in (32, 64):
            T["packed_codes"] = pack_codes_dev(T["codes"], D["N"], M)
            T["packed_lut"] = pack_lut_dev(T["lut"], M * 256, D["n"], M)
        _DEV[M] = T
    return _DEV[M]


class Scan:
    """A descriptor of gnnlm_ivfpq_scan over the data set of M, filled by hand, with the tensors it points to."""

    def __init__(self, dev, layout, M, formula, slots, lut_pad=0, probe_pad=0):
        from gnnlm_amd import _lib
        self.dev, self.M, self.slots = dev, M, slots
        D, T = host(M), device_data(M, dev)
        self.D, self.n = D, D["n"]
        s = self.s = _lib.gnnlm_ivfpq_scan_t()
        s.ids, s.list_off, s.M = T["ids"].data_ptr(), T["list_off"].data_ptr(), M
        lut = T["lut"]
        s.codes = T["codes"].data_ptr()
        if layout == "packed":
            s.codes, s.packed, lut = T["packed_codes"].data_ptr(), 1, T["packed_lut"]
        if lut_pad:                                                           # rows further apart, NaN between them
            wide = sentinel_f((self.n, M * 256 + lut_pad), dev)
            wide[:, :M * 256] = lut
            lut = wide
        pl, pb = T["probe_list"], T["probe_bias"]
        if probe_pad:                                                         # columns the scan must not read: list 3 / NaN
            plw = torch.full((self.n, D["P"] + probe_pad), 3, dtype=torch.int64, device=dev)
            pbw = sentinel_f((self.n, D["P"] + probe_pad), dev)
            plw[:, :D["P"]], pbw[:, :D["P"]] = pl, pb
            pl, pb = plw, pbw
        tq, tp = ref.task_table(D["probe_list"], *slots)
        tq, tp = torch.from_numpy(tq).to(dev), torch.from_numpy(tp).to(dev)
        s.lut, s.ld_lut = lut.data_ptr(), lut.stride(0)
        s.probe_list, s.probe_bias, s.ld_probe = pl.data_ptr(), pb.data_ptr(), pl.stride(0)
        s.task_q, s.task_p, s.n_tasks = tq.data_ptr(), tp.data_ptr(), tq.numel()
        if formula == "list_term":
            s.list_term, s.ld_list_term = T["list_term"].data_ptr(), T["list_term"].stride(0)
        if formula == "key_term":
            s.key_term = T["key_term"].data_ptr()
        self.keep = [lut, pl, pb, tq, tp]

    def call(self):
        from gnnlm_amd import _lib
        _lib.call_desc("gnnlm_ivfpq_scan", self.s)
        torch.cuda.synchronize()

    def dense(self, seg, with_id=False, slack=8):
        """Dense mode over self.slots (p0 = the first slot): out_val [n + 1, n_slots * seg + slack] (the last row belongs to no query)
        and out_id likewise or None, as numpy."""
        s, w = self.s, self.slots[1] - self.slots[0]
        ov = sentinel_f((self.n + 1, w * seg + slack), self.dev)
        oi = sentinel_i((self.n + 1, w * seg + slack), self.dev) if with_id else None
        s.out_val, s.ld_out, s.p0, s.seg = ov.data_ptr(), ov.stride(0), self.slots[0], seg
        if with_id:
            s.out_id = oi.data_ptr()
        self.call()
        return ov.cpu().numpy(), (oi.cpu().numpy() if with_id else None)

    def filtered(self, tau, cap, guard=64):
        """Filtered mode: (cand_val [n, cap], cand_id [n, cap], cand_cnt [n], guard_val, guard_id).  The candidate rows have no stride of
        their own (row q starts at q * cap), so the sentinel columns the rows cannot have lie before the first and behind the last row;
        a write past slot cap - 1 of another row lands in the next query's row, where every slot is checked against that query's
        own survivors."""
        s = self.s
        tau_d = torch.from_numpy(np.asarray(tau, dtype=np.float32)).to(self.dev)
        cv, ci = sentinel_f((guard + self.n * cap + guard,), self.dev), sentinel_i((guard + self.n * cap + guard,), self.dev)
        cc = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        s.tau, s.cap = tau_d.data_ptr(), cap
        s.cand_val, s.cand_id, s.cand_cnt = cv[guard:].data_ptr(), ci[guard:].data_ptr(), cc.data_ptr()
        self.call()
        cv, ci = cv.cpu().numpy(), ci.cpu().numpy()
        mid = slice(guard, guard + self.n * cap)
        return (cv[mid].reshape(self.n, cap), ci[mid].reshape(self.n, cap), cc.cpu().numpy(),
                np.concatenate([cv[:guard], cv[guard + self.n * cap:]]), np.concatenate([ci[:guard], ci[guard + self.n * cap:]]))


def check_dense(M, formula, slots, seg, val, ids, slack=8):
    """Every column of a dense run: scores within the bar, ids exact, the padding beyond the list, the sentinel everywhere else."""
    D = host(M)
    w = slots[1] - slots[0]
    assert val.shape == (D["n"] + 1, w * seg + slack)
    for q in range(D["n"]):
        for p in range(*slots):
            s, mag, rows = task_scores(M, formula)[(q, p)]
            m, c0 = min(len(s), seg), (p - slots[0]) * seg
            err = np.abs(val[q, c0:c0 + m].astype(np.float64) - s[:m])
            print(f"dense M={M} {formula} q={q} slot={p} rows={m}: max err / bar = {float((err / ref.bar(M, mag[:m])).max()) if m else 0.0:.3f}")
            assert (err <= ref.bar(M, mag[:m])).all(), (q, p)
            if ids is None:
                assert np.isneginf(val[q, c0 + m:c0 + seg]).all(), (q, p)     # beyond the list (all of it: -1 slot, empty list)
            else:
                assert np.array_equal(ids[q, c0:c0 + m], D["ids"][rows[:m]]), (q, p)
                assert (ids[q, c0 + m:c0 + seg] == -1).all(), (q, p)          # (out_val beyond the list is unspecified with out_id)
    assert (bits(val[:D["n"], w * seg:]) == SENT_F_BITS).all() and (bits(val[D["n"]]) == SENT_F_BITS).all()    # the kernel wrote nowhere else
    if ids is not None:
        assert (ids[:D["n"], w * seg:] == SENT_I).all() and (ids[D["n"]] == SENT_I).all()


def check_filtered(M, formula, slots, tau, cap, out):
    """cand_cnt counts ALL survivors exactly; the first min(cnt, cap) slots hold distinct (score, id) pairs of the query's true survivor
    set -- all of it when it fits: the id multisets are equal --, each score within the bar of the reference score of its id; the
    slots behind them and the guards still hold the sentinel."""
    D = host(M)
    cv, ci, cc, gv, gi = out
    for q in range(D["n"]):
        s, mag, rows = query_scores(M, formula, q, slots)
        live = s > float(tau[q])
        want = D["ids"][rows[live]]
        assert int(cc[q]) == int(live.sum()), (q, int(cc[q]), int(live.sum()))
        cnt = min(int(cc[q]), cap)
        got = ci[q, :cnt]
        if cnt == len(want):
            assert sorted(got.tolist()) == sorted(want.tolist()), q           # no survivor dropped or doubled
        by_id = {int(i): (v, g) for i, v, g in zip(want, s[live], mag[live])}
        assert len(set(got.tolist())) == cnt and all(int(i) in by_id for i in got), q
        if cnt:
            r, g = np.array([by_id[int(i)] for i in got]).T
            err = np.abs(cv[q, :cnt].astype(np.float64) - r)
            print(f"filtered M={M} {formula} q={q} survivors={int(cc[q])} kept={cnt}: max err / bar = {float((err / ref.bar(M, g)).max()):.3f}")
            assert (err <= ref.bar(M, g)).all(), q
        assert (bits(cv[q, cnt:]) == SENT_F_BITS).all() and (ci[q, cnt:] == SENT_I).all(), q
    assert (bits(gv) == SENT_F_BITS).all() and (gi == SENT_I).all()


# ----------------------------------------------------------------------------------------------------- 1. pack kernels
@pytest.mark.parametrize("M", [32, 64])
@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 3729])
def test_pack_codes_every_byte(dev, M, N):
    codes = host(M)["codes"][:N]
    codes_d = torch.from_numpy(np.ascontiguousarray(host(M)["codes"][:max(N, 1)])).to(dev)       # (N = 0: a valid pointer, no rows)
    got = pack_codes_dev(codes_d, N, M, guard=64).cpu().numpy()
    want = ref.pack_codes_ref(codes)
    assert np.array_equal(got[:len(want)], want)
    assert (got[len(want):] == 0xAB).all() and len(got) == len(want) + 64     # nothing behind the image


@pytest.mark.parametrize("M", [32, 64])
@pytest.mark.parametrize("pad", [0, 64])
def test_pack_lut_every_entry(dev, M, pad):
    D = host(M)
    src = sentinel_f((D["n"], M * 256 + pad), dev)
    src[:, :M * 256] = torch.from_numpy(D["lut"].reshape(D["n"], -1)).to(dev)
    got = pack_lut_dev(src, M * 256 + pad, D["n"], M).cpu().numpy().reshape(D["n"], M // 32, 256, 32)
    assert np.array_equal(got, ref.pack_lut_ref(D["lut"]))


# ----------------------------------------------------------------------------------------------------- 2-5. dense mode
@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_dense_scores_only(dev, layout, M, formula):
    """p0 = 1, slots 1..3, seg = 2300 (the longest list), ld_out = 3 * seg + 8: scores within the bar, -inf beyond the list, the
    sentinel in the slack columns and in the row of no query."""
    val, _ = Scan(dev, layout, M, formula, DENSE_SLOTS).dense(2300)
    check_dense(M, formula, DENSE_SLOTS, 2300, val, None)


@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_dense_with_ids(dev, layout, M, formula):
    """out_id != NULL: ids[list_off[l] + j] in the list (one of them above 2^40), -1 beyond it."""
    val, ids = Scan(dev, layout, M, formula, DENSE_SLOTS).dense(2300, with_id=True)
    check_dense(M, formula, DENSE_SLOTS, 2300, val, ids)
    assert (ids == ref.BIG_ID).sum() == 3                                     # the three tasks on the 2300-row list


@pytest.mark.parametrize("with_id", [False, True])
@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_dense_short_segment(dev, layout, M, formula, with_id):
    """seg = 100 < the 129-, 1100- and 2300-row lists: their first 100 rows, shorter lists padded, nothing past (slot - p0 + 1) * seg."""
    val, ids = Scan(dev, layout, M, formula, DENSE_SLOTS).dense(100, with_id=with_id)
    check_dense(M, formula, DENSE_SLOTS, 100, val, ids)


@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_strides(dev, layout, M, formula):
    """ld_lut = M * 256 + 64 (row-major: the raw tables, packed: the packed table set) and ld_probe = P + 3, NaN tables / another list in
    the gaps: bit for bit the output of the dense strides."""
    val0, ids0 = Scan(dev, layout, M, formula, DENSE_SLOTS).dense(2300, with_id=True)
    val1, ids1 = Scan(dev, layout, M, formula, DENSE_SLOTS, lut_pad=64, probe_pad=3).dense(2300, with_id=True)
    assert np.array_equal(bits(val0), bits(val1)) and np.array_equal(ids0, ids1)
    check_dense(M, formula, DENSE_SLOTS, 2300, val1, ids1)


# ----------------------------------------------------------------------------------------------------- 6-9. filtered mode
@pytest.mark.parametrize("rank", [20, 100, 1000])
@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_filtered_exact_survivor_sets(dev, layout, M, formula, rank):
    """tau[q] in the widest gap of the reference scores around ``rank``; no reference score within one bar of it (a condition of the
    test, asserted first: test_ivfpq_scan_ref_cpu.py checks it without a GPU), so the reference alone decides who survives."""
    D = host(M)
    tau = np.zeros(D["n"], dtype=np.float32)
    for q in range(D["n"]):
        s, mag, _ = query_scores(M, formula, q, ALL_SLOTS)
        tau[q] = ref.gap_threshold(s, rank)
        assert (np.abs(s - float(tau[q])) > ref.bar(M, mag)).all(), q
        assert (s > float(tau[q])).sum() < 4096
    check_filtered(M, formula, ALL_SLOTS, tau, 4096, Scan(dev, layout, M, formula, ALL_SLOTS).filtered(tau, 4096))


@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_staging_overflow(dev, layout, M, formula):
    """tau = -inf: every row of every probed list survives.  Slots 1..3: the 2300-row list is probed by queries 0 and 1 in ONE workgroup
    of the packed kernel (tasks 12 and 13) and by query 2 alone (task 14).  The packed kernel stages 1024 survivors per query in LDS;
    here about 1276 more per query take the direct branch (global atomics straight to the candidate rows) in the same task, next to
    the 1024 that go through staging."""
    D = host(M)
    tau = np.full(D["n"], -np.inf, dtype=np.float32)
    out = Scan(dev, layout, M, formula, DENSE_SLOTS).filtered(tau, 8192)
    assert out[2].tolist() == [2300 + 129, 2300 + 63, 65 + 2300 + 7, 1100 + 129, 1100 + 1 + 64]
    check_filtered(M, formula, DENSE_SLOTS, tau, 8192, out)


@pytest.mark.parametrize("cap", [1500, 7])
@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_capacity_overflow(dev, layout, M, formula, cap):
    """The data of test_staging_overflow with fewer slots than survivors (1500: between the staging size and the count; 7): cand_cnt is
    still the full count, the cap slots hold distinct true survivors of their own query, nothing is written outside the rows."""
    D = host(M)
    tau = np.full(D["n"], -np.inf, dtype=np.float32)
    out = Scan(dev, layout, M, formula, DENSE_SLOTS).filtered(tau, cap)
    assert out[2].tolist() == [2429, 2363, 2372, 1229, 1165]
    check_filtered(M, formula, DENSE_SLOTS, tau, cap, out)
    if cap == 7:
        assert (out[1] != SENT_I).all()                                       # every slot of every row is taken


@pytest.mark.parametrize("layout,M,formula", CASES, ids=CASE_IDS)
def test_strict_threshold(dev, layout, M, formula):
    """``> tau``, not ``>=``: with the kernel's OWN float32 score of a middle-ranked row as tau (bit for bit), that row is not emitted
    and every row whose dense score is greater is, with the identical bit pattern.  The kernel against itself, on purpose: what
    test_thresholded_round_loses_nothing assumes of the two rounds of a search.  Slot 1 of every query: lists 9 9 4 8 8."""
    D = host(M)
    slots = (1, 2)
    dense, _ = Scan(dev, layout, M, formula, slots).dense(2300)
    tau, want = np.zeros(D["n"], dtype=np.float32), []
    for q in range(D["n"]):
        _, _, rows = task_scores(M, formula)[(q, 1)]
        sc = dense[q, :len(rows)]
        mid = int(np.argsort(sc, kind="stable")[len(rows) // 2])
        tau[q] = sc[mid]
        live = sc > tau[q]
        assert 0 < live.sum() < len(rows) and not live[mid]
        want.append((int(D["ids"][rows[mid]]), {int(i): int(b) for i, b in zip(D["ids"][rows[live]], bits(sc[live]))}))
    cv, ci, cc, gv, gi = Scan(dev, layout, M, formula, slots).filtered(tau, 4096)
    for q, (mid_id, live) in enumerate(want):
        cnt = int(cc[q])
        assert cnt == len(live), (q, cnt, len(live))
        got = {int(i): int(b) for i, b in zip(ci[q, :cnt], bits(cv[q, :cnt]))}
        assert mid_id not in got and got == live, q
        assert (ci[q, cnt:] == SENT_I).all()


# ----------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals(dev):
    """Descriptors the entry point must refuse, each one field away from a valid one; nothing is launched (the output keeps the
    sentinel).  n_tasks = 0 is not an error and writes nothing either."""
    from gnnlm_amd._lib import GnnlmError

    def dense_scan(layout, M, formula):
        sc = Scan(dev, layout, M, formula, DENSE_SLOTS)
        ov = sentinel_f((sc.n, 3 * 2300), dev)
        sc.s.out_val, sc.s.ld_out, sc.s.p0, sc.s.seg = ov.data_ptr(), ov.stride(0), 1, 2300
        return sc, ov

    def refused(sc, ov):
        with pytest.raises(GnnlmError):
            sc.call()
        torch.cuda.synchronize()
        assert (bits(ov.cpu().numpy()) == SENT_F_BITS).all()

    T32, T16 = device_data(32, dev), device_data(16, dev)
    sc, ov = dense_scan("rowmajor", 32, "list_term")                          # list_term together with key_term
    sc.s.key_term = T32["key_term"].data_ptr()
    refused(sc, ov)
    sc, ov = dense_scan("packed", 32, "ip")                                   # list_term on the packed image
    sc.s.list_term, sc.s.ld_list_term = T32["list_term"].data_ptr(), 32 * 256
    refused(sc, ov)
    sc, ov = dense_scan("rowmajor", 16, "ip")                                 # packed at M = 16
    sc.s.packed = 1
    refused(sc, ov)
    sc, ov = dense_scan("rowmajor", 128, "ip")                                # M = 144 (the tables are wide enough: M alone is wrong)
    wide = torch.zeros(sc.n, 144 * 256, device=dev)
    sc.s.M, sc.s.lut, sc.s.ld_lut = 144, wide.data_ptr(), wide.stride(0)
    refused(sc, ov)
    sc, ov = dense_scan("rowmajor", 16, "ip")                                 # a table that is not 16-byte aligned
    wide = torch.zeros(sc.n * 16 * 256 + 4, device=dev)
    sc.s.lut = wide.data_ptr() + 4
    refused(sc, ov)
    sc, ov = dense_scan("rowmajor", 16, "ip")                                 # dense mode with seg = 0
    sc.s.seg = 0
    refused(sc, ov)
    sc, ov = dense_scan("rowmajor", 16, "ip")                                 # filtered mode without cand_cnt
    tau = torch.zeros(sc.n, device=dev)
    cv, ci = sentinel_f((sc.n, 64), dev), sentinel_i((sc.n, 64), dev)
    sc.s.tau, sc.s.cand_val, sc.s.cand_id, sc.s.cap = tau.data_ptr(), cv.data_ptr(), ci.data_ptr(), 64
    refused(sc, ov)
    assert (bits(cv.cpu().numpy()) == SENT_F_BITS).all() and (ci.cpu().numpy() == SENT_I).all()
    for layout, M in (("rowmajor", 16), ("packed", 32)):                      # no tasks: OK, nothing written
        sc, ov = dense_scan(layout, M, "ip")
        sc.s.n_tasks = 0
        sc.call()
        assert (bits(ov.cpu().numpy()) == SENT_F_BITS).all()
    assert T16["codes"].shape == (ref.N_ROWS, 16)
