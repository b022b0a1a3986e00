"""gnnlm_ivfpq_select_probes and gnnlm_ivfpq_select_final (csrc/ivfpq_select.hip) at the descriptor level, and the search wired to
them (GNNLM_IVF_SELECT, gnn-lm_amd/ivfpq.py).

Both entry points promise the bits of gnnlm_topk_merge with init = 1 on the same operands, so every case is compared twice, with no
tolerance: with the numpy restatement ``topk_ref.fold`` (ids equal, values equal, padding -1 with the worst infinity) and with
gnnlm_topk_merge run on the same device buffers (ids equal, values as bits except the sign of a zero, which the contract leaves
open).  The split outputs of the final selection are compared with gnnlm_ivfpq_split_payload run over the unsplit result.

Every call reads through a row stride of its own (one layout that keeps rows 16-byte aligned: the dwordx4 loads of the probe
kernel, one that does not: its scalar loads), pad columns and columns beyond row_ncols hold the WINNING infinity with valid ids, and
the outputs lie between guard words over a sentinel, so every slot must be written and none beyond."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import topk_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT_F_BITS = 0x7FC0BEEF
SENT_I = -0x0123456789ABCDEF
SENT_L = 0x5EADBEEF
GUARD = 64
LABEL_BITS = 24
VAL_LAST = -12345


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Outputs:
    """[n, k] values, ids and labels between guards, the sentinel everywhere"""

    def __init__(self, n, k, dev):
        self.n, self.k = n, k
        self.v = to_dev(np.full(2 * GUARD + n * k, SENT_F_BITS, dtype=np.uint32).view(F32), dev)
        self.i = to_dev(np.full(2 * GUARD + n * k, SENT_I, dtype=np.int64), dev)
        self.l = to_dev(np.full(2 * GUARD + n * k, SENT_L, dtype=np.int32), dev)

    def ptrs(self):
        return self.v.data_ptr() + 4 * GUARD, self.i.data_ptr() + 8 * GUARD, self.l.data_ptr() + 4 * GUARD

    def read(self, labels=False, touched=True):
        torch.cuda.synchronize()
        inner = slice(GUARD, GUARD + self.n * self.k)
        out = []
        for t, sent, as_bits in ((self.v, SENT_F_BITS, True), (self.i, SENT_I, False), (self.l, SENT_L, False)):
            a = t.cpu().numpy()
            g = np.concatenate([a[:GUARD], a[GUARD + self.n * self.k:]])
            assert ((bits(g) if as_bits else g) == sent).all()
            mine = a[inner]
            hit = (bits(mine) if as_bits else mine) == sent
            if t is self.l and not labels:
                assert hit.all()                                              # no label array was passed: nothing written there
            else:
                assert not hit.any() if touched else hit.all()
            out.append(mine.reshape(self.n, self.k))
        return out if labels else out[:2]


def check(got, want):
    """against topk_ref.fold: ids exactly, values equal, the padding exactly -1 with the worst infinity"""
    (gv, gi), (wv, wi) = got, want
    assert gv.shape == wv.shape
    for r in range(len(wi)):
        assert np.array_equal(gi[r], wi[r]), (r, int((gi[r] != wi[r]).argmax()), int((wi[r] >= 0).sum()))
        assert np.array_equal(gv[r], wv[r]), (r, int((gv[r] != wv[r]).argmax()))
    pad = wi < 0
    assert (gi[pad] == -1).all() and np.array_equal(bits(gv[pad]), bits(wv[pad]))


def same_bits(got, dev_ref):
    """against gnnlm_topk_merge on the same buffers: the same bits (a zero may differ in sign)"""
    (gv, gi), (dv, di) = got, dev_ref
    assert np.array_equal(gi, di)
    assert np.array_equal(bits(gv + F32(0)), bits(dv + F32(0)))


# ------------------------------------------------------------------------------------------------------ 1. probe selection
PROBE_NCOLS = (1, 31, 32, 33, 63, 64, 65, 255, 4095, 4096)
PROBE_N = (1, 5, 67)
PROBE_K = (1, 32, 64)
PROBE_PATTERNS = ("few_distinct", "constant", "ascending", "specials", "descending", "random_ties")


def probe_rows(rs, n, nc, k, largest, bias, first):
    """scores [n, nc]: row r follows pattern (first + r) % 6, laid out in value space and carried back through the bias (multiples of
    1/4 against values that are multiples of 1/64: exact, a tie that is meant is a tie)"""
    sgn = 1.0 if largest else -1.0
    s = np.zeros((n, nc), dtype=F32)
    for r in range(n):
        pat = PROBE_PATTERNS[(first + r) % len(PROBE_PATTERNS)]
        if pat == "specials":
            s[r] = np.resize(np.roll(ref.SPECIALS, r), nc)
            continue
        g, _ = ref._goodness(rs, pat, nc, k)
        w = (sgn * g).astype(F32)
        s[r] = w - bias if bias is not None else w
    return s


def probe_layout(s, aligned, largest, dev):
    """-> (tensor, pointer, ld): rows 16-byte aligned with a stride of a multiple of 4 floats, or one float into the allocation with
    ld = ncols + 3; the pad holds the winning infinity"""
    n, nc = s.shape
    win = F32(np.inf if largest else -np.inf)
    ld, off = ((nc + 3) // 4 * 4 + 4, 0) if aligned else (nc + 3, 1)
    host = np.full(off + n * ld + 4, win, dtype=F32)
    host[off:off + n * ld].reshape(n, ld)[:, :nc] = s
    t = to_dev(host, dev)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, ld


def run_probes(ptr, ld, n, nc, k, largest, bias_t, dev, out=None):
    from gnnlm_amd import _lib
    out = out or Outputs(n, k, dev)
    d = _lib.gnnlm_ivfpq_select_probes_t()
    d.scores, d.ld, d.n, d.ncols, d.k, d.largest = ptr, ld, n, nc, k, largest
    if bias_t is not None:
        d.col_bias = bias_t.data_ptr()
    d.out_val, d.out_id, _ = out.ptrs()
    _lib.call_desc("gnnlm_ivfpq_select_probes", d)
    return out.read()


def run_topk(ptr, ld, n, nc, k, largest, dev, bias_t=None, ids=None, row_ncols=None):
    """gnnlm_topk_merge, init = 1, over the same buffers"""
    from gnnlm_amd import _lib
    out = Outputs(n, k, dev)
    d = _lib.gnnlm_topk_t()
    d.scores, d.ld, d.n, d.ncols, d.k, d.largest, d.init, d.alpha = ptr, ld, n, nc, k, largest, 1, 1.0
    if bias_t is not None:
        d.col_bias = bias_t.data_ptr()
    if ids is not None:
        d.ids, d.ld_ids = ids
    if row_ncols is not None:
        d.row_ncols = row_ncols.data_ptr()
    d.best_val, d.best_id, _ = out.ptrs()
    _lib.call_desc("gnnlm_topk_merge", d)
    return out, out.read()


@pytest.mark.parametrize("nc", PROBE_NCOLS)
def test_select_probes(dev, nc):
    """every n x k x direction x bias of the issue at this width (k > ncols included), both layouts; the row patterns rotate with the
    case so that the one-row calls see all of them"""
    rs = np.random.RandomState(nc)
    case = 0
    for n in PROBE_N:
        for k in PROBE_K:
            for largest in (1, 0):
                for with_bias in (False, True):
                    bias = (rs.randint(-32, 33, nc) / 4.0).astype(F32) if with_bias else None
                    s = probe_rows(rs, n, nc, k, largest, bias, first=case)
                    case += 1
                    call = dict(scores=s, ncols=nc, k=k, largest=largest, init=1, alpha=1.0, col_scale=None, col_bias=bias, col0=0,
                                col_ids=None, ids=None, row_ncols=None)
                    want = ref.fold(call)
                    for aligned in (True, False):
                        # (the bias is aligned with the rows or one float off with them: the wide loads need both)
                        bias_buf = None if bias is None else to_dev(np.concatenate([np.zeros(0 if aligned else 1, F32), bias]), dev)
                        bias_t = None if bias is None else bias_buf[0 if aligned else 1:]
                        t, ptr, ld = probe_layout(s, aligned, largest, dev)
                        got = run_probes(ptr, ld, n, nc, k, largest, bias_t, dev)
                        what = (n, k, largest, with_bias, aligned)
                        try:
                            check(got, want)
                            same_bits(got, run_topk(ptr, ld, n, nc, k, largest, dev, bias_t)[1])
                        except AssertionError as e:
                            raise AssertionError(f"{what}: {e}") from e


def test_select_probes_empty_and_refused(dev):
    """n = 0 touches nothing, ncols = 0 writes the padding; ncols 4097, k 65, k 0 and null operands are refused with nothing written"""
    from gnnlm_amd import _lib
    rs = np.random.RandomState(0)
    s = rs.randn(3, 4100).astype(F32)
    t, ptr, ld = probe_layout(s, True, 1, dev)

    def desc(out, **kw):
        d = _lib.gnnlm_ivfpq_select_probes_t()
        d.scores, d.ld, d.n, d.ncols, d.k, d.largest = ptr, ld, 3, 40, 8, 1
        d.out_val, d.out_id, _ = out.ptrs()
        for a, b in kw.items():
            setattr(d, a, b)
        return d

    out = Outputs(3, 8, dev)
    _lib.call_desc("gnnlm_ivfpq_select_probes", desc(out, n=0, scores=None))
    out.read(touched=False)
    for largest in (1, 0):
        out = Outputs(3, 8, dev)
        _lib.call_desc("gnnlm_ivfpq_select_probes", desc(out, ncols=0, scores=None, largest=largest))
        check(out.read(), ref.empty_state(3, 8, largest))
    for kw, k in ((dict(ncols=4097), 8), (dict(k=65), 65), (dict(k=0), 8), (dict(scores=None), 8), (dict(out_val=None), 8),
                  (dict(out_id=None), 8), (dict(n=-1), 8), (dict(ncols=-1), 8)):
        out = Outputs(3, k, dev)
        with pytest.raises(_lib.GnnlmError):
            _lib.call_desc("gnnlm_ivfpq_select_probes", desc(out, **kw))
        out.read(touched=False)
    out = Outputs(3, 8, dev)                                                  # and the valid one is accepted
    _lib.call_desc("gnnlm_ivfpq_select_probes", desc(out))
    check(out.read(), ref.fold(dict(scores=s[:, :40], ncols=40, k=8, largest=1, init=1, alpha=1.0, col_scale=None, col_bias=None, col0=0,
                                    col_ids=None, ids=None, row_ncols=None)))


# ------------------------------------------------------------------------------------------------------ 2. final selection
FINAL_CAPS = (1024, 2048, 16384)
FINAL_KS = (1, 1023, 1024)


def final_rows(rs, cap, k):
    """-> (values [n, cap], payloads [n, cap], row_ncols [n]).  Rows of random values with ties by the hundred (multiples of 1/64) and
    unique payloads id << 24 | label, of every length of the issue; rows whose ties across the cut differ in ONE digit of the payload
    (bits 55.., 33.., 22.. and 0..: a high, a middle and the low digit of the id, and the label); duplicate payloads, with equal and
    with different values; a negative payload on the best value; a constant row of 2048 (cap 1024: 1024) -- one bin, ties by id."""
    lens = [0, 1, k - 1, k, k + 1, 1577, cap]
    rows = []
    for m in lens:
        m = max(0, min(m, cap))
        rows.append((rs.randint(-2048, 2048, m) / 64.0, ref._payload_ids(rs, m)))
    m = min(cap, 2 * k + 300)
    for shift in (55, 33, 22, 0):
        rows.append(ref.digit_row(rs, m, k, shift))
    m = min(cap, 1577)
    g, p = rs.randint(-2048, 2048, m) / 64.0, ref._payload_ids(rs, m)
    g[0] = g[1] = 40.0                                                        # the same (value, payload) twice, on top
    p[1] = p[0]
    p[3] = p[2]                                                               # the same payload under two values
    g[2], g[3] = 1.0, -1.0
    p[5] = p[4]                                                               # and twice inside one run of ties
    g[4] = g[5] = g[6]
    rows.append((g, p))
    g, p = rs.randint(-2048, 2048, m) / 64.0, ref._payload_ids(rs, m)
    g[7], p[7] = 50.0, -5                                                     # no candidate, whatever its value
    g[8], p[8] = 50.0, -(1 << 40)
    rows.append((g, p))
    m = min(cap, 2048)
    rows.append((np.full(m, 1.5), ref._payload_ids(rs, m)))
    n = len(rows)
    val = np.full((n, cap), np.inf, dtype=F32)                                # beyond a row: the winning infinity, valid ids
    pay = rs.randint(0, 1 << 40, (n, cap)).astype(np.int64)
    rn = np.zeros(n, dtype=np.int32)
    for r, (g, p) in enumerate(rows):
        val[r, :len(g)], pay[r, :len(g)], rn[r] = g.astype(F32), p, len(g)
    rn[6] = cap + 9                                                           # above cap: clamped
    return val, pay, rn


@pytest.fixture(scope="module")
def final_case(dev):
    """one set of rows per (cap, k), built once, its numpy reference with it; shared by the split and the unsplit run"""
    cache = {}

    def get(cap, k):
        if (cap, k) not in cache:
            rs = np.random.RandomState(cap + k)
            val, pay, rn = final_rows(rs, cap, k)
            call = dict(scores=val, ncols=cap, k=k, largest=1, init=1, alpha=1.0, col_scale=None, col_bias=None, col0=0, col_ids=None,
                        ids=pay, row_ncols=rn)
            n = len(rn)
            ldv, ldi = cap + 3, cap + 1
            hv = np.full(1 + n * ldv, np.inf, dtype=F32)
            hv[1:].reshape(n, ldv)[:, :cap] = val
            hi = np.full((n, ldi), 1, dtype=np.int64)
            hi[:, :cap] = pay
            cache[(cap, k)] = (call, ref.fold(call), to_dev(hv, dev), ldv, to_dev(hi, dev), ldi, to_dev(rn, dev))
        return cache[(cap, k)]
    return get


@pytest.mark.parametrize("split", [False, True], ids=["payload", "split"])
@pytest.mark.parametrize("k", FINAL_KS)
@pytest.mark.parametrize("cap", FINAL_CAPS)
def test_select_final(dev, final_case, cap, k, split):
    from gnnlm_amd import _lib
    call, want, vt, ldv, it, ldi, rnt = final_case(cap, k)
    n = len(call["row_ncols"])
    outs = []
    for with_labels in ((True, False) if split else (False,)):
        out = Outputs(n, k, dev)
        d = _lib.gnnlm_ivfpq_select_final_t()
        d.cand_val, d.ld_val, d.cand_id, d.ld_id = vt.data_ptr() + 4, ldv, it.data_ptr(), ldi
        d.row_ncols, d.n, d.cap, d.k = rnt.data_ptr(), n, cap, k
        d.out_val, d.out_id, lab = out.ptrs()
        if split:
            d.label_bits, d.val_last = LABEL_BITS, VAL_LAST
            if with_labels:
                d.out_vals = lab
        _lib.call_desc("gnnlm_ivfpq_select_final", d)
        outs.append(out.read(labels=with_labels))
    # gnnlm_topk_merge over the same buffers, and gnnlm_ivfpq_split_payload over its result
    tk, (dv, di) = run_topk(vt.data_ptr() + 4, ldv, n, cap, k, 1, dev, ids=(it.data_ptr(), ldi), row_ncols=rnt)
    check((dv, di), want)
    if not split:
        check(outs[0], want)
        same_bits(outs[0], (dv, di))
        return
    wv, wp = want
    check((outs[0][0], outs[0][1]), (wv, np.where(wp < 0, wp, wp >> LABEL_BITS)))
    assert np.array_equal(outs[0][2], np.where(wp < 0, VAL_LAST, wp & ((1 << LABEL_BITS) - 1)).astype(np.int32))
    _, pi, pl = tk.ptrs()
    _lib.call("gnnlm_ivfpq_split_payload", pi, n * k, LABEL_BITS, VAL_LAST, pl, _lib.stream())
    sv, si, sl = tk.read(labels=True)
    same_bits((outs[0][0], outs[0][1]), (sv, si))
    assert np.array_equal(outs[0][2], sl)
    same_bits(outs[1], (sv, si))                                              # without a label array: the ids alone


def test_select_final_empty_and_refused(dev, final_case):
    from gnnlm_amd import _lib
    call, want, vt, ldv, it, ldi, rnt = final_case(1024, 1)
    n = len(call["row_ncols"])

    def desc(out, **kw):
        d = _lib.gnnlm_ivfpq_select_final_t()
        d.cand_val, d.ld_val, d.cand_id, d.ld_id = vt.data_ptr() + 4, ldv, it.data_ptr(), ldi
        d.row_ncols, d.n, d.cap, d.k = rnt.data_ptr(), n, 1024, out.k
        d.out_val, d.out_id, _ = out.ptrs()
        for a, b in kw.items():
            setattr(d, a, b)
        return d

    out = Outputs(n, 8, dev)
    _lib.call_desc("gnnlm_ivfpq_select_final", desc(out, n=0))
    out.read(touched=False)
    out = Outputs(n, 8, dev)
    _lib.call_desc("gnnlm_ivfpq_select_final", desc(out, cap=0, cand_val=None, cand_id=None))
    check(out.read(), ref.empty_state(n, 8, 1))
    out = Outputs(n, 8, dev)                                                  # row_ncols NULL: every row has cap columns
    _lib.call_desc("gnnlm_ivfpq_select_final", desc(out, row_ncols=None, cap=500))
    check(out.read(), ref.fold(dict(call, scores=call["scores"][:, :500], ids=call["ids"][:, :500], ncols=500, k=8, row_ncols=None)))
    for kw, k in ((dict(cap=16385), 8), (dict(k=1025), 1025), (dict(k=0), 8), (dict(cand_val=None), 8), (dict(cand_id=None), 8),
                  (dict(out_val=None), 8), (dict(out_id=None), 8), (dict(label_bits=32), 8), (dict(label_bits=-1), 8), (dict(n=-1), 8)):
        out = Outputs(n, k, dev)
        with pytest.raises(_lib.GnnlmError):
            _lib.call_desc("gnnlm_ivfpq_select_final", desc(out, **kw))
        out.read(touched=False)


# ------------------------------------------------------------------------------------------------------ 3. the search, end to end
CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
from gnnlm_amd.ivfpq import IVFPQIndex
dev = torch.device("cuda:0")
z = np.load(sys.argv[2] + "/inputs.npz")
labels, qt, k = torch.from_numpy(z["labels"]).to(dev), torch.from_numpy(z["q"]).to(dev), 64
out = {}
index = IVFPQIndex.load(sys.argv[2] + "/index.npz", device=dev, nprobe=8).attach_vals(labels)
assert index.tiles is not None and index.M == 64 and index.nlist == 64
v, i, l = index.search_device(qt, k, return_vals=True)
out["v"], out["i"], out["l"] = v.cpu().numpy(), i.cpu().numpy(), l.cpu().numpy()
v, i = index.search_device(qt, k)                                            # ids without labels
out["v1"], out["i1"] = v.cpu().numpy(), i.cpu().numpy()
v, i = index.search_device(qt, 20)                                           # another width of the result
out["v2"], out["i2"] = v.cpu().numpy(), i.cpu().numpy()
# a sampled threshold that fails for most queries: they are searched again on their own and written into the main result
b = IVFPQIndex(index.R, index.coarse, index.pq, index.list_off, index.list_ids, index.list_codes, nprobe=8).attach_vals(labels)
b.threshold_sample, b.sample_min_keys_per_k, b.sample_sigmas, b.sample_fail_frac = 4, 0, -1e9, 1.0
v, i, l = b.search_device(qt, k, return_vals=True)
out["requeried"] = np.array(int(b.stats["requeried"]))
out["vb"], out["ib"], out["lb"] = v.cpu().numpy(), i.cpu().numpy(), l.cpu().numpy()
# the L2 index: probe selection with the -|c|^2 / 2 bias, the float32 scan behind it (the split stays a pass of its own)
l2 = IVFPQIndex(index.R, index.coarse, index.pq, index.list_off, index.list_ids, index.list_codes, nprobe=8, cosine=False,
                metric="l2").attach_vals(labels)
v, i, l = l2.search_device(qt, k, return_vals=True)
out["vl2"], out["il2"], out["ll2"] = v.cpu().numpy(), i.cpu().numpy(), l.cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def test_search_same_with_and_without(dev, tmp_path):
    """A small index with labels (M = 64, 64 lists, 6000 keys, k = 64) searched with GNNLM_IVF_SELECT=1 and =0, each in a fresh child
    process (the switch is read from the environment): scores, ids and labels identical, through the re-search of single queries
    too, and every payload split exactly once (ids are row numbers again, labels are the labels of those rows)."""
    from gnnlm_amd.ivfpq import IVFPQIndex
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rs = np.random.RandomState(5)
    N, d = 6000, 256
    centres = rs.randn(40, d).astype(F32)
    keys = (centres[rs.randint(0, 40, N)] + 0.6 * rs.randn(N, d).astype(F32)).astype(np.float16)
    labels = rs.randint(0, 50000, N).astype(np.int32)
    q = (centres[rs.randint(0, 40, 300)] + 0.6 * rs.randn(300, d).astype(F32)).astype(F32)
    q /= np.sqrt((q ** 2).sum(1, keepdims=True))
    # one index for both children (the k-means of the build adds with atomics: two builds differ in the last bits)
    IVFPQIndex.build(keys, 64, 64, device=dev, cosine=True, nprobe=8, iters=3, seed=3).save(str(tmp_path / "index.npz"))
    np.savez(str(tmp_path / "inputs.npz"), labels=labels, q=q)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    res = {}
    for sw in ("1", "0"):
        env = dict(os.environ, GNNLM_IVF_SELECT=sw)
        path = str(tmp_path / f"out{sw}.npz")
        r = subprocess.run([sys.executable, str(script), root, str(tmp_path), path], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        res[sw] = dict(np.load(path))
    a, b = res["1"], res["0"]
    assert sorted(a) == sorted(b)
    for name in a:
        if a[name].dtype == np.float32:
            assert np.array_equal(bits(a[name]), bits(b[name])), name
        else:
            assert np.array_equal(a[name], b[name]), name
    assert int(a["requeried"]) > 0
    for i, l in (("i", "l"), ("ib", "lb"), ("il2", "ll2")):
        ids = a[i]
        assert ids.min() >= -1 and ids.max() < 6000 and (ids >= 0).any()
        assert np.array_equal(a[l][ids >= 0], labels[ids[ids >= 0]])
    assert np.array_equal(a["i"], a["i1"]) and np.array_equal(bits(a["v"]), bits(a["v1"]))
