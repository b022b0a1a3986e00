"""gnnlm_adaptive_target_logp at the call level (include/gnnlm.h: gnnlm_adaptive_softmax_t), and gnnlm_row_lse_pick on its own: the
descriptor is filled by hand and passed to ``_lib.call``; the reference, the routes, the bound and the table of cases are
tests/adaptive_ref.py, and test_adaptive_ref_cpu.py shows without a GPU that every case reaches the routes it names, that a float32
evaluation of the call stays inside the bound and that nine wrong references leave it.

What EVERY call of this file carries (``lay_out`` / ``run``):
  * ldx = d + 4 with NaN in the pad columns; the x panel is 7 rows taller than n, the extra rows NaN;
  * x and the weights 16-byte aligned, tail dims multiples of 4; the targets between guard bands of zeros;
  * lm_logp ONE float off a 16-byte boundary, between guard bands, holding the NaN-payload sentinel; guard bands come back
    bit-identical;
  * the workspace is exactly gnnlm_adaptive_workspace_bytes bytes between guard bands; every case runs twice, once with the
    workspace filled with the sentinel and once with 1e30: the two results are equal bit for bit.
Every valid row is within adaptive_ref.bound of the float64 reference; every row whose target lies outside the vocabulary is
-INFINITY exactly."""
import ctypes

import numpy as np
import pytest
import torch

import adaptive_ref as ar
import gemm_ref
from test_gemm_abi_gpu import GUARD, Out, bits, dev_in, kernel_names

pytestmark = pytest.mark.gpu
E_INVALID = -22


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Laid:
    """A case on the device: the descriptor, the inputs (kept alive) and fresh outputs per call"""

    def __init__(self, case, dev):
        from gnnlm_amd import _lib
        self.case, self.dev, self.keep = case, dev, []
        n, d, cut, dim = case["n"], case["d"], case["cutoff"], case["dim"]
        self.n, self.ldx = n, d + 4
        w = _lib.gnnlm_adaptive_softmax_t()
        w.d, w.n_bands, w.gemm_precision = d, len(cut), case["precision"]
        for i, c in enumerate(cut):
            w.cutoff[i] = c
        w.head_w = self.put(case["head_w"])
        for b in range(1, len(cut)):
            w.proj_t[b], w.emb[b], w.dim[b] = self.put(case["proj_t"][b]), self.put(case["emb"][b]), dim[b]
        self.w = w
        panel = np.full((n + 7, self.ldx), np.nan, dtype=np.float32)
        panel[:n, :d] = case["x"]
        self.x_t, self.x = dev_in(panel.reshape(-1), dev)
        self.t_t, self.target = dev_in(case["target"].astype(np.int64), dev)
        assert self.x % 16 == 0 and w.head_w % 16 == 0
        self.ws_bytes = int(_lib.lib().gnnlm_adaptive_workspace_bytes(ctypes.byref(w), n))
        assert self.ws_bytes % 4 == 0

    def put(self, a):
        t, p = dev_in(a.reshape(-1), self.dev)
        self.keep.append(t)
        assert p % 16 == 0
        return p

    def outputs(self, fill=None):
        out = Out(gemm_ref.sentinel(max(self.n, 1)), self.dev, 1)
        init = gemm_ref.sentinel(self.ws_bytes // 4) if fill is None else np.full(self.ws_bytes // 4, fill, dtype=np.float32)
        ws = Out(init, self.dev, 0)
        assert ws.ptr % 16 == 0 and out.ptr % 16 == 4
        return out, ws

    def args(self, out_, ws_, **kw):
        a = dict(w=self.w, x=self.x, ldx=self.ldx, target=self.target, n=self.n, out=out_.ptr, ws=ws_.ptr, ws_bytes=self.ws_bytes)
        a.update(kw)
        return a


def raw_call(a):
    from gnnlm_amd import _lib
    vp = ctypes.c_void_p
    return _lib.lib().gnnlm_adaptive_target_logp(ctypes.byref(a["w"]), vp(a["x"]), a["ldx"], vp(a["target"]), a["n"], vp(a["out"]),
                                                 vp(a["ws"]), a["ws_bytes"], _lib.stream())


def launch(laid, fill):
    from gnnlm_amd import _lib
    out, ws = laid.outputs(fill)
    _lib.check(raw_call(laid.args(out, ws)), "gnnlm_adaptive_target_logp")
    torch.cuda.synchronize()
    ws.read()                                                          # the workspace's guard bands
    return out.read()[:laid.n]


def run(case, dev):
    laid = Laid(case, dev)
    got = launch(laid, None)
    again = launch(laid, 1e30)
    assert np.array_equal(bits(got), bits(again)), "the result depends on what the workspace held (or two calls differ)"
    return got


def check(case, got, label):
    ref = ar.case_ref(case)
    assert not (bits(got) == gemm_ref.SENT_BITS).any(), "a row of lm_logp was not written"
    valid = ref["valid"]
    assert np.isneginf(got[~valid]).all(), (label, "a target outside the vocabulary gives -INFINITY", got[~valid])
    v = valid & np.isfinite(ref["logp"])
    ratio = np.abs(got[v].astype(np.float64) - ref["logp"][v]) / ref["bound"][v] if v.any() else np.zeros(1)
    print(f"{label}: precision {case['precision']} worst error / bound {float(np.nanmax(ratio)) if ratio.size else 0.0:.3f} "
          f"(error {float(np.abs(got[v] - ref['logp'][v]).max()) if v.any() else 0.0:.2e}, {int((~valid).sum())} rows outside the vocabulary)")
    bad = ar.outside(got, ref["logp"], ref["bound"], valid)
    assert not len(bad), (label, bad[:5], got[bad[:5]], ref["logp"][bad[:5]], ref["bound"][bad[:5]])


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", ar.CASES)
def test_case(dev, name):
    case = ar.case_by_name(name)
    for k, v in ar.SPEC_BY_NAME[name].get("expect", {}).items():
        assert ar.routes(case)[k] == v
    check(case, run(case, dev), name)


def test_closed_forms(dev):
    """An all-zero row is -log(head logits) - log(band size), the closed form, within four float32 roundings of values below 8;
    rows 5 and 6 carry a logit of +90 and are finite only with the maximum subtracted."""
    case = ar.case_by_name("num-p0")
    got = run(case, dev)
    cut = case["cutoff"]
    want = -np.log(cut[0] + len(cut) - 1) - np.log(cut[2] - cut[1])
    assert abs(float(got[2]) - want) < 2 * 2.0 ** -21 * 8, (got[2], want)
    assert np.isfinite(got[[5, 6]]).all(), "logits of +90: finite only with the maximum subtracted"


def test_n_zero_touches_nothing(dev):
    case = ar.case_by_name("cmp-n65-b3-uniform")
    laid = Laid(case, dev)
    for null_ws in (False, True):
        out, ws = laid.outputs()
        kw = dict(n=0, ws=None, ws_bytes=0) if null_ws else dict(n=0)
        assert raw_call(laid.args(out, ws, **kw)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.read()), bits(out.init)) and np.array_equal(bits(ws.read()), bits(ws.init))


# ------------------------------------------------------------------------------------------ refusals
def _set(field, value, index=None):
    def f(a, laid):
        if index is None:
            setattr(a["w"], field, value)
        else:
            getattr(a["w"], field)[index] = value
    return f


def _arg(**kw):
    def f(a, laid):
        a.update({k: (v(a) if callable(v) else v) for k, v in kw.items()})
    return f


REFUSALS = [
    ("n_bands 0", _set("n_bands", 0)),
    ("n_bands 9", _set("n_bands", 9)),
    ("d % 4", _set("d", 18)),
    ("gemm_precision 4", _set("gemm_precision", 4)),
    ("NULL head_w", _set("head_w", None)),
    ("NULL proj_t[1]", _set("proj_t", None, 1)),
    ("NULL emb[2]", _set("emb", None, 2)),
    ("tail dim 0", _set("dim", 0, 1)),
    ("tail dim % 4", _set("dim", 18, 2)),
    ("cutoffs equal", _set("cutoff", 40, 1)),
    ("cutoffs descend", _set("cutoff", 90, 2)),
    ("ldx < d", _arg(ldx=12)),
    ("ldx % 4", _arg(ldx=22)),
    ("x 4 bytes off", _arg(x=lambda a: a["x"] + 4)),
    ("n < 0", _arg(n=-1)),
    ("NULL workspace", _arg(ws=None)),
    ("workspace half the size", _arg(ws_bytes=lambda a: a["ws_bytes"] // 2)),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refused(dev, what):
    """GNNLM_E_INVALID with a message, and output, workspace and guard bands bit-identical afterwards: nothing was launched"""
    from gnnlm_amd import _lib
    mutate = dict(REFUSALS)[what]
    case = ar.case_by_name("cmp-n65-b3-uniform")
    assert case["cutoff"] == [40, 100, 150] and case["d"] == 16
    laid = Laid(case, dev)
    out, ws = laid.outputs()
    a = laid.args(out, ws)
    mutate(a, laid)
    rc = raw_call(a)
    torch.cuda.synchronize()
    assert rc == E_INVALID, (what, rc)
    assert _lib.lib().gnnlm_last_error().decode().startswith("invalid argument: adaptive"), what
    assert np.array_equal(bits(out.read()), bits(out.init)) and np.array_equal(bits(ws.read()), bits(ws.init)), what
    laid = Laid(case, dev)                                             # the untouched descriptor is accepted
    check(case, launch(laid, None), "refusal base")


# ------------------------------------------------------------------------------------------ graph capture
def test_graph_replay_follows_x_and_targets(dev):
    """Captured on one side stream (no parallel branches) after an eager warm-up; x and the targets are then rewritten in place so
    that every band's count changes, band 1's to 0: each replay equals the eager call on the same inputs bit for bit."""
    from gnnlm_amd import _lib
    case = ar.case_by_name("cmp-n1025-b3-uniform")
    n, cut = case["n"], case["cutoff"]
    laid = Laid(case, dev)
    out, ws = laid.outputs()
    a = laid.args(out, ws)
    side = torch.cuda.Stream(device=dev)

    def eager():
        o2, w2 = laid.outputs(1e30)
        with torch.cuda.stream(side):
            _lib.check(raw_call(laid.args(o2, w2)), "eager")
        torch.cuda.synchronize()
        return o2.read()[:n]

    first = eager()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        _lib.check(raw_call(a), "captured")
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.read()[:n]), bits(first))
    check(case, out.read()[:n], "graph, first inputs")
    # new inputs in the captured buffers: rows reversed, every target of band 1 moved to band 2, a third of band 0 as well
    t2 = case["target"][::-1].copy()
    t2[(t2 >= cut[0]) & (t2 < cut[1])] = cut[1] + 1
    t2[np.arange(n) % 3 == 0] = cut[2] - 1
    case2 = dict(case, name=case["name"] + "-rewritten", x=np.ascontiguousarray(case["x"][::-1]), target=t2)
    c1, c2 = [len(r) for r, _ in ar.compact(case)[1]], [len(r) for r, _ in ar.compact(case2)[1]]
    assert c2[0] == 0 and c1[0] > 0 and c1[1] != c2[1] and (n - sum(c1)) != (n - sum(c2))
    panel = np.full((n + 7, laid.ldx), np.nan, dtype=np.float32)
    panel[:n, :case["d"]] = case2["x"]
    laid.x_t[GUARD:GUARD + panel.size].copy_(torch.from_numpy(panel.reshape(-1)))
    laid.t_t[GUARD:GUARD + n].copy_(torch.from_numpy(t2))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    second = out.read()[:n].copy()
    ws.read()
    assert np.array_equal(bits(second), bits(eager())) and not np.array_equal(bits(second), bits(first))
    check(case2, second, "graph, rewritten inputs")


# ------------------------------------------------------------------------------------------ the launched kernels by name
def test_launched_kernels_are_the_named_ones(dev):
    """The four-wave reduce of a band of 65,409 words, the A-stationary kernel of a band of dim 64, the skinny kernel of a
    projection at d = 512, as torch's profiler names them."""
    for name, wants in (("shape-band-65409", ["lse_reduce_kernel<4>", "lse_reduce_kernel<1>", "band_split_kernel", "tail_combine_kernel"]),
                        ("shape-dim64", ["gemm_lse_astationary_kernel", "head_logp_kernel"]),
                        ("proj-skinny32", ["gemm_nt_f32_skinny_kernel", "gemm_lse_astationary_kernel"])):
        case = ar.case_by_name(name)
        laid = Laid(case, dev)
        launch(laid, None)
        out, ws = laid.outputs()
        names = kernel_names(lambda: raw_call(laid.args(out, ws)))
        assert names, "torch's profiler reported no device kernel of the library"
        for want in wants:
            assert any(want.replace(" ", "") in n.replace(" ", "") for n in names), (name, want, names)


# ------------------------------------------------------------------------------------------ gnnlm_row_lse_pick on its own
def _row_lse_pick(dev, logits, n, m_dev, pick, want_picked):
    """-> (lse, picked or None) as they came back; logits [rows, ld] with NaN pads, between NaN guard bands"""
    from gnnlm_amd import _lib
    rows, ld = logits.shape
    l_t, l_ptr = dev_in(logits.reshape(-1), dev, 1)
    lse = Out(gemm_ref.sentinel(rows), dev, 1)
    picked = Out(gemm_ref.sentinel(rows), dev, 1) if want_picked else None
    pk = None if pick is None else dev_in(pick.astype(np.int32), dev)
    md = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=dev)
    vp = ctypes.c_void_p
    _lib.call("gnnlm_row_lse_pick", vp(l_ptr), ld, rows, _lib.ptr(md), n, vp(pk[1]) if pk else None, vp(lse.ptr),
              vp(picked.ptr) if picked else None, _lib.stream())
    torch.cuda.synchronize()
    return lse.read(), (picked.read() if picked else None)


def _lse64(logits, n):
    return torch.logsumexp(torch.from_numpy(logits[:, :n].astype(np.float64)), 1).numpy()


def _check_lse(got, want, what):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), \
        (what, got, want)
    # the bar test_lse_reduce derives for a sum of n terms: the maximum exact, n terms of relative error 2^-22 summed, logf, one rounding
    bar = 2.0 ** -21 * (np.abs(want[fin]) + 8.0)
    assert (np.abs(got[fin] - want[fin]) <= bar).all(), (what, float(np.abs(got[fin] - want[fin]).max()))


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_row_lse_pick(dev, n, rows):
    rs = np.random.RandomState(n * 7 + rows)
    ld = n + 3
    logits = np.full((rows, ld), np.nan, dtype=np.float32)
    logits[:, :n] = rs.standard_normal((rows, n)) * 3.5
    logits[rows - 1, :n] += 85.0                                      # exp(x) overflows without the maximum
    want = _lse64(logits, n)
    pick = rs.randint(0, n, rows)
    pick[0] = n - 1
    for m_dev in (None, 0, rows - 1, rows, rows + 2):
        m = rows if m_dev is None else min(rows, m_dev)
        for with_pick, with_picked in ((True, True), (False, True), (False, False)):
            lse, picked = _row_lse_pick(dev, logits, n, m_dev, pick if with_pick else None, with_picked)
            what = (n, rows, m_dev, with_pick, with_picked)
            assert (bits(lse[m:]) == gemm_ref.SENT_BITS).all(), what
            _check_lse(lse[:m], want[:m], what)
            if with_picked:
                assert (bits(picked[m:]) == gemm_ref.SENT_BITS).all(), what
                assert np.array_equal(picked[:m], logits[np.arange(m), pick[:m]] if with_pick else np.zeros(m, dtype=np.float32)), what
    # picks outside [0, n): -1 and n lie inside the allocation (the guard band, the pad columns); picked stays untouched
    bad = pick.copy()
    bad[0] = -1
    bad[rows - 1] = n if rows > 1 else -1
    lse, picked = _row_lse_pick(dev, logits, n, None, bad, True)
    _check_lse(lse, want, "out-of-range picks")
    out_of_range = (bad < 0) | (bad >= n)
    assert (bits(picked[out_of_range]) == gemm_ref.SENT_BITS).all(), "picked written for a pick outside [0, n)"
    assert np.array_equal(picked[~out_of_range], logits[np.nonzero(~out_of_range)[0], bad[~out_of_range]])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_row_lse_pick_infinities(dev, n):
    """-inf in every position class of the kernel's 256 threads x 4 waves (element e belongs to thread e % 256): the first element
    of a thread, a whole thread, a whole wave, all of the row but one element, the whole row; one and two +inf; a NaN; a -inf in
    front of a NaN.  The answer is torch.logsumexp's in float64."""
    rs = np.random.RandomState(n)
    e = np.arange(n)
    masks = [e == 7 % n, e % 256 == 7 % n, (e % 256) // 64 == min(1, (n - 1) // 64), e != n // 2, e == e, e == 0, e < 2]
    rows = len(masks) + 5
    logits = np.full((rows, n + 3), np.nan, dtype=np.float32)
    logits[:, :n] = rs.standard_normal((rows, n)) * 3.5
    for r, m in enumerate(masks):
        logits[r, :n][m] = -np.inf
    r = len(masks)
    logits[r, n // 2] = np.inf
    logits[r + 1, [0, n - 1]] = np.inf
    logits[r + 2, n // 3] = np.nan
    logits[r + 3, 0], logits[r + 3, n - 1] = -np.inf, (np.nan if n > 1 else -np.inf)
    logits[r + 4, 0], logits[r + 4, n - 1] = np.inf, (-np.inf if n > 1 else np.inf)
    want = _lse64(logits, n)
    assert np.isneginf(want[4]) and np.isposinf(want[r]) and np.isposinf(want[r + 1]) and np.isnan(want[r + 2])
    assert n == 1 or (np.isfinite(want[[0, 3, 5, 6]]).all() and np.isposinf(want[r + 4]))
    lse, _ = _row_lse_pick(dev, logits, n, None, None, False)
    _check_lse(lse, want, ("infinities", n))


def test_dense_head_with_minus_infinity_in_the_bias(dev):
    """gnnlm_dense_target_logp, route 2 with a bias (GEMM with bias_mode 1 + row_lse_pick): a bias of -inf at column 0 and at a
    column >= 256 masks those words; every other word's log-probability is finite and within the dense test's bar of float64."""
    import dense_head_ref
    import test_dense_head_gpu as tdh
    V, d, n = 513, 64, 300
    rs, x, w, b = tdh.make_inputs(5, V, d, n, True)
    b[0] = b[300] = -np.inf
    t = rs.randint(1, V, size=n).astype(np.int64)
    t[t == 300] = 301
    ds = tdh.build(dev, w, b, d, 2, 0)
    assert ds.route_name() == "general"
    got = ds.target_log_prob(torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
    logits = x.astype(np.float64) @ w.astype(np.float64).T + np.where(np.isinf(b), -np.inf, b.astype(np.float64))
    want = logits[np.arange(n), t] - torch.logsumexp(torch.from_numpy(logits), 1).numpy()
    assert np.isfinite(want).all()
    tdh.check(got, want, [], "route 2, bias with -inf")
