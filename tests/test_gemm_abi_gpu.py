"""gnnlm_gemm_nt and gnnlm_lse_reduce at the descriptor level (include/gnnlm.h: gnnlm_gemm_t): every kernel the dispatcher of
csrc/gemm_f32.hip can launch -- register-staged 64x64 and 128x128 tiles with their in-kernel split precisions, the scheduled kernel,
LDS-DMA 128 / 256 tiles, the A-stationary K = 64 kernel, the skinny kernel, the plane kernels at 128 / 256 tiles -- in the store and the
log-sum-exp flavour, against the numpy restatement of tests/gemm_ref.py.  Descriptors are filled by hand and passed to
``_lib.call_desc``; the table of cases is gemm_ref.CASES, and test_gemm_ref_cpu.py shows without a GPU that every case reaches the route
it names and notices every field it sets.

What EVERY call of this file carries (``lay_out`` / ``run``), so these rules are checked by every case and not by one:
  * lda = K + 4, ldw = K + 8 with NaN in the pad columns; the A panel is 7 rows taller than M; ldc = N + 1, ldr = N + 3;
  * A and W 16-byte aligned (the header's demand), C, R, bias and lse_picked ONE float off a 16-byte boundary, lse_part 8 bytes off;
  * every output buffer between guard bands; the buffer holds a NaN-payload sentinel (or the residual, in place): pad columns, rows
    beyond min(M, *m_dev), C rows no c_rows entry names, lse_part rows beyond the device count and lse_picked entries with a pick
    outside [0, N) must come back bit-identical;
  * every case runs twice into fresh buffers: the two results are equal bit for bit.

Exact data (small integers, dyadic alpha / bias / gate / R): every partial sum is exact in float32 in any order, so the whole output
equals the float64 reference at every precision and on every route -- no tolerance (the sign of a zero is unspecified).  The log-sum-exp
cases hold the maximum and the picked logit to the same rule; their A has three entries per row, so the logits are of order 1 and
sum exp keeps its accuracy.
Random data (normal operands, a range of 1e-2 .. 1e2 along k), error relative to |alpha| sum |a||b| + 1, the bars of
test_kernels_gpu.py::test_gemm_split_precisions and test_fp16_gpu.py: precision 0 and 2 5e-7, precision 1 4e-5, both against the
float64 product of the float32 operands; precision 3 5e-7 against the product of the operands rounded to half on the host.  Where a
case adds a gated bias and a residual, |gate * bias| + |R| join the scale: they are terms of the same float32 sum.  (Measured on
store-reg128-random_all, |gate * bias| up to 8.6 and |R| up to 5: a float32 numpy evaluation of the epilogue on the correctly rounded
product misses 5e-7 of |alpha| sum |a||b| + 1 with 7.06e-7 -- the kernel's own figure to three digits -- and has 1.3e-7 of the full scale.)
Log-sum-exp: per part, m + log s within 2e-5 of the float64 log-sum-exp of the part's columns (operands rounded as the header says for
the precision), and the value gnnlm_lse_reduce makes of the parts within 2e-5 as well."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gemm_ref as ref

pytestmark = pytest.mark.gpu

_SWITCHES = [v for v in ("GNNLM_GEMM_SCHED", "GNNLM_GEMM_SCHED_MINK", "GNNLM_GEMM_SKINNY") if v in os.environ]
if _SWITCHES:
    pytest.skip(f"gemm_ref.route() restates the dispatcher with {', '.join(_SWITCHES)} unset", allow_module_level=True)

GUARD = 64                                                            # floats in front of and behind every buffer
SENT_I = -0x0BADBEEF
E_INVALID = -22
BAR = {0: 5e-7, 1: 4e-5, 2: 5e-7, 3: 5e-7}
LSE_BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev_in(a, dev, off=0):
    """An input behind a guard band: NaN around float data, 0 (a valid index) around index arrays.  -> (tensor, pointer)"""
    a = np.ascontiguousarray(a)
    host = np.full(2 * GUARD + off + a.size, np.nan if a.dtype == np.float32 else 0, dtype=a.dtype)
    host[GUARD + off:GUARD + off + a.size] = a
    t = torch.from_numpy(host).to(dev)
    return t, t.data_ptr() + a.itemsize * (GUARD + off)


class Out:
    """An output between guard bands, ``off`` elements off the allocation's alignment; ``init``: its bytes before the call"""

    def __init__(self, init, dev, off):
        self.n, self.off, self.init = init.size, off, init
        fill = ref.sentinel(1)[0] if init.dtype == np.float32 else SENT_I
        host = np.full(2 * GUARD + off + init.size, fill, dtype=init.dtype)
        host[GUARD + off:GUARD + off + init.size] = init
        self.host0 = host
        self.t = torch.from_numpy(host).to(dev)
        self.ptr = self.t.data_ptr() + init.itemsize * (GUARD + off)

    def read(self):
        h = self.t.cpu().numpy()
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        view = (lambda x: x.view(np.uint32)) if h.dtype == np.float32 else (lambda x: x)
        assert np.array_equal(view(h[:lo]), view(self.host0[:lo])) and np.array_equal(view(h[hi:]), view(self.host0[hi:])), "guard band"
        return h[lo:hi]


def lay_out(d, dev):
    """-> (descriptor without outputs, tensors to keep alive, pointers of the inputs by name)"""
    from gnnlm_amd import _lib
    g, keep = _lib.gnnlm_gemm_t(), []

    def put(a, off=0):
        t, p = dev_in(a, dev, off)
        keep.append(t)
        return p

    g.A, g.W = put(d["A"]), put(d["W"])
    assert g.A % 16 == 0 and g.W % 16 == 0
    for f in ("lda", "ldw", "ldc", "ldr", "bias_mode", "M", "N", "K", "batch1", "batch2", "precision", "tile_order", "a_rows_bound",
              "sA1", "sA2", "sW1", "sW2", "sC1", "sC2", "sB1", "sB2", "sR1", "sR2"):
        setattr(g, f, int(d[f]))
    g.alpha = float(d["alpha"])
    for f in ("a_rows", "c_rows", "lse_pick"):
        if d[f] is not None:
            assert d[f].dtype == np.int32
            setattr(g, f, put(d[f]))
    for f in ("bias", "gate"):
        if d[f] is not None:
            setattr(g, f, put(d[f], 1))
    if d["R"] is not None and not isinstance(d["R"], str):
        g.R = put(d["R"], 1)
    if d["m_dev"] is not None:
        g.m_dev = put(np.array([d["m_dev"]], dtype=np.int32))
    return g, keep


def launch_once(g, d, dev):
    """One call into fresh output buffers -> dict of what came back (guards checked)"""
    from gnnlm_amd import _lib
    M, npart = d["M"], 2 * ref.cdiv(d["N"], 128)
    outs = {}
    if d["lse"]:
        outs["part"] = Out(ref.sentinel(M * npart * 2), dev, 2)
        g.lse_part = outs["part"].ptr
        if d["lse_pick"] is not None:
            outs["picked"] = Out(ref.sentinel(M), dev, 1)
            g.lse_picked = outs["picked"].ptr
    else:
        outs["C"] = Out(d["C"], dev, 1)
        g.C = outs["C"].ptr
        if isinstance(d["R"], str):
            g.R = g.C
    if d["m_out"]:
        outs["m_out"] = Out(np.full(1, SENT_I, dtype=np.int32), dev, 1)
        g.m_out = outs["m_out"].ptr
    _lib.call_desc("gnnlm_gemm_nt", g)
    torch.cuda.synchronize()
    got = {k: o.read() for k, o in outs.items()}
    if d["lse"]:
        mdev = None if d["m_dev"] is None else torch.tensor([d["m_dev"]], dtype=torch.int32, device=dev)
        lse = Out(ref.sentinel(M), dev, 1)
        _lib.call("gnnlm_lse_reduce", ctypes.c_void_p(outs["part"].ptr), npart, M, _lib.ptr(mdev), ctypes.c_void_p(lse.ptr), _lib.stream())
        torch.cuda.synchronize()
        got["lse"] = lse.read()
    return got


def run(d, dev, twice=True):
    g, keep = lay_out(d, dev)
    got = launch_once(g, d, dev)
    if twice:
        again = launch_once(g, d, dev)
        for k in got:
            assert np.array_equal(bits(got[k]), bits(again[k])), f"{k}: two runs differ"
    return got


def check(d, got, want, true=None, label=""):
    """``want``: gemm_ref(d); ``true``: the reference with unrounded operands (random data at precisions 1 and 2)"""
    exact, prec = d["exact"], d["precision"]
    if d["m_out"]:
        assert got["m_out"][0] == want["m_out"]
    if not d["lse"]:
        w = want["written"]
        assert np.array_equal(bits(got["C"])[~w], bits(d["C"])[~w]), "a byte outside the result was written"
        if exact:
            assert np.array_equal(got["C"][w], want["C"][w]), int((got["C"][w] != want["C"][w]).sum())
            return
        assert not (bits(got["C"])[w] == ref.SENT_BITS).any()
        judge = true if true is not None else want
        err = float((np.abs(got["C"][w].astype(np.float64) - judge["C64"][w]) / (judge["scale"][w] + 1.0)).max()) if w.any() else 0.0
        line = f"{label}: err {err:.3e} of the scale + 1 (bar {BAR[prec]:g})"
        if true is not None:
            line += f"; against the plane reference {float((np.abs(got['C'][w] - want['C64'][w]) / (want['scale'][w] + 1.0)).max()):.3e}"
        print(line)
        assert err < BAR[prec], line
        return
    M, mo, npart = d["M"], want["part_rows"], want["n_parts"]
    part = got["part"].reshape(M, npart, 2)
    assert (bits(part[mo:]) == ref.SENT_BITS).all(), "lse_part rows beyond the device count were written"
    assert not (bits(part[:mo]) == ref.SENT_BITS).any()
    wl, gl = ref.part_lse(want["part"][:mo]), ref.part_lse(part[:mo])
    empty = np.isneginf(wl)
    assert np.array_equal(part[:mo][empty], np.broadcast_to(np.float32([-np.inf, 0.0]), part[:mo][empty].shape)), "an empty part is (-inf, 0)"
    err = float(np.abs(gl[~empty] - wl[~empty]).max()) if (~empty).any() else 0.0
    red_w, red_g = ref.lse_reduce_ref(want["part"], d["m_dev"]), got["lse"]
    assert (bits(red_g[mo:]) == ref.SENT_BITS).all()
    err_red = float(np.abs(red_g[:mo] - red_w[:mo]).max()) if mo else 0.0
    err_pick = 0.0
    if d["lse_pick"] is not None:
        pw = want["picked_written"]
        assert (bits(got["picked"])[~pw] == ref.SENT_BITS).all(), "lse_picked written for a row beyond the count or a pick outside [0, N)"
        if exact:
            assert np.array_equal(got["picked"][pw], want["picked"][pw].astype(np.float32))
        elif pw.any():
            err_pick = float(np.abs(got["picked"][pw] - want["picked"][pw]).max())
    if exact:
        assert np.array_equal(part[:mo, :, 0], want["part"][:mo, :, 0].astype(np.float32)), "the maximum of exact logits is exact"
    line = f"{label}: part err {err:.3e}, reduced {err_red:.3e}, picked {err_pick:.3e} (bar {LSE_BAR:g})"
    print(line)
    assert err < LSE_BAR and err_red < LSE_BAR and err_pick < LSE_BAR, line


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("name", [c["name"] for c in ref.CASES])
def test_case(dev, name):
    spec = ref.CASE_BY_NAME[name]
    d = ref.make_case(spec)
    assert ref.route(d) == spec["route"]
    got = run(d, dev)
    prods = ref.case_products(spec, d)
    want = ref.gemm_ref(d, prods)
    true = None
    if not d["exact"] and not d["lse"] and d["precision"] in (1, 2):
        true = ref.gemm_ref(dict(d, precision=0))
    check(d, got, want, true, name)


@pytest.mark.parametrize("name", ref.TILE_ORDER_CASES)
def test_tile_order_never_changes_a_bit(dev, name):
    """tile_order 1, 2, 2 + GM (GM = 1, 4, 64: more m-tiles per band than there are, and a short last band) against tile_order 0
    on the same route: every output byte equal -- so every tile was visited exactly as under order 0, which test_case holds to
    the reference."""
    spec = ref.CASE_BY_NAME[name]
    d = ref.make_case(spec)
    assert spec["route"] in ref.WALKS
    base = run(d, dev, twice=False)
    for order in ref.TILE_ORDERS[1:]:
        dd = dict(d, tile_order=order)
        assert ref.route(dd) == spec["route"]
        got = run(dd, dev, twice=False)
        for k in base:
            assert np.array_equal(bits(got[k]), bits(base[k])), (order, k)


# ------------------------------------------------------------------------------------------ refusals
def _small(dev, lse=False):
    spec = dict(name="refusal", route=None, M=8, N=8, K=8, flavour="lse" if lse else "store")
    return ref.make_case(spec)


def _refused(d, dev, mutate=None, what=""):
    """The call returns GNNLM_E_INVALID with a message and writes nothing."""
    from gnnlm_amd import _lib
    g, keep = lay_out(d, dev)
    npart = 2 * ref.cdiv(d["N"], 128)
    outs = {"C": Out(ref.sentinel(d["M"] * (d["N"] + 1) + 16), dev, 1), "part": Out(ref.sentinel(d["M"] * npart * 2), dev, 2),
            "picked": Out(ref.sentinel(d["M"]), dev, 1), "m_out": Out(np.full(1, SENT_I, dtype=np.int32), dev, 1)}
    if d["lse"]:
        g.lse_part, g.lse_picked = outs["part"].ptr, outs["picked"].ptr
    else:
        g.C = outs["C"].ptr
    g.m_out = outs["m_out"].ptr
    extra = dev_in(np.ones(64, dtype=np.float32), dev, 1)
    idx = dev_in(np.arange(8, dtype=np.int32), dev)
    if mutate:
        mutate(g, extra[1], idx[1])
    rc = _lib.lib().gnnlm_gemm_nt(ctypes.byref(g), _lib.stream())
    torch.cuda.synchronize()
    assert rc == E_INVALID, (what, rc)
    assert _lib.lib().gnnlm_last_error().decode().startswith("invalid argument: gemm"), what
    for k, o in outs.items():
        assert np.array_equal(o.read().view(np.uint32), o.init.view(np.uint32)), (what, k)


REFUSALS = [
    ("K % 4", False, lambda g, f, i: setattr(g, "K", 6)),
    ("lda % 4", False, lambda g, f, i: setattr(g, "lda", 14)),
    ("ldw % 4", False, lambda g, f, i: setattr(g, "ldw", 18)),
    ("sA1 % 4", False, lambda g, f, i: setattr(g, "sA1", 2)),
    ("sA2 % 4", False, lambda g, f, i: setattr(g, "sA2", 6)),
    ("sW1 % 4", False, lambda g, f, i: setattr(g, "sW1", 1)),
    ("sW2 % 4", False, lambda g, f, i: setattr(g, "sW2", 3)),
    ("A 4 bytes off", False, lambda g, f, i: setattr(g, "A", g.A + 4)),
    ("W 8 bytes off", False, lambda g, f, i: setattr(g, "W", g.W + 8)),
    ("precision 4", False, lambda g, f, i: setattr(g, "precision", 4)),
    ("precision -1", False, lambda g, f, i: setattr(g, "precision", -1)),
    ("tile_order 67", False, lambda g, f, i: setattr(g, "tile_order", 67)),
    ("tile_order -1", False, lambda g, f, i: setattr(g, "tile_order", -1)),
    ("tile_order 67, LSE", True, lambda g, f, i: setattr(g, "tile_order", 67)),
    ("NULL A", False, lambda g, f, i: setattr(g, "A", None)),
    ("NULL W", False, lambda g, f, i: setattr(g, "W", None)),
    ("NULL C and lse_part", False, lambda g, f, i: setattr(g, "C", None)),
    ("N = 0", False, lambda g, f, i: setattr(g, "N", 0)),
    ("M < 0", False, lambda g, f, i: setattr(g, "M", -1)),
    ("batch with lse_part", True, lambda g, f, i: setattr(g, "batch1", 2)),
    ("batch2 with lse_part", True, lambda g, f, i: setattr(g, "batch2", 2)),
    ("alpha < 0 with lse_part", True, lambda g, f, i: setattr(g, "alpha", -1.0)),
    ("alpha NaN with lse_part", True, lambda g, f, i: setattr(g, "alpha", float("nan"))),
    ("bias with lse_part", True, lambda g, f, i: (setattr(g, "bias", f), setattr(g, "bias_mode", 1))),
    ("gate with lse_part", True, lambda g, f, i: setattr(g, "gate", f)),
    ("R with lse_part", True, lambda g, f, i: (setattr(g, "R", f), setattr(g, "ldr", 8))),
    ("c_rows with lse_part", True, lambda g, f, i: setattr(g, "c_rows", i)),
]


@pytest.mark.parametrize("what", [r[0] for r in REFUSALS])
def test_refused(dev, what):
    _, lse, mutate = [r for r in REFUSALS if r[0] == what][0]
    _refused(_small(dev, lse), dev, mutate, what)


def test_accepted_at_the_edges(dev):
    """M = 0 is accepted and touches nothing, m_out included; alpha = 0 is read as 1 in both flavours; C is ignored (may be any
    pointer) when lse_part is given."""
    from gnnlm_amd import _lib
    for lse in (False, True):
        d = dict(_small(dev, lse), M=0)
        g, keep = lay_out(d, dev)
        outs = {"C": Out(ref.sentinel(64), dev, 1), "part": Out(ref.sentinel(64), dev, 2), "m_out": Out(np.full(1, SENT_I, dtype=np.int32), dev, 1)}
        g.C, g.m_out = outs["C"].ptr, outs["m_out"].ptr
        if lse:
            g.lse_part = outs["part"].ptr
        _lib.call_desc("gnnlm_gemm_nt", g)
        torch.cuda.synchronize()
        for k, o in outs.items():
            assert np.array_equal(o.read().view(np.uint32), o.init.view(np.uint32)), (lse, k)
    d = _small(dev, True)
    assert d["alpha"] == 0.0
    g, keep = lay_out(d, dev)
    c = Out(ref.sentinel(128), dev, 1)
    g.C, g.ldc = c.ptr, 9
    got = launch_once(g, d, dev)
    check(d, got, ref.gemm_ref(d), None, "lse with a C pointer")
    assert np.array_equal(c.read().view(np.uint32), c.init.view(np.uint32)), "C is ignored when lse_part is given"


# ------------------------------------------------------------------------------------------ gnnlm_lse_reduce on its own
@pytest.mark.parametrize("n_parts", [1, 2, 1023, 1024, 1030])
def test_lse_reduce(dev, n_parts):
    """Hand-made parts: both kernels (one wave per row below 1024 parts, four from there on), (-inf, 0) parts among real ones, a
    row of (-inf, 0) parts only (its log-sum-exp is -inf), a device-side row count (rows beyond it untouched), rows = 0."""
    from gnnlm_amd import _lib
    rs = np.random.RandomState(n_parts)
    rows = 11
    part = np.empty((rows, n_parts, 2), dtype=np.float32)
    part[..., 0] = rs.standard_normal((rows, n_parts)) * 3
    part[..., 1] = 1.0 + 63.0 * rs.rand(rows, n_parts)                # a part's sum lies in [1, 64]
    hole = rs.rand(rows, n_parts) < 0.3
    hole[2] = True                                                    # a row without a column at all
    hole[3] = False
    part[hole] = (-np.inf, 0.0)
    part[5, :, 0] += 80.0                                             # a row whose exp(x) would overflow without the max
    p_t, p_ptr = dev_in(part.reshape(-1), dev, 2)
    for m_dev in (None, 0, 4, rows, rows + 3):
        want = ref.lse_reduce_ref(part, m_dev)
        m = rows if m_dev is None else min(rows, m_dev)
        out = Out(ref.sentinel(rows), dev, 1)
        md = None if m_dev is None else torch.tensor([m_dev], dtype=torch.int32, device=dev)
        _lib.call("gnnlm_lse_reduce", ctypes.c_void_p(p_ptr), n_parts, rows, _lib.ptr(md), ctypes.c_void_p(out.ptr), _lib.stream())
        torch.cuda.synchronize()
        got = out.read()
        assert (bits(got[m:]) == ref.SENT_BITS).all()
        if m > 2:
            assert got[2] == -np.inf and want[2] == -np.inf
        fin = np.isfinite(want[:m])
        assert np.array_equal(np.isfinite(got[:m]), fin)
        # float32: max exact, <= n_parts terms of relative error 2^-22 (expf, the product) summed, logf, one rounding of m + log s
        bar = 2.0 ** -21 * (np.abs(want[:m][fin]) + 8.0)
        assert (np.abs(got[:m][fin] - want[:m][fin]) <= bar).all(), float(np.abs(got[:m][fin] - want[:m][fin]).max())
    out = Out(ref.sentinel(4), dev, 1)
    _lib.call("gnnlm_lse_reduce", ctypes.c_void_p(p_ptr), n_parts, 0, None, ctypes.c_void_p(out.ptr), _lib.stream())
    torch.cuda.synchronize()
    assert (bits(out.read()) == ref.SENT_BITS).all()


# ------------------------------------------------------------------------------------------ the launched kernel by name
ROUTE_CASES = ["store-reg64-plain", "store-reg64ns3-plain", "store-reg128-plain", "store-reg128ns1-plain", "store-sched-plain",
               "store-dma128-plain", "store-dma256-plain", "store-skinny-plain", "store-split128p1-plain", "store-split256p2-plain",
               "lse-reg128-pick", "lse-reg128ns2-pick", "lse-sched-pick", "lse-dma128-pick", "lse-astat-pick", "lse-dma256-pick",
               "lse-split128p3-pick", "lse-split256p1-pick"]


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]


@pytest.mark.parametrize("name", ROUTE_CASES)
def test_route_is_the_launched_kernel(dev, name):
    """The device kernel torch's profiler sees is the one gemm_ref.route() names (function, and template arguments where the profiler
    spells them out)."""
    from gnnlm_amd import _lib
    spec = ref.CASE_BY_NAME[name]
    d = ref.make_case(spec)
    g, keep = lay_out(d, dev)
    launch_once(g, d, dev)                                            # first: the one-time set-up of the route (LDS opt-in, scratch)
    outs = Out(ref.sentinel(d["M"] * 2 * ref.cdiv(d["N"], 128) * 2), dev, 2) if d["lse"] else Out(d["C"], dev, 1)
    if d["lse"]:
        g.lse_part = outs.ptr
    else:
        g.C = outs.ptr
    names = [n for n in kernel_names(lambda: _lib.call_desc("gnnlm_gemm_nt", g)) if "gemm" in n]
    assert names, "torch's profiler reported no device kernel of the library"
    fn, targs = ref.kernel_symbol(spec["route"], d["lse"], d["precision"])
    hits = [n for n in names if fn + "<" in n or n.endswith(fn) or fn + "(" in n]
    assert len(hits) == 1 and not [n for n in names if n not in hits and "split_planes" not in n], (fn, names)
    if "<" in hits[0] and targs:
        spelled = hits[0][hits[0].index(fn + "<") + len(fn) + 1:].split(">")[0].replace(" ", "")
        assert spelled == ",".join(str(a) for a in targs), (hits[0], targs)
