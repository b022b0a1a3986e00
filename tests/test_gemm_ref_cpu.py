"""tests/gemm_ref.py is right before it judges a kernel, and the table of tests/test_gemm_abi_gpu.py reaches every kernel of the
dispatcher and can tell a kernel that ignores a descriptor field from one that honours it.  No GPU.

1. gemm_ref equals what the project already trusts: a plain float64 A @ W.T through every stride of the store flavour, and the head
   and tail log-probabilities of oracle.adaptive_softmax through the log-sum-exp flavour (parts -> lse_reduce_ref, picked logit).
   The plane splits of precisions 1 and 2 stay within the bars the kernels are held to; the three truncated planes add up exactly.
2. route() is the dispatcher: it is compared with gemm_route() of csrc/gemm_route.h itself (tests/gemm_route_main.cpp, built with the host
   compiler) over the edge shapes, the case table and a pair of shapes either side of every constant, under the three runtime switches
   too; the header's constants are gemm_ref's by value.  The 32-bit offset guards of the scheduled kernel are pinned here (no GPU case
   allocates 4 GiB).
3. tile_walk is a permutation of the tiles for every order; the one walk of the sources (gemm_route.h) is tile_walk.
4. For every case and every field it sets, the reference with that one field neutralised or shifted differs in the expected bytes.
5. Every case reaches the route it names; the table reaches every route route() can name, in both flavours where the route has both
   and at every precision the route serves; every route that walks tiles has a tile_order case in both flavours.
6. refusal() and the exact-data condition hold for the table."""
import collections
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gemm_ref as ref
from oracle import adaptive_softmax as oasm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gnn-lm_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def flat(text):
    return re.sub(r"[\s\\]+", "", text)


# ------------------------------------------------------------------------------------------ 1. what the project already trusts
def test_store_reference_is_a_plain_matmul():
    """Through batches with every stride its own, lda / ldw / ldc / ldr, a gather with zero rows, a scatter, both bias modes with a
    gate, the residual, alpha and the device-side row count: a loop over the elements, written from the header."""
    for name in ("store-reg64-batch_rows", "store-reg64-batch_bias2", "store-reg64-batch_bias1_R", "store-reg64-all", "store-reg64-random_all",
                 "store-reg64-c_rows_inplace", "store-reg64-batch_inplace", "store-reg64-batch_wbcast"):
        d = ref.make_case(ref.CASE_BY_NAME[name])
        p = ref.norm(d)
        got = ref.gemm_ref(d)
        M, N, K = p["M"], p["N"], p["K"]
        mo = M if p["m_dev"] is None else min(M, p["m_dev"])
        assert got["m_out"] == mo
        want = p["C"].astype(np.float64)
        hit = np.zeros(len(want), dtype=bool)
        init = p["C"]
        for b1 in range(p["batch1"]):
            for b2 in range(p["batch2"]):
                A = p["A"][b1 * p["sA1"] + b2 * p["sA2"]:]
                W = p["W"][b1 * p["sW1"] + b2 * p["sW2"]:]
                Wm = np.stack([W[n * p["ldw"]:n * p["ldw"] + K] for n in range(N)]).astype(np.float64)
                for r in range(mo):
                    ar = r if p["a_rows"] is None else int(p["a_rows"][r])
                    x = np.zeros(N) if ar < 0 else float(p["alpha"]) * (Wm @ A[ar * p["lda"]:ar * p["lda"] + K].astype(np.float64))
                    cr = r if p["c_rows"] is None else int(p["c_rows"][r])
                    if p["bias"] is not None:
                        g = 1.0 if p["gate"] is None else float(p["gate"][r])
                        b = p["bias"][b1 * p["sB1"] + b2 * p["sB2"]:]
                        x = x + g * (b[:N].astype(np.float64) if p["bias_mode"] == 1 else float(b[r]))
                    if p["R"] is not None:
                        R = init if isinstance(p["R"], str) else p["R"]
                        o = b1 * p["sR1"] + b2 * p["sR2"] + cr * p["ldr"]
                        x = x + R[o:o + N].astype(np.float64)
                    o = b1 * p["sC1"] + b2 * p["sC2"] + cr * p["ldc"]
                    want[o:o + N], hit[o:o + N] = x, True
        assert np.array_equal(hit, got["written"])
        assert np.array_equal(ref.bits(got["C"])[~hit], ref.bits(init)[~hit])
        tol = 1e-12 * (1.0 + np.abs(want[hit]))
        assert (np.abs(got["C64"][hit] - want[hit]) <= tol).all(), name
        assert hit.sum() == mo * N * p["batch1"] * p["batch2"] and (~hit).any()


def _asm_problem():
    w = oasm.init_adaptive_weights(700, 64, [150, 400], dtype=torch.float64)
    w = {k: ([None if t is None else t.float().double() for t in v] if isinstance(v, list) and k != "cutoff" else v) for k, v in w.items()}
    w["class_proj"] = w["class_proj"].float().double()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(50, 64, generator=g).double()
    target = torch.randint(0, 700, (50,), generator=g)
    return w, x, target


def _lse_desc(A, W, pick, alpha=0.0):
    M, K = A.shape
    N = W.shape[0]
    d = dict(ref.DESC_DEFAULTS)
    bufA = np.full(M * (K + 4), np.nan, dtype=np.float32)
    bufA.reshape(M, K + 4)[:, :K] = A
    bufW = np.full(N * (K + 8), np.nan, dtype=np.float32)
    bufW.reshape(N, K + 8)[:, :K] = W
    d.update(A=bufA, lda=K + 4, W=bufW, ldw=K + 8, M=M, N=N, K=K, lse=True, lse_pick=pick.astype(np.int32), a_panel_rows=M, alpha=alpha)
    return d


def test_lse_reference_is_the_adaptive_softmax_oracle():
    """Head: the log-sum-exp over [E_0; class_proj] and the picked logit give the oracle's log-probability of every band-0 target and
    of every tail's class.  Tails: the same over E_i of the projected rows.  The operands are float32 values on both sides; the tail
    input is rounded to float32 on the way into the descriptor, which moves a logit by at most 2^-24 sum |xi||e|."""
    w, x, target = _asm_problem()
    cut = w["cutoff"]
    want = oasm.target_log_prob(x, target, w).numpy()
    head_w = torch.cat([w["emb"][0], w["class_proj"]], 0).numpy()
    band = np.searchsorted(np.array(cut), target.numpy(), side="right")
    head_pick = np.where(band == 0, target.numpy(), cut[0] + band - 1)
    out = ref.gemm_ref(_lse_desc(x.numpy(), head_w, head_pick))
    assert out["n_parts"] == 2 * ref.cdiv(head_w.shape[0], 128) and out["picked_written"].all()
    logp = out["picked"] - ref.lse_reduce_ref(out["part"])
    in0 = band == 0
    assert in0.any() and (~in0).any()
    assert np.abs(logp[in0] - want[in0]).max() < 1e-12
    for i in range(1, len(cut)):
        m = band == i
        assert m.any()
        xi = (x[torch.from_numpy(m)] @ w["proj"][i]).numpy()
        e = w["emb"][i].numpy()
        t = ref.gemm_ref(_lse_desc(xi.astype(np.float32), e, target.numpy()[m] - cut[i - 1]))
        tail = t["picked"] - ref.lse_reduce_ref(t["part"])
        bar = 2 * 2.0 ** -24 * float((np.abs(xi) @ np.abs(e).T).max()) + 1e-12
        assert np.abs(logp[m] + tail - want[m]).max() < bar
    # alpha scales the logits before the softmax; every part pairs alpha * max with the sum over the part
    d = _lse_desc(x.numpy(), head_w, head_pick, alpha=0.5)
    half = ref.gemm_ref(d)
    logits = 0.5 * (x.numpy() @ head_w.T)
    for p in range(half["n_parts"]):
        sl = logits[:, 64 * p:64 * p + 64]
        if sl.shape[1] == 0:
            assert np.isneginf(half["part"][:, p, 0]).all() and (half["part"][:, p, 1] == 0).all()
            continue
        assert np.allclose(half["part"][:, p, 0], sl.max(1), rtol=1e-15) and np.allclose(half["part"][:, p, 1], np.exp(sl - sl.max(1, keepdims=True)).sum(1), rtol=1e-13)
    assert np.isneginf(half["part"][:, -1, 0]).all()                  # 152 columns: the fourth part is empty


def test_lse_reference_rules():
    rs = np.random.RandomState(0)
    A, W = rs.standard_normal((6, 8)).astype(np.float32), rs.standard_normal((130, 8)).astype(np.float32)
    pick = np.array([0, 129, 130, -1, 64, 63])
    d = _lse_desc(A, W, pick)
    d["m_dev"] = 5
    out = ref.gemm_ref(d)
    assert out["m_out"] == out["part_rows"] == 5 and out["part"].shape == (6, 4, 2)
    assert np.isnan(out["part"][5]).all() and not np.isnan(out["part"][:5]).any()
    assert list(out["picked_written"]) == [True, True, False, False, True, False]          # outside [0, N) and beyond the count
    assert np.isneginf(out["part"][:5, 3, 0]).all() and (out["part"][:5, 3, 1] == 0).all()
    assert (out["part"][:5, 2, 1] >= 1).all() and (out["part"][:5, 2, 1] <= 2).all()       # two columns in the third part
    lse = ref.lse_reduce_ref(out["part"], 5)
    x = A.astype(np.float64) @ W.astype(np.float64).T
    assert np.allclose(lse[:5], np.log(np.exp(x[:5]).sum(1)), rtol=1e-13) and np.isnan(lse[5])
    assert ref.lse_reduce_ref(np.array([[[-np.inf, 0.0]] * 3]))[0] == -np.inf              # a row of empty parts
    d["a_rows"] = np.array([0, 1, -1, 2, 3, 4], dtype=np.int32)
    with pytest.raises(AssertionError):                                                   # LSE: every a_rows entry must be >= 0
        ref.gemm_ref(d)
    for m_dev, mo in ((0, 0), (5, 5), (6, 6), (11, 6)):                                    # a count above M is M
        assert ref.m_effective(dict(d, m_dev=m_dev)) == mo
    with pytest.raises(AssertionError):                                                   # a negative count is outside the contract
        ref.m_effective(dict(d, m_dev=-3))


@pytest.mark.parametrize("precision,bar", [(1, 4e-5), (2, 5e-7), (3, None)])
def test_operand_planes(precision, bar):
    """bf16x6: three truncated planes add up to the value exactly; bf16x3: value and residual rounded to nearest, 2^-17 of the value
    left over; the kept cross products stay within the bar the kernels are held to against the unrounded product.  fp16: numpy's
    float16 cast (nearest even, overflow to infinity)."""
    rs = np.random.RandomState(precision)
    K = 256
    x = (rs.standard_normal((64, K)) * np.logspace(-2, 2, K)).astype(np.float32)
    pl = ref.planes(x, precision)
    if precision == 3:
        assert len(pl) == 1 and np.array_equal(pl[0], x.astype(np.float16).astype(np.float32))
        big = ref.planes(np.float32([65504.0, 65519.9, 65520.0, -70000.0, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]), 3)[0]
        assert np.array_equal(big, np.float32([65504.0, 65504.0, np.inf, -np.inf, 0.0, 1.0, 1.0 + 2.0 ** -9]))
        return
    assert len(pl) == precision + 1
    for p in pl:
        assert (ref.bits(p) & 0xFFFF == 0).all()                                           # bf16 values
    total = sum(p.astype(np.float64) for p in pl)
    if precision == 2:
        assert np.array_equal(total, x.astype(np.float64))
    else:
        assert (np.abs(total - x) <= 2.0 ** -17 * np.abs(x)).all() and (np.abs(pl[0] - x) <= 2.0 ** -8 * np.abs(x)).all()
    w = rs.standard_normal((48, K)).astype(np.float32)
    d = dict(ref.DESC_DEFAULTS)
    d.update(A=x.reshape(-1), lda=K, W=w.reshape(-1), ldw=K, M=64, N=48, K=K, a_panel_rows=64, c_panel_rows=64, C=ref.sentinel(64 * 48), ldc=48)
    true = ref.gemm_ref(d)
    got = ref.gemm_ref(dict(d, precision=precision))
    err = (np.abs(got["C64"] - true["C64"]) / (true["scale"] + 1.0)).max()
    assert 0 < err < bar / 2, err


# ------------------------------------------------------------------------------------------ 2. the dispatcher itself
CONSTANTS = ("DMA_BK", "DMA_BIG_TILES", "DMA_MIN_K", "DMA_STORE_MIN_K", "ASTAT_K", "ASTAT_MAX_M", "SCHED_MIN_K", "SCHED_K_MULT",
             "SCHED_HEAD_TILES", "SKINNY_MAX_N", "SKINNY_K_MULT", "SKINNY_MIN_K", "SPLIT_MIN_K", "SPLIT_MIN_TILES", "SPLIT_BIG_TILES",
             "SPLIT_MDEV_BIG_M", "SMALL_TILES")


@pytest.fixture(scope="module")
def route_program(tmp_path_factory):
    """tests/gemm_route_main.cpp: csrc/gemm_route.h behind a command line, built with the host compiler alone"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("gemm_route") / "gemm_route_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_route_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(exe, *args, stdin="", env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GNNLM_GEMM_")}
    e.update(env or {})
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


def real_routes(exe, descs, env=None):
    """[(route name, resolved tile_order)] of gemm_route() / gemm_tile_order() for normalised descriptors"""
    lines = []
    for d in descs:
        p = ref.norm(d)
        lines.append(" ".join(str(int(x)) for x in (
            p["M"], p["N"], p["K"], p["precision"], bool(p["lse"]), p["m_dev"] is not None, p["batch1"], p["batch2"], p["lda"], p["ldw"],
            p["a_rows"] is not None, p["a_rows_bound"], p["tile_order"])))
    out = [l.split() for l in ask(exe, "route", stdin="\n".join(lines) + "\n", env=env)]
    assert len(out) == len(descs)
    return [(r, int(o)) for r, o in out]


def _shape(M, N, K, **kw):
    d = dict(ref.DESC_DEFAULTS)
    d.update(A=True, W=True, C=True, M=M, N=N, K=K, lda=K, ldw=K)
    d.update(kw)
    return d


_BIG = dict(M=2050, N=1990)
_G = dict(a_rows=True, K=256, **_BIG)
# (descriptor, the route it must take): one step to either side of every constant, written by hand
EDGES = [
    (_shape(K=256, **_BIG), "sched128"), (_shape(K=192, **_BIG), "reg128"), (_shape(K=288, **_BIG), "reg128"),
    (_shape(K=320, **_BIG), "sched128"), (_shape(K=256, precision=3, **_BIG), "split128"),
    (_shape(K=252, precision=3, **_BIG), "reg128"),
    (_shape(2048, 2048, 256), "sched128"), (_shape(2048, 1920, 256), "reg64"),             # 256 / 240 tiles of 128
    (_shape(2048, 1920, 256, lse=True), "dma128"),                                              # LSE is never small
    (_shape(2048, 1920, 256, precision=1), "reg64"),
    (_shape(K=544, **_BIG), "dma128"), (_shape(K=544, m_dev=5, **_BIG), "reg128"),
    (_shape(K=480, **_BIG), "reg128"), (_shape(K=512 + 32, batch1=2, **_BIG), "dma128"),
    (_shape(257, 261, 128, batch1=16, batch2=32), "dma256"), (_shape(257, 261, 128, batch1=16, batch2=31), "reg128"),
    (_shape(257, 261, 96, batch1=16, batch2=32), "reg128"),
    (_shape(2049, 58200, 128, lse=True), "dma256"), (_shape(2048, 58200, 128, lse=True), "dma128"),
    (_shape(2049, 58200, 256, lse=True), "dma256"), (_shape(2049, 58200, 256, lse=True, m_dev=9), "sched128"),
    (_shape(129, 300, 64, lse=True), "astat128"), (_shape(129, 300, 64, lse=True, precision=3), "reg128"),
    (_shape(128 * 768, 300, 64, lse=True), "astat128"), (_shape(128 * 768 + 1, 300, 64, lse=True), "reg128"),
    (_shape(129, 300, 96, lse=True), "reg128"), (_shape(129, 300, 128, lse=True), "dma128"),
    (_shape(129, 300, 64), "reg64"),
    (_shape(70, 256, 512), "skinny32"), (_shape(70, 257, 512), "reg64"), (_shape(70, 256, 480), "reg64"),
    (_shape(70, 256, 528), "reg64"), (_shape(70, 256, 512, batch2=2), "reg64"),
    (_shape(70, 256, 512, precision=2), "reg64"), (_shape(70, 256, 512, lse=True), "dma128"),
    (_shape(100000, 256, 512), "skinny32"),                                                     # never from the row count
    (_shape(5900, 5900, 256, precision=1), "split256"), (_shape(5900, 5632, 256, precision=1), "split256"),    # 24 x 22 = 528, 24 x 21 = 504
    (_shape(5900, 5376, 256, precision=1), "split128"),
    (_shape(5900, 5900, 256, precision=1, m_dev=1), "split128"),
    (_shape(1 << 17, 300, 256, precision=2, m_dev=1), "split256"), (_shape((1 << 17) - 1, 300, 256, precision=2, m_dev=1), "split128"),
    (_shape(0, 5, 8), "none"),
    # the 32-bit byte offsets of the scheduled kernel: N * ldw * 4 and a_rows_bound * lda * 4 below 2^32
    (_shape(300, 1 << 20, 256, ldw=1020), "sched128"), (_shape(300, 1 << 20, 256, ldw=1024), "dma256"),
    (_shape(1 << 20, 300, 256, lda=1020), "sched128"), (_shape(1 << 20, 300, 256, lda=1024), "dma256"),
    (_shape(a_rows_bound=0, **_G), "reg128"), (_shape(a_rows_bound=5, **_G), "sched128"),
    (_shape(a_rows_bound=1 << 22, **_G), "reg128"), (_shape(a_rows_bound=(1 << 22) - 1, **_G), "sched128"),
    (_shape(a_rows_bound=0, lse=True, **_G), "dma128"),
]
HEAD = _shape(2049, 58200, 256, lse=True)                              # the head shape of EDGES: >= 2048 tiles of 256, no m_dev
assert any(d == HEAD for d, _ in EDGES)

# per constant, two shapes one step either side of it (and the routes that tells them apart)
PAIRS = {
    "DMA_BK": ((_shape(K=544, **_BIG), "dma128"), (_shape(K=548, **_BIG), "reg128")),
    "DMA_BIG_TILES": ((_shape(257, 261, 128, batch1=16, batch2=32), "dma256"), (_shape(257, 261, 128, batch1=16, batch2=31), "reg128")),
    "DMA_MIN_K": ((_shape(129, 300, 128, lse=True), "dma128"), (_shape(129, 300, 96, lse=True), "reg128")),
    "DMA_STORE_MIN_K": ((_shape(K=544, **_BIG), "dma128"), (_shape(K=480, **_BIG), "reg128")),
    "ASTAT_K": ((_shape(129, 300, 64, lse=True), "astat128"), (_shape(129, 300, 68, lse=True), "reg128")),
    "ASTAT_MAX_M": ((_shape(128 * 768, 300, 64, lse=True), "astat128"), (_shape(128 * 768 + 1, 300, 64, lse=True), "reg128")),
    "SCHED_MIN_K": ((_shape(K=256, **_BIG), "sched128"), (_shape(K=192, **_BIG), "reg128")),
    "SCHED_K_MULT": ((_shape(K=320, **_BIG), "sched128"), (_shape(K=288, **_BIG), "reg128")),
    "SCHED_HEAD_TILES": ((_shape(2048, 58200, 256, lse=True), "sched128"), (HEAD, "dma256")),     # 8 x 228 = 1824, 9 x 228 = 2052
    "SKINNY_MAX_N": ((_shape(70, 256, 512), "skinny32"), (_shape(70, 257, 512), "reg64")),
    "SKINNY_K_MULT": ((_shape(70, 256, 544), "skinny32"), (_shape(70, 256, 528), "reg64")),
    "SKINNY_MIN_K": ((_shape(70, 256, 512), "skinny32"), (_shape(70, 256, 480), "reg64")),
    "SPLIT_MIN_K": ((_shape(K=256, precision=3, **_BIG), "split128"), (_shape(K=252, precision=3, **_BIG), "reg128")),
    "SPLIT_MIN_TILES": ((_shape(2048, 2048, 256, precision=1), "split128"), (_shape(2048, 1920, 256, precision=1), "reg64")),
    "SPLIT_BIG_TILES": ((_shape(5900, 5632, 256, precision=1), "split256"), (_shape(5900, 5376, 256, precision=1), "split128")),
    "SPLIT_MDEV_BIG_M": ((_shape(1 << 17, 300, 256, precision=2, m_dev=1), "split256"),
                         (_shape((1 << 17) - 1, 300, 256, precision=2, m_dev=1), "split128")),
    "SMALL_TILES": ((_shape(2048, 2048, 192), "reg128"), (_shape(2048, 1920, 192), "reg64")),
}


def _all_shapes():
    cases = [ref.shape_desc(c)[0] for c in ref.CASES]
    cases = [dict(d, alpha=0.0) if isinstance(d["alpha"], str) else d for d in cases]      # "unit": a value make_case() works out
    return [d for d, _ in EDGES] + cases + [d for pair in PAIRS.values() for d, _ in pair]


def test_route_constants_are_the_sources(route_program):
    """gemm_ref.route() against the dispatcher itself (csrc/gemm_route.h: gemm_route, gemm_tile_order), and the header's constants
    against gemm_ref's, by value."""
    got = dict(l.split() for l in ask(route_program, "constants"))
    assert set(got) == set(CONSTANTS) | {"MAX_TILE_ORDER"} and set(PAIRS) == set(CONSTANTS) and len(CONSTANTS) == 17
    for name in got:
        assert int(got[name]) == getattr(ref, name), name
    for name, pair in PAIRS.items():                                   # the pairs straddle: two routes, as written
        assert pair[0][1] != pair[1][1] and [ref.route(d) for d, _ in pair] == [r for _, r in pair], name
    shapes = _all_shapes()
    real = real_routes(route_program, shapes)
    for d, (rt, order) in zip(shapes, real):
        assert rt == ref.route(d), (d, rt)
        assert order == ref.resolved_tile_order(d), d
    for (d, want), (rt, _) in zip(EDGES, real):                       # (the hand-written expectations, asked of the code too)
        assert rt == want, d
    # the three runtime switches
    lse = [bool(d["lse"]) for d in shapes]
    base = [r for r, _ in real]
    assert "sched128" in base and "skinny32" in base and any(r == "sched128" and l for r, l in zip(base, lse))
    off = [r for r, _ in real_routes(route_program, shapes, env={"GNNLM_GEMM_SCHED": "0"})]
    assert "sched128" not in off and all(a == b for a, b in zip(off, base) if b != "sched128")
    one = [r for r, _ in real_routes(route_program, shapes, env={"GNNLM_GEMM_SCHED": "1"})]
    assert not any(r == "sched128" and l for r, l in zip(one, lse)) and any(r == "sched128" for r in one)
    assert all(a == b for a, b, l in zip(one, base, lse) if not l)
    assert real_routes(route_program, [HEAD])[0][0] == "dma256"
    assert real_routes(route_program, [HEAD], env={"GNNLM_GEMM_SCHED": "7"})[0][0] == "sched128"
    noskinny = [r for r, _ in real_routes(route_program, shapes, env={"GNNLM_GEMM_SKINNY": "0"})]
    assert "skinny32" not in noskinny and all(a == b for a, b in zip(noskinny, base) if b != "skinny32")
    k256, k512 = _shape(K=256, **_BIG), _shape(K=512, **_BIG)
    assert [r for r, _ in real_routes(route_program, [k256, k512])] == ["sched128", "sched128"]
    assert [r for r, _ in real_routes(route_program, [k256, k512], env={"GNNLM_GEMM_SCHED_MINK": "512"})] == ["reg128", "sched128"]
    # what the sources still say in text: the log-sum-exp flavour exists for 128-wide tiles only (LSE is never `small`), the
    # A-stationary kernel is written for one K, and lse_reduce's choice of kernel
    main, dma = src("gemm_f32.hip"), src("gemm_f32_dma.hip")
    assert "if constexpr (BN == 128) {" in main
    assert "gemm_lse_astationary_kernel<ASTAT_K>" in dma and "static_assert(K == 64" in dma and ref.ASTAT_K == 64
    red = main[main.index("int lse_reduce("):]
    assert "if (n_parts >= 1024)" in red


def test_refusals_are_the_sources():
    """every GNNLM_REQUIRE of gemm_nt() has its line in refusal()"""
    main = src("gemm.hip")
    body = main[main.index("int gemm_nt(const GemmParams& desc"):main.index("if (p.M == 0) return OK;")]
    msgs = re.findall(r'GNNLM_REQUIRE\(.*?"gemm: ([^"]*)"\);', body)
    assert len(msgs) == 11
    ok = ref.make_case(dict(name="r", route=None, M=8, N=8, K=8))
    lse = ref.make_case(dict(name="r", route=None, M=8, N=8, K=8, flavour="lse"))
    one = np.ones(8, dtype=np.float32)
    bad = [(ok, dict(A=None)), (ok, dict(W=None)), (ok, dict(C=None)), (ok, dict(M=-1)), (ok, dict(N=0)), (ok, dict(K=0)), (ok, dict(K=6)),
           (ok, dict(lda=10)), (ok, dict(ldw=18)), (ok, dict(sA1=2)), (ok, dict(sA2=2)), (ok, dict(sW1=2)), (ok, dict(sW2=2)),
           (ok, dict(batch1=-1)), (ok, dict(precision=4)), (ok, dict(precision=-1)), (ok, dict(tile_order=67)), (ok, dict(tile_order=-1)),
           (lse, dict(batch1=2)), (lse, dict(batch2=3)), (lse, dict(alpha=-1.0)), (lse, dict(alpha=float("nan"))),
           (lse, dict(bias=one)), (lse, dict(gate=one)), (lse, dict(R=one)), (lse, dict(c_rows=np.arange(8, dtype=np.int32)))]
    assert ref.refusal(ok) is None and ref.refusal(lse) is None
    seen = set()
    for d, change in bad:
        why = ref.refusal(dict(d, **change))
        assert why is not None, change
        assert any(why in m or m.startswith(why) for m in msgs), (why, msgs)
        seen.add(why)
    assert len(seen) == len(msgs) - 1 and "operands must be 16-byte aligned" in msgs      # (pointers: the GPU test's to try)
    for change in (dict(alpha=0.0), dict(alpha=-0.0), dict(tile_order=66), dict(precision=3), dict(m_dev=0), dict(M=0)):
        assert ref.refusal(dict(lse, **change)) is None, change


def test_route_edges():
    """One step to either side of every constant."""
    for d, want in EDGES:
        assert ref.route(d) == want, d
    # tile_order: resolved before the dispatch, never part of it
    assert ref.resolved_tile_order(_shape(10, 9, 8)) == 1 and ref.resolved_tile_order(_shape(9, 9, 8)) == 2
    assert ref.resolved_tile_order(_shape(10, 9, 8, m_dev=3)) == 2 and ref.resolved_tile_order(_shape(10, 9, 8, tile_order=6)) == 6
    for c in ref.CASES[::7]:
        d = ref.shape_desc(c)[0]
        assert len({ref.route(dict(d, tile_order=o)) for o in ref.TILE_ORDERS}) == 1


# ------------------------------------------------------------------------------------------ 3. the tile walk
@pytest.mark.parametrize("tile_order", [1, 2, 3, 4, 6, 9, 66])
def test_tile_walk_is_a_permutation(tile_order):
    for tiles_m in (1, 2, 5, 17):
        for tiles_n in (1, 3, 16):
            walk = ref.tile_walk(tile_order, tiles_m, tiles_n)
            assert sorted(walk) == [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n)], (tiles_m, tiles_n)
            if tile_order > 2:                                        # bands of GM m-tiles, n slow inside a band, m fastest
                GM = tile_order - 2
                assert [tm // GM for tm, _ in walk] == sorted(tm // GM for tm, _ in walk)
                assert walk[:min(GM, tiles_m)] == [(tm, 0) for tm in range(min(GM, tiles_m))]
    assert ref.tile_walk(1, 2, 3) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)]
    assert ref.tile_walk(2, 2, 3) == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)]
    assert ref.tile_walk(4, 3, 2) == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 1)]      # GM = 2: a short last band


def test_the_four_kernels_spell_one_walk(route_program):
    """One walk, in csrc/gemm_route.h: it is ref.tile_walk, and no kernel file decodes tile_order itself."""
    for tile_order in (1, 2, 3, 4, 6, 9, 66):                          # the orders and tile counts of test_tile_walk_is_a_permutation
        for tiles_m in (1, 2, 5, 17):
            for tiles_n in (1, 3, 16):
                got = [tuple(int(x) for x in l.split()) for l in ask(route_program, "walk", str(tile_order), str(tiles_m), str(tiles_n))]
                assert got == ref.tile_walk(tile_order, tiles_m, tiles_n), (tile_order, tiles_m, tiles_n)
    files = sorted(f for f in os.listdir(CSRC) if f.startswith("gemm") and f.endswith(".hip"))
    assert {"gemm.hip", "gemm_f32.hip", "gemm_f32_sched.hip", "gemm_f32_dma.hip", "gemm_f32_skinny.hip", "gemm_split.hip"} <= set(files)
    for f in files:
        assert "tile_order ==" not in src(f) and "tile_order==" not in flat(src(f)), f
    walkers = [f for f in files if "gemm_tile_walk(" in src(f) or "GNNLM_TILE_WALK(" in src(f)]
    assert walkers == ["gemm_f32.hip", "gemm_f32_dma.hip", "gemm_f32_sched.hip", "gemm_split.hip"]
    # the two kernels without a walk do not read the field
    assert "tile_order" not in src("gemm_f32_skinny.hip")
    astat = src("gemm_f32_dma.hip")
    astat = astat[astat.index("void gemm_lse_astationary_kernel"):astat.index("int launch_dma(")]
    assert "tile_order" not in astat and "void gemm_nt_f32_dma_kernel" not in astat


# ------------------------------------------------------------------------------------------ 4. no case is blind to a field it sets
def expected_bytes(d, prods):
    out = ref.gemm_ref(d, prods, strict=False)
    if d["lse"]:
        return out["part"].tobytes() + out["picked"].tobytes() + out["picked_written"].tobytes() + (bytes([out["m_out"] % 251]) if d["m_out"] else b"")
    return ref.bits(out["C"]).tobytes() + (bytes([out["m_out"] % 251]) if d["m_out"] else b"")


def mutations(d):
    """(field, mutated descriptor, products still valid) for every field the case sets"""
    M, N = d["M"], d["N"]
    mo = ref.m_effective(d)
    nb = (d["batch1"] or 1) * (d["batch2"] or 1)
    out = []
    if d["m_dev"] is not None:
        out.append(("m_dev", dict(d, m_dev=M - 1) if mo == M else dict(d, m_dev=None), True))
        if d["m_dev"] > M:
            out.append(("m_dev clamp", dict(d, M=M - 1, **({"lse_pick": d["lse_pick"][:M - 1]} if d["lse_pick"] is not None else {})), True))
    if d["m_out"]:
        out.append(("m_out", dict(d, m_out=False), True))
    if mo == 0:
        return out
    last_row = mo - 1 if d["c_rows"] is None else int(d["c_rows"][:mo].max())             # row 0 alone: no leading dimension matters
    if d["a_rows"] is not None:
        a = d["a_rows"]
        out.append(("a_rows", dict(d, a_rows=None) if not np.array_equal(a[:mo], np.arange(mo)) else dict(d, a_rows=np.roll(a, 1)), True))
        if (a[:mo] < 0).any():
            out.append(("a_rows < 0", dict(d, a_rows=np.maximum(a, 0)), True))
    if d["c_rows"] is not None:
        out.append(("c_rows", dict(d, c_rows=None), True))
    if d["bias"] is not None:
        out.append(("bias", dict(d, bias=None), True))
        out.append(("bias values", dict(d, bias=d["bias"] * 2), True))
        if M != N:
            n = max(M, N) + max(d["sB1"] * ((d["batch1"] or 1) - 1) + d["sB2"] * ((d["batch2"] or 1) - 1), 0)
            wide = np.resize(d["bias"], n)
            out.append(("bias_mode", dict(d, bias=wide, bias_mode=3 - d["bias_mode"]), True))
        for s in ("sB1", "sB2"):
            if d[s]:
                out.append((s, dict(d, **{s: 0}), True))
    if d["gate"] is not None:
        out.append(("gate", dict(d, gate=None), True))
    if d["R"] is not None:
        out.append(("R", dict(d, R=None), True))
        if not isinstance(d["R"], str):
            if last_row:
                out.append(("ldr", dict(d, ldr=d["ldc"]), True))
            for s in ("sR1", "sR2"):
                if d[s]:
                    out.append((s, dict(d, **{s: 0}), True))
    if np.float32(d["alpha"]) != 0:
        out.append(("alpha", dict(d, alpha=0.0), True))
    if not d["lse"]:
        if last_row:
            out.append(("ldc", dict(d, ldc=N), True))
        for s in ("sC1", "sC2"):
            if d[s]:
                out.append((s, dict(d, **{s: 0}), True))
    if d["lse_pick"] is not None:
        out.append(("lse_pick", dict(d, lse_pick=None), True))
        out.append(("lse_pick values", dict(d, lse_pick=d["lse_pick"] + 1), True))
    if M * N * d["K"] * nb <= 3e8:                                     # (the big shapes: the same code reads lda / ldw / the strides)
        if (mo > 1 if d["a_rows"] is None else d["a_rows"][:mo].max() > 0):
            out.append(("lda", dict(d, lda=d["K"]), False))
        if N > 1:
            out.append(("ldw", dict(d, ldw=d["K"]), False))
        for s in ("sA1", "sA2", "sW1", "sW2"):
            if d[s]:
                out.append((s, dict(d, **{s: 0}), False))
        if not d["exact"] and d["precision"]:
            out.append(("precision", dict(d, precision=0), False))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in ref.CASES])
def test_every_case_notices_every_field_it_sets(name):
    spec = ref.CASE_BY_NAME[name]
    d = ref.make_case(spec)
    assert ref.route(d) == spec["route"] and ref.refusal(d) is None
    if d["exact"]:
        assert ref.check_exact(d)
    prods = ref.case_products(spec, d) if ref.m_effective(d) else None
    # the fields act per row and per batch: the first 300 rows and the first two batch1 panels tell as much as all of them
    d = dict(d, M=min(d["M"], 300), batch1=min(d["batch1"], 2))
    base = expected_bytes(d, prods)
    muts = mutations(d)
    s = dict(ref.SPEC_DEFAULTS)
    s.update(spec)
    claimed = {"a_rows": s["a_rows"], "c_rows": s["c_rows"], "bias": s["bias_mode"], "gate": s["gate"], "R": s["R"], "m_dev": s["m_dev"] is not None,
               "lse_pick": s["pick"], "alpha": s["alpha"], "sA1": (s["batch"][0] or 1) * (s["batch"][1] or 1) > 1}
    names = {m[0] for m in muts}
    for f, on in claimed.items():
        if on and (ref.m_effective(d) or f == "m_dev") and not (f.startswith("sA") and "lda" not in names):
            assert f in names, f
    for field, dd, keep in muts:
        assert expected_bytes(dd, prods if keep else None) != base, field


# ------------------------------------------------------------------------------------------ 5. the table reaches every route
def test_route_coverage(capsys):
    count = collections.Counter((c["route"], ref.flavour_of(c), c.get("precision", 0), c.get("data", "exact")) for c in ref.CASES)
    both = ("exact", "random")
    need = []
    for rt in ("reg64", "reg128"):
        for prec in (0, 1, 2, 3):
            need += [(rt, "store", prec, k) for k in both]
    need += [("reg128", "lse", prec, k) for prec in (0, 1, 2, 3) for k in both]
    for rt in ("sched128", "dma128"):
        need += [(rt, fl, 0, k) for fl in ("store", "lse") for k in both]
    need += [("dma256", "store", 0, "exact"), ("dma256", "lse", 0, "exact")]            # the big tiles: exact data (the reference's cost)
    need += [("astat128", "lse", 0, k) for k in both] + [("skinny32", "store", 0, k) for k in both]
    need += [("split128", fl, prec, k) for fl in ("store", "lse") for prec in (1, 2, 3) for k in both]
    need += [("split256", "store", prec, k) for prec in (1, 2, 3) for k in both] + [("split256", "lse", prec, "exact") for prec in (1, 2, 3)]
    for n in need:
        assert count[n] > 0, n
    assert {k[:3] for k in count} == {n[:3] for n in need}             # and route() names nothing else for the table
    with capsys.disabled():
        per = collections.Counter((c["route"], ref.flavour_of(c)) for c in ref.CASES)
        print("\ncases per route and flavour:", ", ".join(f"{r}/{f} {n}" for (r, f), n in sorted(per.items())), f"-- {len(ref.CASES)} in all")
    walks = {(ref.CASE_BY_NAME[n]["route"], ref.flavour_of(ref.CASE_BY_NAME[n])) for n in ref.TILE_ORDER_CASES}
    assert walks == {(r, f) for r in ref.WALKS for f in ("store", "lse")} - {("reg64", "lse")}
    for n in ref.TILE_ORDER_CASES:                                    # more than one tile each way, so an order can go wrong
        c = ref.CASE_BY_NAME[n]
        t = ref.ROUTE_TILE[c["route"]]
        assert ref.cdiv(c["M"], t) > 1 and ref.cdiv(c["N"], t) > 1, n
    # m_dev = 0, 1, M - 1, M and M + 5 on every route of both flavours that takes a device-side count at its shape
    for fl, routes in (("store", ("reg64", "reg128", "skinny32", "split128")), ("lse", ("reg128", "sched128", "dma128", "astat128", "split128"))):
        for rt in routes:
            seen = {c.get("m_dev") for c in ref.CASES if c["route"] == rt and ref.flavour_of(c) == fl}
            assert {0, 1, "M-1", "M+0", "M+5"} <= seen, (fl, rt, seen)
    assert {"sched128"} <= {c["route"] for c in ref.CASES if c.get("m_dev") == "M-1" and ref.flavour_of(c) == "store"}
    # a_rows with a real bound and with bound 0 on the scheduled kernel's shape: both routes shown
    assert ref.CASE_BY_NAME["store-sched-a_neg"]["route"] == "reg128" and ref.CASE_BY_NAME["store-sched-a_neg_bound"]["route"] == "sched128"
    assert ref.CASE_BY_NAME["lse-sched-a_rows"]["route"] == "dma128" and ref.CASE_BY_NAME["lse-sched-a_rows_bound"]["route"] == "sched128"
    # batches with row maps and a device count on every route that takes batches
    for rt in ("reg64", "reg128", "sched128"):
        assert any(c["route"] == rt and c.get("batch") and c.get("a_rows") and c.get("c_rows") and c.get("m_dev") for c in ref.CASES), rt
    for rt in ("reg64", "reg128", "sched128", "dma128", "dma256"):
        assert any(c["route"] == rt and c.get("batch") and c.get("bias_mode") == 2 for c in ref.CASES), rt
        assert any(c["route"] == rt and c.get("batch") and (c.get("w_bcast") or rt == "dma256") for c in ref.CASES), rt


def test_shapes_are_off_the_tile():
    for c in ref.CASES:
        t = ref.ROUTE_TILE[c["route"]]
        if c["name"].startswith(("lse-reg128-N", "lse-dma128-N", "lse-astat-N")) or c["name"] == "store-reg64-M1N1":
            continue                                                   # the part-layout cases choose N on the part edges on purpose
        if c["name"] in ("store-skinny-N256",):
            continue
        assert c["M"] % t and c["N"] % t, c["name"]
