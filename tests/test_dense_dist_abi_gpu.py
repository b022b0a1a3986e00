"""The dense next-token entry points at the call level (include/gnnlm.h: gnnlm_adaptive_log_probs, gnnlm_dense_log_probs,
gnnlm_knn_mix_dense, gnnlm_row_rank; gnnlm_topk_merge with ncols = V): descriptors filled by hand, outputs between guard bands
holding a NaN-payload sentinel, the float64 restatement and the inputs of tests/dense_dist_ref.py (test_dense_dist_ref_cpu.py
pins both without a GPU).  GPU only.

Bars: every log-prob within 2e-5 of the restatement (the project's bar for log-probs); out[r, t] of the mix within 4e-5 of
gnnlm_knn_interp for target t (each side gets the bar once); out_pknn against the reference's own dense fixtures at the
rtol 1e-3 / atol 2e-5 of test_mirrors_gpu.py; rank and top-N bit for bit; the fp16 case at the bar of test_fp16_gpu.py's head test
(no further from the reference's float64 run than the reference's own half run, RMS)."""
import ctypes

import numpy as np
import pytest
import torch

import dense_dist_ref as R
import fp16_inputs as fi
import gemm_ref
from test_gemm_abi_gpu import GUARD, Out, bits, dev_in

pytestmark = pytest.mark.gpu
E_INVALID = -22
BAR = 2e-5
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def L():
    from gnnlm_amd import _lib
    return _lib.lib()


def stream():
    from gnnlm_amd import _lib
    return _lib.stream()


class Keep:
    def __init__(self, dev):
        self.dev, self.t = dev, []

    def put(self, a, off=0):
        t, p = dev_in(np.ascontiguousarray(a).reshape(-1), self.dev, off)
        self.t.append(t)
        return p


def pad4(a):
    return np.pad(a, ((0, 0), (0, (-a.shape[1]) % 4)))


def adaptive_desc(w, keep, precision=0):
    """gnnlm_adaptive_softmax_t of oracle-style weights: head_w = [emb_0; class_proj], proj_t[b] = proj[b]^T, tail dims padded to 4"""
    from gnnlm_amd import _lib
    d = _lib.gnnlm_adaptive_softmax_t()
    d.d, d.n_bands, d.gemm_precision = w["emb"][0].shape[1], len(w["cutoff"]), precision
    for i, c in enumerate(w["cutoff"]):
        d.cutoff[i] = int(c)
    d.head_w = keep.put(np.concatenate([w["emb"][0], w["class_proj"]], 0).astype(np.float32))
    for b in range(1, len(w["cutoff"])):
        d.proj_t[b] = keep.put(np.ascontiguousarray(pad4(w["proj"][b]).T))
        d.emb[b] = keep.put(pad4(w["emb"][b]))
        d.dim[b] = pad4(w["emb"][b]).shape[1]
    return d


def plain_desc(weight, bias, keep, precision=0):
    from gnnlm_amd import _lib
    d = _lib.gnnlm_dense_softmax_t()
    d.vocab, d.d = weight.shape
    d.gemm_precision, d.w, d.ldw = precision, keep.put(weight), weight.shape[1]
    if bias is not None:
        d.bias = keep.put(bias)
    return d


def head_call(entry, desc, x_ptr, ldx, n, out_ptr, ldo, ws_ptr, ws_bytes):
    return getattr(L(), "gnnlm_" + entry)(ctypes.byref(desc) if desc is not None else None, vp(x_ptr), ldx, n, vp(out_ptr), ldo, vp(ws_ptr), ws_bytes, stream())


def run_head(entry, desc, x, V, dev, keep, least=False, pad=5):
    """One call with ldx = d + 4 (NaN pad), ldo = V + pad, out one float off a 16-byte boundary, the workspace exactly as large as
    the library asks -> [n, V]; the pad columns and every guard band must come back untouched."""
    n, d = x.shape
    panel = np.full((n + 3, d + 4), np.nan, dtype=np.float32)
    panel[:n, :d] = x
    xp = keep.put(panel)
    ldo = V + pad
    size = getattr(L(), f"gnnlm_{entry}_workspace_bytes" + ("_min" if least else ""))
    size.restype = ctypes.c_size_t
    ws_bytes = int(size(ctypes.byref(desc), n))
    assert ws_bytes > 0 and ws_bytes % 4 == 0
    out, ws = Out(gemm_ref.sentinel(n * ldo), dev, 1), Out(gemm_ref.sentinel(ws_bytes // 4), dev, 0)
    assert out.ptr % 16 == 4 and ws.ptr % 16 == 0 and xp % 16 == 0
    rc = head_call(entry, desc, xp, d + 4, n, out.ptr, ldo, ws.ptr, ws_bytes)
    assert rc == 0, L().gnnlm_last_error()
    torch.cuda.synchronize()
    ws.read()
    got = out.read().reshape(n, ldo)
    assert (bits(got[:, V:]) == gemm_ref.SENT_BITS).all(), "a pad column of ldo > V was written"
    assert not (bits(got[:, :V]) == gemm_ref.SENT_BITS).any(), "a column below V was not written"
    return got[:, :V]


def worst(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max())


# ---------------------------------------------------------------------------------------------------- heads
def test_adaptive_golden_shape(dev, golden):
    """V = 24, d = 16, tail dims 4 and 1 (padded to 4): the reference's own dense tensor."""
    g = golden("adaptive_softmax")
    w = {"cutoff": [int(c) for c in g["cutoff"]], "emb": [g[f"emb{i}"] for i in range(3)], "proj": [None, g["proj1"], g["proj2"]],
         "class_proj": g["class_proj"]}
    keep = Keep(dev)
    x = g["x"].reshape(-1, 16)
    got = run_head("adaptive_log_probs", adaptive_desc(w, keep), x, 24, dev, keep)
    ref = g["dense"].reshape(-1, 24)
    print(f"golden: max |d| = {worst(got, ref):.2e}")
    assert worst(got, ref) < BAR
    assert worst(got, R.adaptive_log_probs(x, w)) < BAR


@pytest.mark.parametrize("n", R.HEAD_ROWS)
@pytest.mark.parametrize("kind", ["adaptive", "plain", "plain-bias"])
def test_heads(dev, kind, n):
    """cutoffs [100, 300, 603] with dims 64 / 16 / 4 and a plain head of V = 205: ldo = V + 5 with the sentinel in the pad, two
    identical calls -> identical bits, every entry within 2e-5."""
    x, w, pw, pb = R.head_inputs(n)
    keep = Keep(dev)
    if kind == "adaptive":
        entry, desc, V, ref = "adaptive_log_probs", adaptive_desc(w, keep), R.HEAD_CUTOFF[-1], R.adaptive_log_probs(x, w)
    else:
        bias = pb if kind == "plain-bias" else None
        entry, desc, V, ref = "dense_log_probs", plain_desc(pw, bias, keep), R.PLAIN_V, R.plain_log_probs(x, pw, bias)
    got = run_head(entry, desc, x, V, dev, keep)
    again = run_head(entry, desc, x, V, dev, keep)
    assert np.array_equal(bits(got), bits(again)), "two identical calls differ"
    print(f"{kind} n={n}: max |d| = {worst(got, ref):.2e}")
    assert worst(got, ref) < BAR
    np.testing.assert_allclose(np.exp(got.astype(np.float64)).sum(1), 1.0, atol=1e-4)


@pytest.mark.parametrize("kind", ["adaptive", "plain-bias"])
def test_chunk_boundary_at_the_minimum_workspace(dev, kind):
    """n = 130 with the least workspace the call accepts: chunks of 128 and 2 rows."""
    n = 130
    x, w, pw, pb = R.head_inputs(n)
    keep = Keep(dev)
    if kind == "adaptive":
        entry, desc, V, ref = "adaptive_log_probs", adaptive_desc(w, keep), R.HEAD_CUTOFF[-1], R.adaptive_log_probs(x, w)
    else:
        entry, desc, V, ref = "dense_log_probs", plain_desc(pw, pb, keep), R.PLAIN_V, R.plain_log_probs(x, pw, pb)
    full = int(getattr(L(), f"gnnlm_{entry}_workspace_bytes")(ctypes.byref(desc), n))
    least = int(getattr(L(), f"gnnlm_{entry}_workspace_bytes_min")(ctypes.byref(desc), n))
    assert 0 < least < full
    got = run_head(entry, desc, x, V, dev, keep, least=True)
    print(f"{kind} min workspace ({least} of {full} bytes): max |d| = {worst(got, ref):.2e}")
    assert worst(got, ref) < BAR


def test_offsets_beyond_2_to_31(dev):
    """V = 267744, d = 16, n = 8192: 8.8 GB of output, rows 8021 .. 8191 start beyond 2^31 elements.  Rows 0, n - 1 and the two
    rows either side of the 2^31 boundary are held to the restatement; every row's first and last band column was written."""
    c = R.BIG
    n, V, d = c["n"], c["cutoff"][-1], c["d"]
    w = R.adaptive_weights(c["cutoff"], c["dims"], d, seed=21)
    x = (1.5 * np.random.RandomState(22).randn(n, d)).astype(np.float32)
    keep = Keep(dev)
    desc = adaptive_desc(w, keep)
    xt = torch.from_numpy(x).to(dev)
    out = torch.full((n, V), float("nan"), device=dev, dtype=torch.float32)
    ws_bytes = int(L().gnnlm_adaptive_log_probs_workspace_bytes(ctypes.byref(desc), n))
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
    assert n * V > 2 ** 31
    rc = head_call("adaptive_log_probs", desc, xt.data_ptr(), d, n, out.data_ptr(), V, ws.data_ptr(), ws_bytes)
    assert rc == 0, L().gnnlm_last_error()
    torch.cuda.synchronize()
    edge = 2 ** 31 // V
    rows = [0, edge, edge + 1, n - 1]
    got = out[rows].cpu().numpy()
    ref = R.adaptive_log_probs(x[rows], w)
    print(f"big: max |d| over rows {rows} = {worst(got, ref):.2e}")
    assert worst(got, ref) < BAR
    cols = torch.tensor([0, c["cutoff"][0] - 1, c["cutoff"][0], c["cutoff"][1], V - 1], device=dev)
    assert bool(torch.isfinite(out[:, cols]).all()), "a row was not finished"
    assert bool(torch.isfinite(out[edge - 1:edge + 2]).all())


def test_head_fp16_operands(dev, golden):
    """gemm_precision 3 on the inputs of tests/fp16_inputs.py at the bar of test_fp16_gpu.py's head test: the target column of the
    dense result is no further (RMS) from the reference's float64 run than the reference's own model.half() run, and the f32 call
    is within 5e-5 of it; the dense rows stay normalised."""
    g, c, inp = golden("hgt_fp16"), fi.ASM_CASE, fi.asm_inputs()
    assert np.array_equal(g["asm.checksum"], fi.checksum(inp))
    w = {"cutoff": list(c["cutoff"]) + [c["vocab"]], "emb": inp["emb"], "proj": inp["proj"], "class_proj": inp["class_proj"]}
    keep = Keep(dev)
    rows = np.arange(c["n"])
    f32 = run_head("adaptive_log_probs", adaptive_desc(w, keep, 0), inp["x"], c["vocab"], dev, keep)
    f16 = run_head("adaptive_log_probs", adaptive_desc(w, keep, 3), inp["x"], c["vocab"], dev, keep)
    rms = lambda v: float(np.sqrt(np.mean(np.square(np.asarray(v, dtype=np.float64)))))
    ref64, ref_half = g["asm.ref_f64"], g["asm.ref_half"].astype(np.float64)
    e_ours, e_ref = rms(f16[rows, inp["target"]] - ref64), rms(ref_half - ref64)
    e_f32 = float(np.abs(f32[rows, inp["target"]] - ref64).max())
    print(f"fp16 head: rms(ours fp16 - f64) = {e_ours:.3e}, rms(reference half - f64) = {e_ref:.3e}, max|ours f32 - f64| = {e_f32:.3e}")
    assert e_f32 < 5e-5
    assert not np.array_equal(f16, f32)
    assert e_ours <= e_ref
    assert worst(f32, R.adaptive_log_probs(inp["x"], w)) < BAR
    np.testing.assert_allclose(np.exp(f16.astype(np.float64)).sum(1), 1.0, atol=1e-4)


# ---------------------------------------------------------------------------------------------------- mix
def mix_desc(case, keep, temperature, lmbda, source, ld_pad, off):
    """-> (descriptor without outputs, ld): labels through ``vals`` (int32 / int16 table) or ``knn_vals``"""
    from gnnlm_amd import _lib
    n, V, k = case["lm_logp"].shape[0], case["V"], case["k"]
    d = _lib.gnnlm_knn_mix_dense_t()
    ld = V + ld_pad
    lm = np.full((n, ld), np.nan, dtype=np.float32)
    lm[:, :V] = case["lm_logp"]
    d.lm_logp, d.ld_lm = keep.put(lm, off), ld
    d.sims, d.ids = keep.put(case["sims"]), keep.put(case["ids"])
    if source == "knn_vals":
        d.knn_vals = keep.put(case["labels"].astype(np.int32))
    else:
        vals = case["vals"].astype(np.int16 if source == "vals16" else np.int32)
        d.vals, d.vals_itemsize = keep.put(vals), vals.itemsize
        d.n_store, d.row0, d.n_local = case["n_store"], 0, len(vals)
    d.n, d.k, d.V, d.temperature, d.lmbda = n, k, V, temperature, lmbda
    return d, ld


def run_mix(case, dev, temperature, lmbda, source="vals", ld_pad=5, off=1, want_pknn=True):
    keep = Keep(dev)
    d, ld = mix_desc(case, keep, temperature, lmbda, source, ld_pad, off)
    n, V = case["lm_logp"].shape[0], case["V"]
    out, pk = Out(gemm_ref.sentinel(n * ld), dev, off), Out(gemm_ref.sentinel(n * ld), dev, off)
    d.out, d.ldo = out.ptr, ld
    if want_pknn:
        d.out_pknn, d.ld_pknn = pk.ptr, ld
    rc = L().gnnlm_knn_mix_dense(ctypes.byref(d), stream())
    assert rc == 0, L().gnnlm_last_error()
    torch.cuda.synchronize()
    got, gpk = out.read().reshape(n, ld), pk.read().reshape(n, ld)
    assert (bits(got[:, V:]) == gemm_ref.SENT_BITS).all() and (bits(gpk[:, V:]) == gemm_ref.SENT_BITS).all(), "a pad column was written"
    assert not (bits(got[:, :V]) == gemm_ref.SENT_BITS).any()
    assert want_pknn or (bits(gpk) == gemm_ref.SENT_BITS).all()
    return got[:, :V], gpk[:, :V]


def interp_targets(case, dev, temperature, lmbda, targets):
    """gnnlm_knn_interp for ``targets`` [n, m]: every row repeated m times with the language model's own column of each target"""
    from gnnlm_amd import ops
    n, m = targets.shape
    rep = lambda a: torch.from_numpy(np.repeat(a, m, axis=0)).to(dev)
    lm = np.take_along_axis(case["lm_logp"], targets, axis=1).reshape(-1)
    out, _, _ = ops.knn_interp(torch.from_numpy(lm).to(dev), rep(case["sims"]), rep(case["ids"]), torch.from_numpy(targets.reshape(-1)).to(dev),
                               temperature, lmbda, vals=torch.from_numpy(case["vals"]).to(dev), n_store=case["n_store"], vals_tag=False)
    return out.cpu().numpy().reshape(n, m)


MIX_CASES = [(k, t, l, p) for k in R.MIX_KS for t in R.MIX_TS for l in R.MIX_LMBDAS for p in R.MIX_PATTERNS]


@pytest.mark.parametrize("k,t,lmbda,pattern", MIX_CASES)
def test_mix(dev, k, t, lmbda, pattern):
    i = MIX_CASES.index((k, t, lmbda, pattern))
    case = R.mix_case(k, pattern, seed=100 * k + i % 4)
    source = ("vals", "knn_vals")[(i // 4) % 2]
    aligned = (i // 8) % 2 == 0                     # 16-byte path (ld % 4 == 0, aligned bases) or the scalar one
    kw = dict(source=source, ld_pad=4 if aligned else 5, off=0 if aligned else 1)
    got, gpk = run_mix(case, dev, t, lmbda, **kw)
    again, _ = run_mix(case, dev, t, lmbda, **kw)
    assert np.array_equal(bits(got), bits(again)), "two identical calls differ"
    p_ref, ref = R.mix_expected(case, t, lmbda)
    e, ep = worst(got, ref), worst(gpk, p_ref)
    # out[r, t] against the target-column kernel: 50 random targets per row (every label of the row's neighbours among them first)
    rs = np.random.RandomState(i)
    tg = rs.randint(0, case["V"], size=(got.shape[0], 50)).astype(np.int64)
    lab = np.where((case["labels"] >= 0) & (case["labels"] < case["V"]), case["labels"], 0)
    tg[:, :min(25, k)] = lab[:, :min(25, k)]
    ei = float(np.abs(np.take_along_axis(got, tg, 1).astype(np.float64) - interp_targets(case, dev, t, lmbda, tg)).max())
    print(f"k={k} t={t} lmbda={lmbda} {pattern} {source} {'vec' if aligned else 'scalar'}: |out - f64| {e:.2e}, |p_knn - f64| {ep:.2e}, "
          f"|out[t] - knn_interp| {ei:.2e}")
    assert e < BAR
    assert ep < 2e-6                                # a probability: a few float32 roundings of values <= 1
    assert ei < 4e-5
    assert (gpk[p_ref == 0] == 0).all(), "p_knn is zero where no neighbour has the label"
    if pattern == "outside":
        assert (gpk[1] == 0).all()                  # every label of row 1 lies outside [0, V): nothing but the no-neighbour term


def test_mix_label_sources_agree(dev):
    case = R.mix_case(100, "padded", seed=7)
    a, pa = run_mix(case, dev, 0.01, 0.25, source="vals")
    b, pb = run_mix(case, dev, 0.01, 0.25, source="knn_vals")
    c, pc = run_mix(case, dev, 0.01, 0.25, source="vals16")
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(pa), bits(pb))
    assert np.array_equal(bits(a), bits(c)) and np.array_equal(bits(pa), bits(pc))
    d, _ = run_mix(case, dev, 0.01, 0.25, source="vals", want_pknn=False)
    assert np.array_equal(bits(a), bits(d))


@pytest.mark.parametrize("metric_type", ["do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2"])
def test_mix_pknn_against_the_reference_dense(dev, golden, metric_type):
    """out_pknn against ``KNNModel.get_knn_prob(targets=None)`` of the reference, the sixteen dense fixtures of knn.npz."""
    g = golden("knn")
    for cos in ("raw", "cos"):
        for t in (1.0, 0.01):
            tag = f"{metric_type}.{cos}.t{t}"
            ids = g[tag + ".ids"]
            case = dict(sims=g[tag + ".sims"], ids=ids, vals=g["vals"].astype(np.int16), labels=R.neighbour_labels(ids, g["vals"]),
                        lm_logp=np.full((ids.shape[0], 50), np.log(1 / 50), dtype=np.float32), V=50, n_store=len(g["vals"]), k=ids.shape[1])
            _, gpk = run_mix(case, dev, t, 0.25, source="vals16")
            np.testing.assert_allclose(gpk, g[tag + ".dense"], rtol=1e-3, atol=2e-5)


# ---------------------------------------------------------------------------------------------------- rank and top-N
def test_rank_and_topn_bit_for_bit(dev):
    from gnnlm_amd import _lib
    v, t = R.rank_case()
    n, V = v.shape
    ld = V + 3
    keep = Keep(dev)
    panel = np.full((n, ld), np.inf, dtype=np.float32)          # pad columns that would win if they were read
    panel[:, :V] = v
    vptr, tptr = keep.put(panel), keep.put(t)
    rank = Out(np.full(n, -77, dtype=np.int32), dev, 1)
    rc = L().gnnlm_row_rank(vp(vptr), ld, n, V, vp(tptr), vp(rank.ptr), stream())
    assert rc == 0, L().gnnlm_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(rank.read(), R.rank(v, t))
    for N in (1, 8, 300):
        bv, bi = Out(gemm_ref.sentinel(n * N), dev, 0), Out(np.full(n * N, -5, dtype=np.int64), dev, 0)
        d = _lib.gnnlm_topk_t()
        d.scores, d.ld, d.n, d.ncols, d.k, d.largest, d.init = vptr, ld, n, V, N, 1, 1
        d.best_val, d.best_id = bv.ptr, bi.ptr
        _lib.call_desc("gnnlm_topk_merge", d)
        torch.cuda.synchronize()
        ids, vals = R.topn(v, N)
        assert np.array_equal(bi.read().reshape(n, N), ids)
        assert np.array_equal(bits(bv.read().reshape(n, N) + np.float32(0)), bits(vals))
        # the rank is the target's position in that list
        rk = R.rank(v, t)
        for r in range(n):
            if 0 <= rk[r] < N and R.present(v[r, t[r]]):
                assert ids[r, rk[r]] == t[r]


# ---------------------------------------------------------------------------------------------------- refusals, n = 0
def test_head_refusals_leave_out_untouched(dev):
    x, w, pw, pb = R.head_inputs(33)
    n, d = x.shape
    keep = Keep(dev)
    xp = keep.put(x)
    for entry, desc, V in (("adaptive_log_probs", adaptive_desc(w, keep), R.HEAD_CUTOFF[-1]), ("dense_log_probs", plain_desc(pw, pb, keep), R.PLAIN_V)):
        ws_bytes = int(getattr(L(), f"gnnlm_{entry}_workspace_bytes")(ctypes.byref(desc), n))
        least = int(getattr(L(), f"gnnlm_{entry}_workspace_bytes_min")(ctypes.byref(desc), n))
        out, ws = Out(gemm_ref.sentinel(n * (V + 5)), dev, 0), Out(gemm_ref.sentinel(ws_bytes // 4), dev, 0)
        good = dict(x=xp, ldx=d, n=n, out=out.ptr, ldo=V + 5, ws=ws.ptr, ws_bytes=ws_bytes)
        bad = [dict(x=None), dict(out=None), dict(ws=None), dict(x=xp + 4), dict(out=out.ptr + 2), dict(ws=ws.ptr + 4, ws_bytes=ws_bytes - 4),
               dict(ldo=V - 1), dict(ldx=d - 4), dict(ldx=d + 1), dict(ws_bytes=least - 256), dict(ws_bytes=0), dict(n=-1)]
        for kw in bad:
            a = dict(good, **kw)
            rc = head_call(entry, desc, a["x"], a["ldx"], a["n"], a["out"], a["ldo"], a["ws"], a["ws_bytes"])
            assert rc == E_INVALID, (entry, kw, rc)
        assert head_call(entry, None, xp, d, n, out.ptr, V + 5, ws.ptr, ws_bytes) == E_INVALID
        assert head_call(entry, desc, xp, d, 0, out.ptr, V + 5, None, 0) == 0             # n = 0: accepted, nothing touched
        torch.cuda.synchronize()
        assert (bits(out.read()) == gemm_ref.SENT_BITS).all() and (bits(ws.read()) == gemm_ref.SENT_BITS).all()
    bad_w = adaptive_desc(w, keep)
    bad_w.cutoff[1] = bad_w.cutoff[0]
    out = Out(gemm_ref.sentinel(n * 700), dev, 0)
    assert head_call("adaptive_log_probs", bad_w, xp, d, n, out.ptr, 700, xp, 1 << 20) == E_INVALID
    bad_p = plain_desc(pw, pb, keep, precision=4)
    assert head_call("dense_log_probs", bad_p, xp, d, n, out.ptr, 700, xp, 1 << 20) == E_INVALID
    torch.cuda.synchronize()
    assert (bits(out.read()) == gemm_ref.SENT_BITS).all()


def test_mix_and_rank_refusals_leave_out_untouched(dev):
    case = R.mix_case(8, "padded", seed=3)
    keep = Keep(dev)
    n, V = case["lm_logp"].shape[0], case["V"]
    out, pk = Out(gemm_ref.sentinel(n * (V + 4)), dev, 0), Out(gemm_ref.sentinel(n * (V + 4)), dev, 0)

    def desc(**kw):
        d, ld = mix_desc(case, keep, 1.0, 0.25, kw.pop("source", "vals"), 4, 0)
        d.out, d.ldo, d.out_pknn, d.ld_pknn = out.ptr, ld, pk.ptr, ld
        for f, v in kw.items():
            setattr(d, f, v(d) if callable(v) else v)
        return d

    good = desc()
    bad = [dict(lm_logp=None), dict(sims=None), dict(ids=None), dict(out=None), dict(vals=None), dict(k=0), dict(k=1025), dict(k=-1),
           dict(lmbda=0.0), dict(lmbda=1.0), dict(lmbda=-0.1), dict(lmbda=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
           dict(ldo=V - 1), dict(ld_lm=V - 1), dict(ld_pknn=V - 1), dict(V=0), dict(n=-1), dict(vals_itemsize=8), dict(n_store=0),
           dict(out=out.ptr + 2), dict(lm_logp=good.lm_logp + 1), dict(ids=good.ids + 4), dict(out=lambda d: d.lm_logp), dict(out_pknn=lambda d: d.out)]
    for kw in bad:
        rc = L().gnnlm_knn_mix_dense(ctypes.byref(desc(**kw)), stream())
        assert rc == E_INVALID, (kw, rc)
    assert L().gnnlm_knn_mix_dense(None, stream()) == E_INVALID
    assert L().gnnlm_knn_mix_dense(ctypes.byref(desc(n=0)), stream()) == 0
    v, t = R.rank_case()
    vptr, tptr = keep.put(v), keep.put(t)
    rank = Out(np.full(v.shape[0], -77, dtype=np.int32), dev, 0)
    rr = lambda a, ld, n_, V_, b, c: L().gnnlm_row_rank(vp(a), ld, n_, V_, vp(b), vp(c), stream())
    for args in ((None, v.shape[1], 9, v.shape[1], tptr, rank.ptr), (vptr, v.shape[1], 9, v.shape[1], None, rank.ptr),
                 (vptr, v.shape[1], 9, v.shape[1], tptr, None), (vptr, v.shape[1] - 1, 9, v.shape[1], tptr, rank.ptr),
                 (vptr, v.shape[1], 9, 0, tptr, rank.ptr), (vptr, v.shape[1], -1, v.shape[1], tptr, rank.ptr),
                 (vptr + 2, v.shape[1], 9, v.shape[1], tptr, rank.ptr)):
        assert rr(*args) == E_INVALID, args
    assert rr(vptr, v.shape[1], 0, v.shape[1], tptr, rank.ptr) == 0
    torch.cuda.synchronize()
    assert (bits(out.read()) == gemm_ref.SENT_BITS).all() and (bits(pk.read()) == gemm_ref.SENT_BITS).all()
    assert (rank.read() == -77).all()
    assert GUARD > 0
