"""`--fp16`: precision 3 of the C ABI -- float16 GEMM operands (round-to-nearest-even), exact products, f32 accumulation; every
epilogue, every tensor in memory and everything that is not a GEMM of the two orchestrators stays f32.  GPU only.

Kernel level: against float64 on the PRE-ROUNDED operands (A.half(), W.half()), at the tolerance the f32 MFMA path itself has in
tests/test_kernels_gpu.py -- products of two float16 values are exact in float32, so only the accumulation order differs; a
round-toward-zero conversion misses that bound by three orders of magnitude, which pins the rounding mode.
Model level: against the reference's own ``model.half()`` run (tests/golden/hgt_fp16.npz, made by tests/golden/make_fp16.py):
ours may not be further from the reference's float64 run than the reference's half run is (RMS, no margin).

Measured on an MI355X (rms(ours fp16 - ref f64) / rms(ref half - ref f64) / max|ours f32 - ref f64|):
d32L1 1.75e-4 / 4.36e-4 / 4.3e-7, d128L3 3.56e-4 / 8.65e-4 / 9.9e-7, d256L2 1.71e-4 / 6.03e-4 / 1.1e-6, adaptive softmax
4.15e-4 / 4.09e-3 / 2.3e-6; the GEMM tests 7e-8 .. 1.3e-7 of sum|a||b| (bar 5e-7)."""
import dataclasses
import json
import logging

import numpy as np
import pytest
import torch

import fp16_inputs as fi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from gnnlm_amd import ops as _ops
    return _ops


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


# ------------------------------------------------------------------------------------------ 1. operand rounding, every kernel variant
@pytest.mark.parametrize("M,N,K", [(130, 257, 100), (512, 1024, 1024), (64, 20002, 64),
                                   (1000, 5000, 264),      # pre-converted image + LDS-DMA kernel, 128x128 tiles
                                   (4100, 8200, 272)])     # the same with 256x256 tiles
def test_gemm_fp16_rounding(ops, dev, M, N, K):
    """Shapes and input recipe of test_gemm_split_precisions (wide dynamic range along k, lda != K): the result is the float64
    product of the operands rounded to half by round-to-nearest-even, at the f32 MFMA path's own tolerance."""
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K + 4, generator=g)[:, :K] * torch.logspace(-2, 2, K)
    W = torch.randn(N, K, generator=g)
    Ah, Wh = A.half().double(), W.half().double()
    ref = Ah @ Wh.t()
    scale = Ah.abs() @ Wh.abs().t() + 1e-30
    out = ops.gemm_nt(A.to(dev), W.to(dev), precision="fp16").cpu().double()
    err = ((out - ref).abs() / scale).max().item()
    print(f"fp16 gemm {M}x{N}x{K}: max err / sum|a||b| = {err:.3e}")
    assert err < 5e-7, err
    assert not torch.equal(out, ops.gemm_nt(A.to(dev), W.to(dev)).cpu().double())      # not the f32 path


def test_gemm_fp16_overflow_is_inf(ops, dev):
    """Beyond +-65504 an operand becomes +-inf, as torch.Tensor.half() makes it (documented, not clamped)."""
    A = torch.zeros(64, 32)
    A[:, 0] = 1.0
    A[1, 0], A[2, 0], A[3, 0] = 70000.0, -70000.0, 65504.0
    W = torch.zeros(64, 32)
    W[:, 0] = 1.0
    out = ops.gemm_nt(A.to(dev), W.to(dev), precision="fp16").cpu()
    assert torch.equal(out, A.half().float() @ W.half().float().t())
    assert out[1, 0] == float("inf") and out[2, 0] == float("-inf") and out[3, 0] == 65504.0 and out[0, 0] == 1.0


# ------------------------------------------------------------------------------------------ 2. the full contract
@pytest.mark.parametrize("M,N,K", [(700, 300, 100),       # small tiles (64x64), k tail
                                   (2100, 2050, 288)])    # the pre-converted image kernel
def test_gemm_fp16_full_contract(ops, dev, M, N, K):
    """test_gemm_full_contract under fp16 against the pre-rounded float64 reference: row gather with zero rows, scattered store +
    residual through c_rows, gated per-column bias, alpha, device-side row count, untouched rows beyond it."""
    g = torch.Generator().manual_seed(M + N + K)
    n_src = M + 37
    A = torch.randn(n_src, K, generator=g)
    W = torch.randn(N, K, generator=g)
    a_rows = torch.randint(0, n_src, (M,), generator=g, dtype=torch.int32)
    a_rows[::11] = -1
    c_rows = torch.randperm(M + 5, generator=g)[:M].to(torch.int32)
    bias = torch.randn(N, generator=g)
    gate = (torch.rand(M, generator=g) < 0.7).float() * 1.5
    R = torch.randn(M + 5, N, generator=g)
    m = M - 77
    Ah, Wh = A.half().double(), W.half().double()
    prod = Ah[a_rows.clamp(min=0).long()] @ Wh.t()
    prod[a_rows < 0] = 0
    ref = torch.full((M + 5, N), 3.25, dtype=torch.float64)
    val = 0.75 * prod + gate.double()[:, None] * bias.double()[None, :] + R.double()[c_rows.long()]
    ref[c_rows[:m].long()] = val[:m]
    scale = torch.ones(M + 5, N, dtype=torch.float64)
    scale[c_rows.long()] = Ah.abs()[a_rows.clamp(min=0).long()] @ Wh.abs().t() + 1.0
    out = torch.full((M + 5, N), 3.25, device=dev)
    ops.gemm_nt(A.to(dev), W.to(dev), bias=bias.to(dev), gate=gate.to(dev), residual=R.to(dev), alpha=0.75, out=out,
                a_rows=a_rows.to(dev), c_rows=c_rows.to(dev), m_dev=torch.tensor([m], dtype=torch.int32, device=dev),
                precision="fp16")
    err = ((out.cpu().double() - ref).abs() / scale).max().item()
    print(f"fp16 full contract {M}x{N}x{K}: {err:.3e}")
    assert err < 5e-7, err
    untouched = torch.ones(M + 5, dtype=torch.bool)
    untouched[c_rows[:m].long()] = False
    assert torch.all(out.cpu()[untouched] == 3.25)


# ------------------------------------------------------------------------------------------ 3. the LSE epilogue
@pytest.mark.parametrize("M,N,K", [(2100, 20002, 256),    # 256x256 image tiles
                                   (1000, 5000, 288)])    # 128x128 image tiles
def test_gemm_fp16_lse(ops, dev, M, N, K):
    """test_gemm_lse_large under fp16 against the pre-rounded reference (tolerance of its f32 row): transposed accumulators,
    ragged last n-tile, device-side M."""
    g = torch.Generator().manual_seed(M + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    pick = torch.randint(0, N, (M,), generator=g, dtype=torch.int32)
    pick[:8] = torch.tensor([0, N - 1, N - 2, 63, 64, 127, 128, N - 65])
    logits = 0.05 * (A.half().double() @ W.half().double().t())
    m = M - 130
    lse, picked = ops.gemm_lse(A.to(dev), W.to(dev), pick.to(dev), alpha=0.05, precision="fp16",
                               m_dev=torch.tensor([m], dtype=torch.int32, device=dev))
    e1 = (lse.cpu().double()[:m] - torch.logsumexp(logits, 1)[:m]).abs().max().item()
    e2 = (picked.cpu().double()[:m] - logits.gather(1, pick.long()[:, None])[:m, 0]).abs().max().item()
    print(f"fp16 lse {M}x{N}x{K}: lse {e1:.3e} picked {e2:.3e}")
    assert e1 < 2e-5 and e2 < 2e-5


def test_gemm_precision_range(ops, dev):
    """3 is accepted, 4 and above refused as before."""
    from gnnlm_amd._lib import GnnlmError
    A = torch.randn(8, 8, device=dev)
    ops.gemm_nt(A, A, precision=3)
    with pytest.raises(GnnlmError):
        ops.gemm_nt(A, A, precision=4)


# ------------------------------------------------------------------------------------------ 4. against the reference's half
def _run_hgt(dev, name, precision, profile=False):
    from gnnlm_amd import _lib
    from gnnlm_amd.hgt import HGT, CodeStore, NeighborGraph
    c, x = fi.HGT_CASES[name], fi.hgt_inputs(name)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    store = CodeStore(codes=t(x["codes"]), centroids=t(x["cen"]), n_store=c["n_store"], vals=None, A=None, b=None)
    model = HGT(in_dim=c["d"], hidden_dim=c["d"], out_dim=c["d"], n_layers=c["L"], n_heads=c["H"])
    assert sorted((k, tuple(v.shape)) for k, v in model.state_dict().items()) == fi.hgt_param_shapes(c["d"], c["H"], c["L"])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in x["sd"].items()}, strict=True)
    model.gemm_precision = precision
    model.state_cache_gib = 0.0              # every group computed in this call (a second call would be served by the centre-state cache)
    G = NeighborGraph(ids=t(x["nb"]), n_blocks=1, T=c["T"], left=c["l"], right=c["r"], store=store)
    if profile:
        model(G, features={"tgt": t(x["tgt"])})                       # warm-up: one-time allocations
        torch.cuda.synchronize()
        _lib.profile_begin()
    out = model(G, features={"tgt": t(x["tgt"])})["tgt"]
    torch.cuda.synchronize()
    kernels = _lib.profile_end() if profile else None
    return out.cpu().numpy(), kernels


@pytest.mark.parametrize("name", list(fi.HGT_CASES))
def test_hgt_fp16_vs_reference_half(dev, golden, name):
    g = golden("hgt_fp16")
    assert np.array_equal(g[name + ".checksum"], fi.checksum(fi.hgt_inputs(name))), "the regenerated inputs are not the fixture's"
    ref64, ref_half = g[name + ".ref_f64"], g[name + ".ref_half"].astype(np.float64)
    f32, _ = _run_hgt(dev, name, 0)
    f16, kernels = _run_hgt(dev, name, 3, profile=(name == "d256L2"))
    e_ours, e_ref, e_f32 = rms(f16 - ref64), rms(ref_half - ref64), float(np.abs(f32 - ref64).max())
    print(f"{name}: rms(ours fp16 - f64) = {e_ours:.3e}, rms(reference half - f64) = {e_ref:.3e}, max|ours f32 - f64| = {e_f32:.3e}")
    assert e_f32 < 5e-5                                                # the yardstick is sound
    assert not np.array_equal(f16, f32)                                # the mode is really taken
    assert e_ours <= e_ref                                             # never narrower than the reference's own half run
    if kernels is not None:                                            # the inner layer's ntgt projections took the big-tile image path
        assert kernels.get("split_planes_kernel", {}).get("launches", 0) > 0, sorted(kernels)


def test_adaptive_softmax_fp16_vs_reference_half(dev, golden):
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    g, c, x = golden("hgt_fp16"), fi.ASM_CASE, fi.asm_inputs()
    assert np.array_equal(g["asm.checksum"], fi.checksum(x))
    tt = lambda a: None if a is None else torch.from_numpy(a)
    asm = AdaptiveSoftmax(list(c["cutoff"]) + [c["vocab"]], [tt(e) for e in x["emb"]], [tt(p) for p in x["proj"]],
                          tt(x["class_proj"]), dev)
    xd, td = torch.from_numpy(x["x"]).to(dev), torch.from_numpy(x["target"]).to(dev)
    f32 = asm.target_log_prob(xd, td).cpu().numpy()
    asm.gemm_precision = 3
    f16 = asm.target_log_prob(xd, td).cpu().numpy()
    ref64, ref_half = g["asm.ref_f64"], g["asm.ref_half"].astype(np.float64)
    e_ours, e_ref, e_f32 = rms(f16 - ref64), rms(ref_half - ref64), float(np.abs(f32 - ref64).max())
    print(f"asm: rms(ours fp16 - f64) = {e_ours:.3e}, rms(reference half - f64) = {e_ref:.3e}, max|ours f32 - f64| = {e_f32:.3e}")
    assert e_f32 < 5e-5
    assert not np.array_equal(f16, f32)
    assert e_ours <= e_ref


# ------------------------------------------------------------------------------------------ 5. graph capture
def _problem(n_layers=2, seed=3):
    from gnnlm_amd.synthetic import make_problem
    return make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=n_layers, k=32, seed=seed)


def test_fp16_step_is_graph_capturable(dev):
    """Shape of test_step_is_graph_capturable, L = 2, gemm_precision = 3: captured after an eager warm-up, replayed bit for bit."""
    from gnnlm_amd.synthetic import build_engine, to_batch
    prob = _problem()
    eng = build_engine(prob, dev)
    eng.precision = "fp16"
    assert eng.hgt.gemm_precision == 3 and eng.asm.gemm_precision == 3 and eng.precision == "fp16"
    batch = to_batch(prob["block"], dev)
    eager = {k: v.clone() for k, v in eng.score(batch, 0.25, 1.0).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = eng.score(batch, 0.25, 1.0)
    g.replay()
    torch.cuda.synchronize()
    for k in ("logp", "lm_logp", "gcn_feat"):
        assert torch.equal(out[k], eager[k]), k
    tgt0 = batch.targets.clone()
    batch.targets.copy_(torch.roll(tgt0, 1))
    g.replay()
    torch.cuda.synchronize()
    ref = eng.score(batch, 0.25, 1.0)
    assert torch.equal(out["logp"], ref["logp"]) and not torch.equal(out["logp"], eager["logp"])


# ------------------------------------------------------------------------------------------ 6. the cache never mixes precisions
def test_precision_never_mixes_in_the_state_cache(dev):
    from gnnlm_amd.synthetic import build_engine, to_batch
    prob = _problem(seed=5)
    batch = to_batch(prob["block"], dev)

    def engine(precision):
        e = build_engine(prob, dev)
        e.hgt.state_cache_gib, e.hgt.state_cache_slots, e.hgt.state_cache = 1.0, 4096, None
        e.precision = precision
        return e
    eng = engine("f32")
    runs = []
    for prec in ("f32", "fp16", "f32"):
        eng.precision = prec
        o = eng.score(batch, 0.25, 1.0)
        assert eng.hgt.state_cache is not None                          # the cached path is the one under test
        runs.append({k: o[k].clone() for k in ("gcn_feat", "lm_logp", "logp")})
    fresh = engine("fp16").score(batch, 0.25, 1.0)
    for k in ("gcn_feat", "lm_logp", "logp"):
        assert torch.equal(runs[0][k], runs[2][k]), k
        assert torch.equal(runs[1][k], fresh[k]), k
        assert not torch.equal(runs[0][k], runs[1][k]), k


# ------------------------------------------------------------------------------------------ 7. the driver
SENT_SIZES = [17, 1, 60, 5, 33, 1, 1, 48, 9, 26, 2, 41, 13, 1, 55, 30, 7, 22, 1, 38, 12, 19]


class _Recorder:
    """Wraps SequenceScorer.generate_finish: keeps every batch's inputs, the model's own outputs (features, LM log-probs) and the
    per-token scores of the hypotheses."""

    def __init__(self, monkeypatch):
        from gnnlm_amd.sequence_scorer import SequenceScorer
        self.batches = []
        inner = SequenceScorer.generate_finish
        rec = self

        def finish(scorer, h):
            lm = h["probs"].clone()
            hypos = inner(scorer, h)
            graph = h["sample"]["net_input"]["graph"]
            rec.batches.append(dict(
                graph=dataclasses.replace(graph, ids=graph.ids.clone(), tgt_h=graph.tgt_h.clone()), target=h["sample"]["target"].clone(),
                lm=lm, feat=h["decoder_out"][0].clone(), queries=None if h["queries"] is None else h["queries"].clone(),
                knn_model=h["knn_model"] if h["use_knn"] else None, lmbda=h["lmbda"], temperature=h["temperature"],
                blockwise=bool(h["sample"].get("blockwise_knn")),
                scores=torch.cat([hy[0]["positional_scores"].float().reshape(-1) for hy in hypos]).clone(),
                starts=[int(v) for v in h["sample"].get("start_indices", [])]))
            return hypos
        monkeypatch.setattr(SequenceScorer, "generate_finish", finish)

    def take(self):
        out, self.batches = self.batches, []
        return out


@pytest.mark.parametrize("mode", ["knnlm", "eos"])
def test_eval_lm_fp16(dev, tmp_path, monkeypatch, caplog, mode):
    """`eval_lm --fp16` on the tiny data directory of the driver tests: the log line, "precision" in --result-json, per-token scores
    bit-equal to GnnLmEngine.score with the precision set programmatically on the same batches (the LM term and the features; with
    --knnlm the engine's two outputs go through the run's own interpolation) and different from the f32 run's; without the flag the
    output is the f32 engine's."""
    from test_ragged_gpu import make_ragged_dir
    from gnnlm_amd import eval_lm
    from gnnlm_amd.engine import BlockBatch, GnnLmEngine
    from gnnlm_amd.model import GnnLmModel
    c = make_ragged_dir(tmp_path, SENT_SIZES, L=2)
    args = c["base"] + ["--tokens-per-sample", "64", "--max-tokens", "128"]
    if mode == "knnlm":
        args += ["--knnlm", "--k", "8", "--lmbda", "0.25", "--dstore-dir", str(c["data"] / "train_dstore"),
                 "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]
    else:
        args += ["--sample-break-mode", "eos"]
    rec = _Recorder(monkeypatch)
    runs = {}
    for prec, flag in (("f32", []), ("fp16", ["--fp16"])):
        out = str(tmp_path / f"res_{prec}.json")
        with caplog.at_level(logging.INFO):
            caplog.clear()
            res = eval_lm.cli_main(args + flag + ["--result-json", out])
        said = any("--fp16: float16 matrix-core GEMMs with float32 accumulation" in r.getMessage() for r in caplog.records)
        assert said == (prec == "fp16")
        assert not any("ignored" in r.getMessage() for r in caplog.records)
        assert json.load(open(out))["precision"] == prec and res["precision"] == prec
        runs[prec] = rec.take()
        assert len(runs[prec]) >= 2
    for prec in ("f32", "fp16"):
        model, _ = GnnLmModel.from_checkpoint(str(tmp_path / "ckpt.pt"), dev, vocab_size=600)
        for b in runs[prec]:
            G = b["graph"]
            eng = GnnLmEngine(model.hgt_decoder, model.adaptive_softmax, G.store, G.left, G.right, G.max_intra_context, precision=prec)
            assert eng.precision == prec
            batch = BlockBatch(ids=G.ids, tgt_feats=G.tgt_h, targets=b["target"].reshape(-1), n_blocks=G.n_blocks, T=G.T, block_off=G.block_off)
            o = eng.score(batch)
            assert torch.equal(o["gcn_feat"].reshape(-1), b["feat"].reshape(-1))
            assert torch.equal(o["lm_logp"].reshape(-1), b["lm"].reshape(-1))
            if b["knn_model"] is None:
                scores = o["lm_logp"].view(b["target"].shape)
            else:                                              # the run's own kNN term on the engine's outputs (sequence_scorer.py)
                bsz, tsz = b["target"].shape
                q = o["gcn_feat"].view(bsz, tsz, -1).transpose(0, 1).contiguous()
                tq = (b["target"].transpose(0, 1) if b["blockwise"] else b["target"]).reshape(-1)
                lm_flat = o["lm_logp"].view(bsz, tsz).transpose(0, 1).reshape(-1)
                km = b["knn_model"]
                mixed, _, _ = km.interpolate_finish(km.interpolate_begin(q.view(tsz * bsz, -1)), tq.clamp(min=0), lm_flat, b["temperature"], b["lmbda"])
                scores = mixed.view(tsz, bsz).transpose(0, 1)
            if G.block_off is None:
                s0 = b["starts"][0] if b["starts"] else 0
                assert len(set(b["starts"])) <= 1
                mine = scores[:, s0:].reshape(-1)
            else:
                mine = scores.reshape(-1)
            assert mine.numel() == b["scores"].numel() and torch.equal(mine.float(), b["scores"])
    a = torch.cat([b["scores"] for b in runs["f32"]])
    h = torch.cat([b["scores"] for b in runs["fp16"]])
    assert a.shape == h.shape and not torch.equal(a, h)
