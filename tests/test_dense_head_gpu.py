"""The plain (non-adaptive) output layer on the GPU (csrc/dense_logp.hip, gnnlm_amd/dense_softmax.py): the head of a
``--arch transformer_lm`` checkpoint (enwik8), transformer.py:843-852,1081-1085.  GPU only.

Every comparison is against the float64 restatement of tests/dense_head_ref.py at 2e-5, the project's tolerance for
log-probabilities against float64 (README "Parity").  Under gemm_precision 3 the restatement runs on the PRE-ROUNDED operands
(x.half(), w.half()) with the bias unrounded, as tests/test_fp16_gpu.py does: products of two float16 values are exact in float32,
so only the accumulation order differs.

Shapes are the smallest at which the one-launch kernel can go wrong: V on both sides of every 32-column accumulator tile and
128-column template step (TN = ceil(V / 128)), d with a partial k-tile (4, 132) and many k-tiles (1024), n with a partial and more
than one 32-row workgroup, and the two row counts from which a workgroup owns 64 and 128 rows.  Inputs: x ~ N(0, 1), w ~ N(0, 1) * 2 / sqrt(d) (logits with a standard deviation of 2), bias ~ N(0, 1).
Budget at d = 1024: an f32 fmaf chain is within ~1.5e-7 * sum|x w| = 1.5e-7 * 1024 * 0.64 * 2 / 32 = 6e-6 of float64, the target's
logit and the row maximum each carry it: 1.2e-5 < 2e-5.
"""
import ctypes
import json
import logging
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

import dense_head_ref as ref

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def boundary_targets(rs, V, n, bad=True):
    """Random targets with column 0, column V - 1 and both sides of every 32- and 128-column boundary in the first rows; with
    `bad` (n >= 8) one target of -1 and one of V."""
    t = rs.randint(0, V, size=n).astype(np.int64)
    edge = sorted({0, V - 1} | {c for b in range(32, V, 32) for c in (b - 1, b)})
    m = min(len(edge), n)
    t[:m] = edge[:m] if n >= len(edge) else rs.choice(edge, size=m, replace=False)
    bad_rows = []
    if bad and n >= 8:
        bad_rows = [n - 2, n - 5]
        t[n - 2], t[n - 5] = -1, V
    return t, bad_rows


def make_inputs(seed, V, d, n, with_bias, pad=0):
    rs = np.random.RandomState(seed)
    x = rs.randn(n, d + pad).astype(np.float32)
    w = (rs.randn(V, d + pad) * (2.0 / math.sqrt(d))).astype(np.float32)
    b = rs.randn(V).astype(np.float32) if with_bias else None
    return rs, x, w, b


def build(dev, w, b, d, route, precision):
    """DenseSoftmax over w[:, :d] (a view when w has padding columns: ldw > d)."""
    from gnnlm_amd.dense_softmax import DenseSoftmax
    wd = torch.from_numpy(w).to(dev)
    ds = DenseSoftmax(wd[:, :d].contiguous(), None if b is None else torch.from_numpy(b), dev)
    if w.shape[1] != d:                     # keep the padded rows: the descriptor reads [V, d] with row stride ldw = d + pad
        ds.weight = wd
        ds._w.w, ds._w.ldw = wd.data_ptr(), wd.stride(0)
    ds.route, ds.gemm_precision = route, precision
    return ds


def reference(x, w, b, t, d, precision):
    xs, ws = x[:, :d], w[:, :d]
    if precision == 3:
        xs, ws = ref.half_round(xs), ref.half_round(ws)
    return ref.dense_logp64(xs, ws, b, t)


def check(got, want, bad_rows, what):
    got = got.astype(np.float64)
    ok = np.ones(len(want), bool)
    ok[bad_rows] = False
    assert np.isfinite(got[ok]).all() and np.isfinite(want[ok]).all(), what
    err = float(np.abs(got[ok] - want[ok]).max()) if ok.any() else 0.0
    print(f"{what}: max |ours - float64| = {err:.2e} over {int(ok.sum())} rows")
    for r in bad_rows:
        assert got[r] == -np.inf and want[r] == -np.inf, (what, r, got[r])
    assert err < TOL, what


# ------------------------------------------------------------------------------------------ 1. the one-launch kernel
ONE_LAUNCH = [  # V, d, n, bias, pad (ldx = ldw = d + pad)
    (1, 4, 1, False, 0), (31, 64, 31, True, 0), (32, 132, 33, False, 4), (33, 64, 257, True, 0), (205, 1024, 257, True, 0),
    (256, 132, 33, False, 0), (257, 64, 31, True, 8), (260, 1024, 33, False, 0), (511, 4, 257, True, 0), (512, 132, 257, False, 4),
    (512, 1024, 257, True, 0),
    # long inputs: workgroups of 64 rows (n >= 32768) and, for V <= 256, of 128 rows (n >= 65536) -- every (row tiles, column tiles)
    # pair of the kernel, the last workgroup partial
    (33, 64, 32801, True, 0), (205, 64, 32801, False, 0), (260, 64, 32801, True, 0), (512, 64, 32801, True, 4),
    (33, 64, 65569, False, 0), (205, 64, 65569, True, 0),
]


@pytest.mark.parametrize("precision", [0, 3])
@pytest.mark.parametrize("V,d,n,with_bias,pad", ONE_LAUNCH)
def test_one_launch_kernel(dev, V, d, n, with_bias, pad, precision):
    rs, x, w, b = make_inputs(V * 7 + d + n, V, d, n, with_bias, pad)
    t, bad_rows = boundary_targets(rs, V, n)
    ds = build(dev, w, b, d, 1, precision)
    assert ds.route_name() == "one-launch"
    xd = torch.from_numpy(x).to(dev)
    got = ds.target_log_prob(xd[:, :d], torch.from_numpy(t).to(dev)).cpu().numpy()          # a view: ldx = d + pad
    assert not ds._ws                                                                       # no workspace on this route
    check(got, reference(x, w, b, t, d, precision), bad_rows, f"route 1 V={V} d={d} n={n} bias={with_bias} ld+{pad} prec={precision}")


@pytest.mark.parametrize("precision", [0, 3])
@pytest.mark.parametrize("V", [205, 512])
def test_one_launch_kernel_subtracts_the_maximum(dev, V, precision):
    """Logits scaled x30: exp(logit) overflows float32 (> 88.7) unless the row maximum is subtracted first, and every output must
    be finite.  At this scale a logit is ~100 and its float32 half-ulp 3.8e-6, so the GEMM's own rounding (checked by the cases
    above at the scale the project's 2e-5 is meant for) would eat the tolerance: the operands lie on a dyadic grid (x = 30 i / 8,
    |i| <= 8; w = j / 8, |j| <= 3; bias = k / 16), every product and every partial sum is exact in float32 and in float16 x float16,
    and what is left is the softmax's arithmetic -- the final rounding of a result below 256 (7.6e-6) plus the exp / log (~1e-6)."""
    d, n = 64, 257
    rs = np.random.RandomState(V)
    x = (30.0 * rs.randint(-8, 9, size=(n, d)) / 8.0).astype(np.float32)
    w = (rs.randint(-3, 4, size=(V, d)) / 8.0).astype(np.float32)
    b = (rs.randint(-32, 33, size=V) / 16.0).astype(np.float32)
    t, _ = boundary_targets(rs, V, n, bad=False)
    logits = x.astype(np.float64) @ w.astype(np.float64).T + b
    assert (logits.max(axis=1) > 89.0).mean() > 0.5                                                # exp overflows in most rows
    assert np.abs(ref.dense_logp64(x, w, b, t)).max() < 256                                        # (the final rounding's half-ulp: 7.6e-6)
    assert np.array_equal(ref.half_round(x), x) and np.array_equal(ref.half_round(w), w)           # exact under precision 3 too
    ds = build(dev, w, b, d, 1, precision)
    got = ds.target_log_prob(torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
    assert np.isfinite(got).all()
    check(got, ref.dense_logp64(x, w, b, t), [], f"x30 V={V} prec={precision}")


# ------------------------------------------------------------------------------------------ 2. the general route
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("V,precision", [(205, 0), (513, 0), (1000, 0), (5000, 0), (205, 3), (1000, 2)])
def test_general_route(dev, V, with_bias, precision):
    """n = 300 with the least workspace the library accepts: with a bias the logits go through it in 128-row chunks -- 128, 128
    and a partial one of 44."""
    from gnnlm_amd import _lib
    d, n = 64, 300
    rs, x, w, b = make_inputs(V + 11, V, d, n, with_bias)
    t, bad_rows = boundary_targets(rs, V, n)
    ds = build(dev, w, b, d, 2, precision)
    ds.small_workspace = True
    assert ds.route_name() == "general"
    got = ds.target_log_prob(torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
    L = _lib.lib()
    least, full = L.gnnlm_dense_workspace_bytes_min(ctypes.byref(ds._w), n), L.gnnlm_dense_workspace_bytes(ctypes.byref(ds._w), n)
    (ws,) = ds._ws.values()
    assert ws.numel() == least
    if with_bias:
        row_bytes = 4 * ((V + 3) // 4 * 4)
        assert (full - least) == (n - 128) * row_bytes            # the default holds all 300 rows, the least one 128: 3 chunks, 44 rows last
    else:
        assert full == least
    # precision 2 (bf16x6) is f32-level; precision 3 is compared on the pre-rounded operands
    check(got, reference(x, w, b, t, d, precision), bad_rows, f"route 2 V={V} bias={with_bias} prec={precision}")
    if with_bias:                                                 # chunking changes nothing: the default workspace gives the same bits
        ds.small_workspace = False
        again = ds.target_log_prob(torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)).cpu().numpy()
        assert np.array_equal(again, got)


@pytest.mark.parametrize("precision", [0, 3])
@pytest.mark.parametrize("V", [205, 512])
def test_routes_agree(dev, V, precision):
    d, n = 132, 257
    for with_bias in (False, True):
        rs, x, w, b = make_inputs(V + precision, V, d, n, with_bias)
        t, bad_rows = boundary_targets(rs, V, n)
        xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
        one = build(dev, w, b, d, 1, precision).target_log_prob(xd, td).cpu().numpy().astype(np.float64)
        two = build(dev, w, b, d, 2, precision).target_log_prob(xd, td).cpu().numpy().astype(np.float64)
        auto = build(dev, w, b, d, 0, precision).target_log_prob(xd, td).cpu().numpy().astype(np.float64)
        ok = np.ones(n, bool)
        ok[bad_rows] = False
        err = float(np.abs(one[ok] - two[ok]).max())
        print(f"V={V} prec={precision} bias={with_bias}: max |route 1 - route 2| = {err:.2e}")
        assert err < TOL and np.array_equal(one[~ok], two[~ok]) and np.isneginf(one[~ok]).all()
        assert np.array_equal(auto, one) or np.array_equal(auto, two)             # auto is one of the two


# ------------------------------------------------------------------------------------------ 3. the fixture through GnnLmModel
def test_fixture_through_the_model(dev, golden):
    """The reference's recorded target column for every case and ratio, with the fixture's GNN output fed straight to
    target_log_probs (no graph decoder: the decoder's place is taken by the scripted output, the base branch reads h)."""
    from gnnlm_amd import ops
    from gnnlm_amd.dense_softmax import DenseSoftmax
    from gnnlm_amd.model import GnnLmModel
    g = golden("dense_head")
    x, h = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["h"]).to(dev)
    tgt = torch.from_numpy(g["target"]).to(dev)
    ratios = [float(a) for a in g["ratios"]]
    for kind, with_bias in ref.CASES:
        w, b = ref.case_weights(g, kind, with_bias)
        name = ref.case_name(kind, with_bias)
        ds = DenseSoftmax(torch.from_numpy(w), None if b is None else torch.from_numpy(b), dev)
        plain = ds.target_log_prob(x.reshape(-1, x.shape[-1]), tgt.reshape(-1)).view(tgt.shape)
        single = {}
        for a in ratios:
            model = GnnLmModel(None, ds, None, orig_prob_ratio=a)
            extra = {"orig_x": h, "orig_ratio": a} if a > 0 else {}
            got = model.target_log_probs((x, extra), tgt)
            single[a] = got.clone()
            err = float((got.double().cpu() - torch.from_numpy(g[f"logp.{name}.{a}"]).double()).abs().max())
            print(f"{name} ratio {a}: max |ours - reference| = {err:.2e}")
            assert err < TOL
            if a > 0:                                             # the two unmixed rows are left for a sweep
                assert torch.equal(extra["branch_logp"][0], plain)
        assert torch.equal(single[0.0], plain)                    # ratio 0 is the plain call, bit for bit
        # a driver that sweeps the ratio (keep_branches) mixes the two rows of one pass at every ratio: the single-ratio runs
        model = GnnLmModel(None, ds, None)
        model.keep_branches = True
        extra = {"orig_x": h, "orig_ratio": 0.0}
        assert torch.equal(model.target_log_probs((x, extra), tgt), plain)
        gnn, base = extra["branch_logp"]
        rows = ops.logp_mix(gnn.reshape(-1), base.reshape(-1), ratios + [1.0])
        for i, a in enumerate(ratios):
            assert torch.equal(rows[i].view(tgt.shape), single[a]), (name, a)
        err1 = float((rows[-1].double().cpu().view(tgt.shape) - torch.from_numpy(g[f"logp.{name}.1.0"]).double()).abs().max())
        assert err1 < TOL                                         # the sweep's point 1: the base LM alone, as the reference's ratio 1


# ------------------------------------------------------------------------------------------ 4. from_checkpoint
def _checkpoint(tmp_path, name, shared, with_bias, adaptive=False, V=205):
    from gnnlm_amd.synthetic import make_problem
    d, H = 64, 4
    prob = make_problem(n_store=500, d=d, n_heads=H, M=16, dsub=4, vocab=V, cutoff=[50, 100], T=16, kg=4, left=1, right=1,
                        n_layers=1, k=4, seed=2)
    rs = np.random.RandomState(5)
    sd = {"decoder.hgt_decoder." + k: v for k, v in prob["sd"].items()}
    sd["decoder.tgt_quantizer.centroids_torch"] = torch.from_numpy(prob["cen"])
    sd["decoder.tgt_quantizer.A"] = torch.from_numpy(prob["A"])
    sd["decoder.tgt_quantizer.b"] = torch.from_numpy(prob["b"])
    margs = Namespace(decoder_embed_dim=d, decoder_attention_heads=H, graph_layer=1, decoder_gcn_dim=d, orig_prob_ratio=0.0,
                      short_cut=False, quantizer_path="")
    if adaptive:
        w = prob["asm"]
        for i, e in enumerate(w["emb"]):
            sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = e
            if i:
                sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = w["proj"][i]
        sd["decoder.adaptive_softmax.head.class_proj.weight"] = w["class_proj"]
        margs.adaptive_softmax_cutoff = "50,100"
    else:
        sd["decoder.embed_tokens.weight"] = torch.from_numpy((rs.randn(V, d) / 8).astype(np.float32))
        if not shared:
            sd["decoder.embed_out"] = torch.from_numpy((rs.randn(V, d) / 8).astype(np.float32))
        if with_bias:
            sd["decoder.xl_bias"] = torch.from_numpy((rs.randn(V) / 2).astype(np.float32))
        margs.share_decoder_input_output_embed = shared
        margs.adaptive_softmax_cutoff = None
    path = str(tmp_path / name)
    torch.save({"args": margs, "model": sd}, path)
    return path, sd, prob


def test_from_checkpoint(dev, tmp_path):
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    from gnnlm_amd.dense_softmax import DenseSoftmax
    from gnnlm_amd.model import GnnLmModel
    for shared in (True, False):
        for with_bias in (False, True):
            path, sd, _ = _checkpoint(tmp_path, f"dense_{shared}_{with_bias}.pt", shared, with_bias)
            model, _ = GnnLmModel.from_checkpoint(path, dev, vocab_size=205)
            head = model.adaptive_softmax
            assert isinstance(head, DenseSoftmax) and head.vocab == 205 and head.d == 64
            assert torch.equal(head.weight.cpu(), sd["decoder.embed_tokens.weight" if shared else "decoder.embed_out"])
            assert (head.bias is not None) == with_bias and (not with_bias or torch.equal(head.bias.cpu(), sd["decoder.xl_bias"]))
            assert model.precision == "f32"
            model.precision = "fp16"
            assert head.gemm_precision == 3
    model, _ = GnnLmModel.from_checkpoint(path, dev)                       # no dictionary size given: the weight's own
    assert model.adaptive_softmax.vocab == 205
    with pytest.raises(ValueError, match=r"600.*205|205.*600"):
        GnnLmModel.from_checkpoint(path, dev, vocab_size=600)
    path, _, _ = _checkpoint(tmp_path, "adaptive.pt", False, False, adaptive=True)
    model, _ = GnnLmModel.from_checkpoint(path, dev, vocab_size=205)
    assert isinstance(model.adaptive_softmax, AdaptiveSoftmax) and model.adaptive_softmax.cutoff == [50, 100, 205]


# ------------------------------------------------------------------------------------------ 5. graph capture
@pytest.mark.parametrize("route,with_bias", [(1, True), (2, False), (2, True)])
def test_target_log_prob_is_graph_capturable(dev, route, with_bias):
    """Captured on a side stream after an eager warm-up (the pattern of test_fp16_step_is_graph_capturable): the replay equals the
    eager result bit for bit, and follows new targets written into the captured buffer."""
    V, d, n = 205, 64, 300
    rs, x, w, b = make_inputs(3, V, d, n, with_bias)
    ds = build(dev, w, b, d, route, 0)
    ds.small_workspace = route == 2                                        # (the chunk loop inside the capture)
    xd = torch.from_numpy(x).to(dev)
    td = torch.from_numpy(rs.randint(0, V, size=n).astype(np.int64)).to(dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        eager = ds.target_log_prob(xd, td).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ds.target_log_prob(xd, td)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    td.copy_(torch.roll(td, 1))
    g.replay()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        again = ds.target_log_prob(xd, td)
    torch.cuda.synchronize()
    assert torch.equal(out, again) and not torch.equal(out, eager)


# ------------------------------------------------------------------------------------------ 6. the driver
V_E2E = 205


def make_dense_dir(tmp_path, sizes):
    """The tiny data directory of the driver tests (tests/test_ragged_gpu.py::make_ragged_dir) with a 205-entry vocabulary, a
    1-layer HGT and a dense checkpoint with xl_bias (unshared output weights)."""
    import os
    from gnnlm_amd.synthetic import make_problem
    from test_ragged_gpu import write_idx_bin
    d, H, M, dsub, V, kg, L = 64, 4, 16, 4, V_E2E, 6, 1
    n_train, n_test = 2000, int(np.sum(sizes))
    prob = make_problem(n_store=n_train, d=d, n_heads=H, M=M, dsub=dsub, vocab=V, cutoff=[50, 100], T=n_test, kg=kg, left=2, right=2,
                        n_layers=L, k=8, seed=3)
    data = tmp_path / "data-bin"

    def write_dstore(path, keys, vals):
        os.makedirs(path, exist_ok=True)
        keys.tofile(os.path.join(path, "keys.npy"))
        vals.tofile(os.path.join(path, "vals.npy"))
        json.dump({"dstore_size": len(vals), "hidden_size": keys.shape[1], "vocab_size": V, "dstore_fp16": True, "val_size": 1},
                  open(os.path.join(path, "info.json"), "w"))

    rs = np.random.RandomState(0)
    train_keys = rs.randn(n_train, d).astype(np.float16)
    write_dstore(str(data / "train_dstore"), train_keys, prob["vals"].astype(np.int16))
    np.save(str(data / "train_dstore" / "quantized-keys.npy"), prob["codes"])
    blk = prob["block"]
    blk["targets"] = np.maximum(blk["targets"], 4)        # ids 0-3 are fairseq's specials
    write_dstore(str(data / "test_dstore"), blk["tgt_feats"], blk["targets"].astype(np.int16))
    blk["ids"].tofile(str(data / "test_dstore" / f"neighbors.mmap.{kg}"))
    write_idx_bin(data, "test", sizes, blk["targets"])
    sd = {"decoder.hgt_decoder." + k: v for k, v in prob["sd"].items()}
    w_out = (rs.randn(V, d) / 8).astype(np.float32)        # features are LayerNorm outputs: logits with a standard deviation of ~1
    bias = (rs.randn(V) / 2).astype(np.float32)
    sd["decoder.embed_tokens.weight"] = torch.from_numpy((rs.randn(V, d) / 8).astype(np.float32))     # the input embedding: not the head
    sd["decoder.embed_out"] = torch.from_numpy(w_out)
    sd["decoder.xl_bias"] = torch.from_numpy(bias)
    sd["decoder.tgt_quantizer.centroids_torch"] = torch.from_numpy(prob["cen"])
    sd["decoder.tgt_quantizer.A"] = torch.from_numpy(prob["A"])
    sd["decoder.tgt_quantizer.b"] = torch.from_numpy(prob["b"])
    margs = Namespace(decoder_embed_dim=d, decoder_attention_heads=H, graph_layer=L, decoder_gcn_dim=d, adaptive_softmax_cutoff=None,
                      share_decoder_input_output_embed=False, orig_prob_ratio=0.0, short_cut=False, quantizer_path="")
    torch.save({"args": margs, "model": sd}, str(tmp_path / "ckpt.pt"))
    base = [str(data), "--path", str(tmp_path / "ckpt.pt"), "--gen-subset", "test", "--graph", "--neighbor-context", "2",
            "--gcn-k", str(kg), "--use-precompute-feat", "--knn-keytype", "gcn_feat"]
    model = {"sd": prob["sd"], "n_layers": L, "n_heads": H, "centroids": prob["cen"], "A": prob["A"], "b": prob["b"],
             "codes": prob["codes"], "vals": prob["vals"], "n_store": n_train, "left": 2, "right": 2}
    return dict(prob=prob, blk=blk, data=data, base=base, model=model, train_keys=train_keys, n_test=n_test, w=w_out, bias=bias)


def restatement(c, ranges, lam=0.0, temp=1.0, k=8, ratio=0.0):
    """Sum of the scored tokens' log-probs over (context_start, start, end) blocks: the oracle's graph and HGT in float64, the
    dense head of tests/dense_head_ref.py, the exact kNN term of tests/test_ragged_gpu.py::oracle_run."""
    from oracle import knn as oknn_, pipeline
    blk, m, total, count = c["blk"], c["model"], 0.0, 0
    for cs, s, e in ranges:
        g, ncodes, _ = pipeline.gather_block(blk["ids"][cs:e], m["codes"], m["vals"], m["n_store"], m["left"], m["right"])
        feats = pipeline.hgt_block(m["sd"], m["n_layers"], m["n_heads"], blk["tgt_feats"][cs:e], ncodes, g, m["centroids"], m["A"], m["b"],
                                   torch.float64)["tgt"]
        tgt = blk["targets"][cs:e]
        lm = ref.dense_logp64(feats.numpy(), c["w"], c["bias"], tgt)
        if ratio > 0:
            lm = ref.mix64(ref.dense_logp64(blk["tgt_feats"][cs:e].astype(np.float64), c["w"], c["bias"], tgt), lm, ratio)
        if lam > 0:
            q = oknn_.normalize_queries(feats.float(), True).numpy()
            dd, ii = oknn_.brute_force_search(q, c["train_keys"], k, "ip", cosine=True)
            p, _ = oknn_.knn_target_prob(dd, ii, c["prob"]["vals"], tgt, temp)
            lm = oknn_.combine_knn_and_vocab_probs(p, torch.from_numpy(lm).float(), lam).double().numpy()
        total += float(lm[s - cs:].sum())
        count += e - s
    return total, count


@pytest.mark.parametrize("mode", ["plain", "knnlm", "fp16", "eos"])
def test_eval_lm_dense_head(dev, tmp_path, caplog, mode):
    """eval_lm.main on a dense checkpoint with bias: the perplexity within the 0.02 of the driver tests of the float64
    restatement, the head's log line, "head": "dense" in --result-json.  `plain` also runs the ratio sweep."""
    from test_ragged_gpu import SENT_SIZES
    from gnnlm_amd import eval_lm, token_blocks
    c = make_dense_dir(tmp_path, SENT_SIZES)
    T, lam, k = 64, 0.25, 8
    # (--knnlm: one block per batch, the recipe's shape -- with more, the reference pairs queries [T, B] with targets [B, T],
    # sequence_scorer.py:117, a quirk the driver reproduces and this restatement does not model)
    args = c["base"] + ["--tokens-per-sample", str(T), "--max-tokens", str(T if mode == "knnlm" else 2 * T), "--gcn-context-window", "0"]
    if mode == "knnlm":
        args += ["--knnlm", "--k", str(k), "--lmbda", str(lam), "--dstore-dir", str(c["data"] / "train_dstore"),
                 "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]
    if mode == "fp16":
        args += ["--fp16"]
    if mode == "eos":
        args += ["--sample-break-mode", "eos"]
    ranges = token_blocks.block_ranges(SENT_SIZES, "eos" if mode == "eos" else "none", T, 0)
    total, count = restatement(c, ranges, lam if mode == "knnlm" else 0.0, 1.0, k)
    out = str(tmp_path / "res.json")
    with caplog.at_level(logging.INFO):
        caplog.clear()
        res = eval_lm.cli_main(args + ["--result-json", out])
    lines = [r.getMessage() for r in caplog.records if "output layer: dense softmax" in r.getMessage()]
    route = "one-launch" if mode == "fp16" else "general"            # what auto resolves to
    assert lines == [f"output layer: dense softmax, V = {V_E2E}, bias yes, route {route}"], lines
    assert json.load(open(out))["head"] == "dense" and res["head"] == "dense"
    ref_ppl = math.exp(-total / count)
    print(f"{mode}: {count} tokens, ppl {res['ppl']:.4f} (float64 restatement {ref_ppl:.4f}), score_sum {res['score_sum']:.5f} ({total:.5f})")
    assert res["count"] == count == c["n_test"]
    assert abs(res["ppl"] - ref_ppl) < 0.02
    if mode == "plain":
        cap = eval_lm.cli_main(args + ["--graph-capture"])                        # the head inside the shape's replayed graph
        assert cap["count"] == count and abs(cap["score_sum"] - res["score_sum"]) < 1e-6 * count
        # the ratio through the existing sweep: its rows are the single-ratio runs
        sw = eval_lm.cli_main(args + ["--sweep-orig-prob-ratio", "0,0.5,1"])
        rows = {r["orig_prob_ratio"]: r for r in sw["sweep"]}
        one = eval_lm.cli_main(args + ["--model-overrides", "{'orig_prob_ratio': 0.5}"])
        assert abs(rows[0.0]["score_sum"] - res["score_sum"]) < 1e-6 * count
        assert abs(rows[0.5]["score_sum"] - one["score_sum"]) < 1e-6 * count
        for a in (0.5, 1.0):
            t_a, _ = restatement(c, ranges, ratio=a)
            print(f"ratio {a}: ppl {rows[a]['ppl']:.4f} (float64 restatement {math.exp(-t_a / count):.4f})")
            assert abs(rows[a]["ppl"] - math.exp(-t_a / count)) < 0.02
