"""``orig_prob_ratio`` > 0 on the device: the base-LM / GNN mixture (transformer.py:987-1005,1056-1077) from the mix kernel up to
the driver, and the ratio as the outer axis of the tuning sweep.  The bar for log-probs is the project's 2e-5 absolute."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orig_ratio.npz")
BAR = 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from gnnlm_amd import ops as o
    return o


def mix64(gnn, base, a):
    """float64 restatement of combinetow_probs on the target column."""
    with np.errstate(divide="ignore"):
        return np.logaddexp(np.log(np.float64(a)) + np.asarray(base, np.float64), np.log(1.0 - np.float64(a)) + np.asarray(gnn, np.float64))


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 8195])
def test_logp_mix_against_float64(ops, dev, n, A):
    rs = np.random.RandomState(n * 10 + A)
    gnn = (-12.0 * rs.rand(n)).astype(np.float32)
    base = (gnn + rs.randn(n) * 3.0).astype(np.float32)
    base[::5] = gnn[::5] - 80.0                                  # pairs 80 apart, either way round: no underflow to -inf
    base[1::7] = gnn[1::7] + 80.0
    alphas = [0.3, 0.0, 1.0, 0.5, 1e-6, 0.999, 0.1, 0.9][:A]
    g_d, b_d = torch.from_numpy(gnn).to(dev), torch.from_numpy(base).to(dev)
    out = ops.logp_mix(g_d, b_d, alphas)
    assert out.shape == (A, n) and out.dtype == torch.float32
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    for j, a in enumerate(alphas):
        # the coefficients are the float32 roundings of the float64 logs (as the reference's float32 coeffs tensor holds them)
        c0, c1 = np.float64(np.float32(math.log(a))) if a > 0 else -np.inf, np.float64(np.float32(math.log1p(-a))) if a < 1 else -np.inf
        want = np.logaddexp(c0 + base.astype(np.float64), c1 + gnn.astype(np.float64))
        err = np.abs(got[j] - want).max()
        print(f"n {n} A {A} alpha {a}: max |d| = {err:.2e}")
        assert err < BAR
        if a == 0.0:
            assert torch.equal(out[j], g_d)
        if a == 1.0:
            assert torch.equal(out[j], b_d)
    # each row equals the one-ratio call: one read serves all rows, nothing else changes
    for j, a in enumerate(alphas):
        assert torch.equal(ops.logp_mix(g_d, b_d, [a])[0], out[j])


def test_logp_mix_refusals(ops, dev):
    from gnnlm_amd import _lib
    g_d = torch.full((65,), -3.0, device=dev)
    b_d = torch.full((65,), -4.0, device=dev)
    for alphas in ([-0.1], [1.5], [0.2, float("nan")], [0.1] * 9, []):
        out = torch.full((len(alphas), 65), 7.0, device=dev)
        with pytest.raises(_lib.GnnlmError):
            ops.logp_mix(g_d, b_d, alphas, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())                              # nothing was launched
    with pytest.raises(_lib.GnnlmError):
        ops.logp_mix(g_d.cpu(), b_d.cpu(), [0.5])
    with pytest.raises(TypeError):
        ops.logp_mix(g_d.double(), b_d.double(), [0.5])


def grid_inputs(n, k, A, seed):
    rs = np.random.RandomState(seed)
    sims = np.sort(rs.randn(n, k).astype(np.float32) * 4.0, axis=1)[:, ::-1].copy()
    ids = rs.randint(0, 5000, size=(n, k)).astype(np.int64)
    ids[::3, -2:] = -1
    kv = rs.randint(0, 50, size=(n, k)).astype(np.int32)
    tg = rs.randint(0, 50, size=n).astype(np.int64)
    lm = (-10.0 * rs.rand(A, n)).astype(np.float32)
    return lm, sims, ids, kv, tg


@pytest.mark.parametrize("k,A,grid", [
    (64, 2, ([64, 7], [1.0], [0.25])),
    (1000, 3, ([1000, 256, 64], [1.0, 0.1, 0.01, 10.0, 0.5], [0.0, 0.1, 0.25, 0.5, 1.0])),       # 3 x 5 x 5 x 5
    (1024, 8, ([1024, 300], [1.0, 0.01], [0.0, 0.25, 1.0])),
    (1024, 8, ([1024], [1.0], [j / 16 for j in range(16)])),                                      # 128 mixes: both rounds of lanes
    (200, 5, ([200, 1], [0.3], [j / 13 for j in range(13)])),                                     # 65 mixes: one lane in round two
], ids=["k64", "k1000-3x5x5x5", "k1024-A8", "k1024-128mixes", "k200-65mixes"])
def test_grid_lm_rows_equal_the_single_row_grid(ops, dev, k, A, grid):
    n = 301
    lm, sims, ids, kv, tg = grid_inputs(n, k, A, k + A)
    t = lambda a: torch.from_numpy(a).to(dev)
    lm_d, rest = t(lm), (t(sims), t(ids), t(tg))
    out, pk, rec = ops.knn_interp_grid(lm_d, *rest, *grid, knn_vals=t(kv))
    G = len(ops.grid_points(*grid))
    assert out.shape == (A * G, n) and pk.shape == (len(grid[0]) * len(grid[1]), n) and rec.shape == (len(grid[0]), n)
    for a in range(A):
        one, pk1, rec1 = ops.knn_interp_grid(lm_d[a].contiguous(), *rest, *grid, knn_vals=t(kv))
        assert torch.equal(out[a * G:(a + 1) * G], one), a
        assert torch.equal(pk, pk1) and torch.equal(rec, rec1)
    # the 1-D call through both entries
    one, pk1, rec1 = ops.knn_interp_grid(lm_d[0].contiguous(), *rest, *grid, knn_vals=t(kv))
    via_lm, pk2, rec2 = ops.knn_interp_grid(lm_d[:1].contiguous(), *rest, *grid, knn_vals=t(kv))
    assert torch.equal(one, via_lm) and torch.equal(pk1, pk2) and torch.equal(rec1, rec2)
    # ... and against the single-setting kernel where that is defined
    kp, tt, ll = grid[0][0], grid[1][0], grid[2][-1]
    if 0 < ll < 1:
        single = ops.knn_interp(lm_d[A - 1].contiguous(), t(sims[:, :kp].copy()), t(ids[:, :kp].copy()), t(tg), tt, ll, knn_vals=t(kv[:, :kp].copy()))[0]
        assert torch.equal(out[(A - 1) * G + ops.grid_points(*grid).index((kp, tt, ll))], single)


def test_grid_lm_refusals(ops, dev):
    from gnnlm_amd import _lib
    lm, sims, ids, kv, tg = grid_inputs(10, 64, 9, 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    with pytest.raises(_lib.GnnlmError, match="lm rows"):
        ops.knn_interp_grid(t(lm), t(sims), t(ids), t(tg), [64], [1.0], [0.5], knn_vals=t(kv))
    with pytest.raises(ValueError):
        ops.knn_interp_grid(t(lm)[:, :5].contiguous(), t(sims), t(ids), t(tg), [64], [1.0], [0.5], knn_vals=t(kv))


# ---------------------------------------------------------------------------------------------------------------------------------
# model, engine
# ---------------------------------------------------------------------------------------------------------------------------------
def fixture_model(dev, alpha, short_cut=False):
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    from gnnlm_amd.model import GnnLmModel
    g = np.load(GOLDEN)
    emb = [torch.from_numpy(g[f"emb{i}"]) for i in range(3)]
    proj = [None] + [torch.from_numpy(g[f"proj{i}"]) for i in (1, 2)]
    asm = AdaptiveSoftmax([int(c) for c in g["cutoff"]], emb, proj, torch.from_numpy(g["class_proj"]), dev)
    x, h = torch.from_numpy(g["x"]).to(dev), torch.from_numpy(g["h"]).to(dev)

    class Scripted(GnnLmModel):                       # the forward scripted (the fixture has no graph), the rest is the model's own
        def __init__(self):
            GnnLmModel.__init__(self, None, asm, None, orig_prob_ratio=alpha, short_cut=short_cut)

        def forward(self, src_tokens=None, src_lengths=None, graph=None):
            extra = {"inner_states": [h.transpose(0, 1)], "gcn_feat": x.transpose(0, 1)}
            if self.orig_prob_ratio > 0 or self.keep_branches:
                extra["orig_x"], extra["orig_ratio"] = h, self.orig_prob_ratio
            return (h if short_cut else x), extra

    return Scripted(), g, torch.from_numpy(g["target"]).to(dev)


def test_model_on_the_fixture(dev):
    plain, g, target = fixture_model(dev, 0.0)
    gnn0 = plain.target_log_probs(plain(), target)
    for a in (0.1, 0.3, 0.5, 0.9):
        model, _, _ = fixture_model(dev, a)
        out = model()
        got = model.target_log_probs(out, target)
        err = float(np.abs(got.cpu().numpy() - g[f"mixed.{a}"]).max())
        print(f"alpha {a}: max |model - reference| = {err:.2e}")
        assert got.shape == target.shape and err < BAR
        gnn, base = out[1]["branch_logp"]
        assert torch.equal(gnn, gnn0)                                 # the GNN branch is the alpha = 0 model's, bit for bit
        assert np.abs(got.cpu().numpy() - mix64(gnn.cpu().numpy(), base.cpu().numpy(), a)).max() < BAR
    # a row's result does not depend on how many rows the call has: one call over the stacked [2n, d] rows gives both branches
    model, _, _ = fixture_model(dev, 0.3)
    out = model()
    model.target_log_probs(out, target)
    x2, h2, t2 = out[0].reshape(-1, out[0].shape[-1]), out[1]["orig_x"].reshape(-1, out[0].shape[-1]), target.reshape(-1)
    both = model.adaptive_softmax.target_log_prob(torch.cat([x2, h2]), torch.cat([t2, t2])).view(2, *target.shape)
    assert torch.equal(both[0], out[1]["branch_logp"][0]) and torch.equal(both[1], out[1]["branch_logp"][1]) and torch.equal(both[0], gnn0)
    # short_cut: both branches on h -> the mixture of a distribution with itself, whatever alpha
    sc, _, _ = fixture_model(dev, 0.3, short_cut=True)
    out = sc()
    got = sc.target_log_probs(out, target)
    assert torch.equal(out[1]["branch_logp"][0], out[1]["branch_logp"][1])
    assert float((got - out[1]["branch_logp"][1]).abs().max()) < BAR
    # keep_branches with the model's own ratio at 0: the branches are there, the result is the GNN's
    base_sc = out[1]["branch_logp"][1]                               # (the softmax of h)
    plain.keep_branches = True
    out = plain()
    assert torch.equal(plain.target_log_probs(out, target), gnn0)
    assert torch.equal(out[1]["branch_logp"][0], gnn0) and torch.equal(out[1]["branch_logp"][1], base_sc)


def test_model_forward_puts_orig_x(dev):
    """The model's own _forward (not scripted): extra["orig_x"] is the float32 h [bsz, tgt_len, d], extra["orig_ratio"] the ratio."""
    from gnnlm_amd.hgt import NeighborGraph
    from gnnlm_amd.model import GnnLmModel
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=1, k=32, seed=1)
    eng, batch = build_engine(prob, dev), to_batch(prob["block"], dev)
    n = batch.targets.shape[0]
    graph = NeighborGraph(ids=batch.ids, n_blocks=batch.n_blocks, T=batch.T, left=eng.left, right=eng.right, store=eng.store, tgt_h=batch.tgt_feats)
    tokens = batch.targets.view(batch.n_blocks, batch.T)
    for a, sc in ((0.0, False), (0.3, False), (0.3, True)):
        model = GnnLmModel(eng.hgt, eng.asm, None, orig_prob_ratio=a, short_cut=sc)
        x, extra = model(tokens, graph=graph)
        assert ("orig_x" in extra) == (a > 0)
        got = model.target_log_probs((x, extra), tokens)
        ref = eng.score(batch, orig_prob_ratio=a)
        if a > 0:
            assert extra["orig_ratio"] == a and extra["orig_x"].dtype == torch.float32 and extra["orig_x"].shape == (batch.n_blocks, batch.T, 64)
            assert torch.equal(extra["orig_x"].reshape(n, -1), batch.tgt_feats.float())
        if not sc:
            assert torch.equal(got.reshape(-1), ref["lm_logp"])       # model and engine: the same calls
        else:
            assert float((got.reshape(-1) - ref["lm_logp_base"]).abs().max()) < BAR


def test_engine_orig_prob_ratio_and_four_axis_sweep(ops, dev):
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=16, kg=8,
                        left=2, right=2, n_layers=1, k=32, seed=1)
    eng, batch = build_engine(prob, dev), to_batch(prob["block"], dev)
    n = batch.targets.shape[0]
    zero = eng.score(batch)
    assert "lm_logp_gnn" not in zero
    for a in (0.3, 0.9):
        out = eng.score(batch, orig_prob_ratio=a)
        assert torch.equal(out["lm_logp_gnn"], zero["lm_logp"])
        want = mix64(out["lm_logp_gnn"].cpu().numpy(), out["lm_logp_base"].cpu().numpy(), a)
        assert np.abs(out["lm_logp"].cpu().numpy() - want).max() < BAR and torch.equal(out["logp"], out["lm_logp"])
        assert float((out["lm_logp_gnn"] - out["lm_logp_base"]).abs().max()) > 0.1
    for bad in (1.0, 1.5):
        with pytest.raises(ValueError, match="math domain error"):
            eng.score(batch, orig_prob_ratio=bad)
    assert torch.equal(eng.score(batch, orig_prob_ratio=-0.1)["lm_logp"], zero["lm_logp"])
    # the ratio alone
    alone = eng.score(batch, sweep=(None, None, None, [0.0, 0.3, 1.0]))
    assert alone["sweep_logp"].shape == (3, n) and torch.equal(alone["logp"], zero["lm_logp"])
    assert torch.equal(alone["sweep_logp"][0], zero["lm_logp"]) and torch.equal(alone["sweep_logp"][2], alone["lm_logp_base"])
    assert torch.equal(alone["sweep_logp"][1], eng.score(batch, orig_prob_ratio=0.3)["lm_logp"])

    # four axes, with the search inside the step (an index with the device-search contract, as tests/test_sweep_gpu.py scripts one)
    class Found:
        def __init__(self, r):
            self.r = r

        def result(self):
            return self.r

    class Index:
        def search_begin(self, q, k, return_vals=True):
            kv = eng.store.vals[torch.where(batch.knn_ids < 0, batch.knn_ids + eng.store.n_store, batch.knn_ids)].int()
            return Found((batch.knn_sims[:, :k].contiguous(), batch.knn_ids[:, :k].contiguous(), kv[:, :k].contiguous()))

    sweep = ([5, 32], [1.0, 0.1], [0.25, 0.5], [0.0, 0.3, 0.6])
    pts = ops.grid_points(*sweep)
    for kw in (dict(knn_index=Index(), k=32), dict()):                   # search inside the step / search given with the batch
        out = eng.score(batch, 0.25, 1.0, sweep=sweep, orig_prob_ratio=0.3, **kw)
        assert out["sweep_logp"].shape == (len(pts), n) == (24, n)
        assert torch.equal(out["sweep_logp"][pts.index((0.3, 32, 1.0, 0.25))], out["logp"])
        three = eng.score(batch, 0.25, 1.0, sweep=sweep[:3], orig_prob_ratio=0.3, **kw)             # 3-tuples behave as before
        assert three["sweep_logp"].shape == (8, n) and torch.equal(three["sweep_logp"], out["sweep_logp"][8:16])
        for g, (a, kp, t, l) in enumerate(pts):
            if kw:
                class IndexK(Index):
                    def search_begin(self, q, k, return_vals=True, kp=kp):
                        return Index.search_begin(self, q, kp, return_vals)
                one = eng.score(batch, l, t, knn_index=IndexK(), k=kp, orig_prob_ratio=a)
            else:
                import dataclasses
                b1 = dataclasses.replace(batch, knn_sims=batch.knn_sims[:, :kp].contiguous(), knn_ids=batch.knn_ids[:, :kp].contiguous())
                one = eng.score(b1, l, t, orig_prob_ratio=a)
            assert torch.equal(out["sweep_logp"][g], one["logp"]), (a, kp, t, l)


# ---------------------------------------------------------------------------------------------------------------------------------
# driver
# ---------------------------------------------------------------------------------------------------------------------------------
SENT_SIZES = [17, 1, 60, 5, 33, 1, 1, 48, 9, 26, 2, 41, 13, 1, 55, 30, 7, 22, 1, 38, 12, 19]
T_BLOCK, K = 64, 8


def restated(c, ranges, alpha, lam=0.0, temp=1.0, k=K, short_cut=False):
    """float64 restatement of the run: per block the oracle's HGT + adaptive softmax of x and of h in float64, the mixture, the exact
    kNN term on top -> (sum of the scored tokens' log-probs, count)."""
    from oracle import adaptive_softmax as oasm, knn as oknn, pipeline
    blk, total, count = c["blk"], 0.0, 0
    w = c["model"]["asm"]
    w64 = {"cutoff": w["cutoff"], "emb": [e.double() for e in w["emb"]], "proj": [None if p is None else p.double() for p in w["proj"]],
           "class_proj": w["class_proj"].double()}
    for cs, s, e in ranges:
        one = {"neighbor_idxs": blk["ids"][cs:e], "tgt_feats": blk["tgt_feats"][cs:e], "targets": blk["targets"][cs:e], "knn_sims": None, "knn_ids": None}
        o = pipeline.eval_block(one, c["model"], 0.0, 1.0, dtype=torch.float64)
        tgt = torch.as_tensor(blk["targets"][cs:e]).long()
        base = oasm.target_log_prob(torch.as_tensor(blk["tgt_feats"][cs:e]).double(), tgt, w64).numpy()
        gnn = base if short_cut else oasm.target_log_prob(o["gcn_feat"].double(), tgt, w64).numpy()
        lm = mix64(gnn, base, alpha)
        if lam > 0:
            q = oknn.normalize_queries((torch.as_tensor(blk["tgt_feats"][cs:e]) if short_cut else o["gcn_feat"]).float(), True).numpy()
            dd, ii = oknn.brute_force_search(q, c["train_keys"], k, "ip", cosine=True)
            p, _ = oknn.knn_target_prob(dd, ii, c["prob"]["vals"], blk["targets"][cs:e], temp)
            lm = np.logaddexp(math.log(1 - lam) + lm, math.log(lam) + np.log(p.double().numpy() + 1e-10))
        total += float(lm[s - cs:].sum())
        count += e - s
    return total, count


def knn_args(c, lam):
    return ["--knnlm", "--k", str(K), "--lmbda", str(lam), "--dstore-dir", str(c["data"] / "train_dstore"),
            "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]


def with_overrides(args, text):
    args = list(args)
    args[args.index("--model-overrides") + 1] = text
    return args


@pytest.mark.parametrize("variant", ["plain", "knnlm", "graph-capture", "streams-2", "break-mode-eos", "knnlm-break-mode-eos"])
def test_eval_lm_end_to_end(dev, tmp_path, capsys, variant):
    from gnnlm_amd import eval_lm, token_blocks
    from test_ragged_gpu import make_ragged_dir
    c = make_ragged_dir(tmp_path, SENT_SIZES, L=1)
    n_test = c["n_test"]
    mode = "eos" if "eos" in variant else "none"
    knn = "knnlm" in variant
    lam = 0.25 if knn else 0.0
    extra = {"graph-capture": ["--graph-capture", "--batch-blocks", "0"], "streams-2": ["--streams", "2"]}.get(variant, [])
    common = c["base"] + ["--sample-break-mode", mode, "--tokens-per-sample", str(T_BLOCK), "--max-tokens", str(2 * T_BLOCK if mode == "eos" else T_BLOCK),
                          "--gcn-context-window", "0"] + (knn_args(c, lam) if knn else []) + extra
    ranges = token_blocks.block_ranges(SENT_SIZES, mode, T_BLOCK, 0) if mode != "none" else eval_lm.block_ranges(n_test, T_BLOCK, 0)

    # {'orig_prob_ratio': 0.3} against the float64 restatement
    capsys.readouterr()
    r03 = eval_lm.cli_main(with_overrides(common, "{'orig_prob_ratio': 0.3}"))
    lines03 = capsys.readouterr().out.strip().split("\n")
    total, count = restated(c, ranges, 0.3, lam)
    ref_ppl = 2 ** (-total / count / math.log(2))
    print(f"{variant}: ppl {r03['ppl']:.5f} (float64 restatement {ref_ppl:.5f}), score_sum {r03['score_sum']:.6f} ({total:.6f})")
    assert r03["count"] == count == n_test and abs(r03["ppl"] - ref_ppl) < 0.02
    assert len(lines03) == 2 and "sweep" not in r03                          # no new flag: the two lines, nothing else
    capsys.readouterr()                                                       # (drop this test's own print)
    r0 = eval_lm.cli_main(common)                                             # the plain alpha = 0 run
    lines0 = capsys.readouterr().out.strip().split("\n")
    assert len(lines0) == 2 and abs(r0["ppl"] - r03["ppl"]) > 1e-3            # the ratio does something on this model
    # ratios >= 1 are the reference's ValueError, before any batch
    with pytest.raises(ValueError, match="math domain error"):
        eval_lm.cli_main(with_overrides(common, "{'orig_prob_ratio': 1.0}"))
    capsys.readouterr()

    # the sweep: run at 0.3, ratios 0, 0.3, 0.6, 1
    sw = eval_lm.cli_main(with_overrides(common, "{'orig_prob_ratio': 0.3}") + ["--sweep-orig-prob-ratio", "0,0.3,0.6,1"])
    lines = capsys.readouterr().out.strip().split("\n")
    assert sw["score_sum"] == r03["score_sum"] and sw["ppl"] == r03["ppl"] and lines[1] == lines03[1]
    rows = {r["orig_prob_ratio"]: r for r in sw["sweep"]}
    assert list(rows) == [0.0, 0.3, 0.6, 1.0] and len(lines) == 6 and lines[2:] == eval_lm.sweep_lines(sw["sweep"])
    if knn:
        assert all((r["k"], r["temperature"], r["lmbda"]) == (K, 1.0, lam) for r in sw["sweep"])
        assert lines[2].startswith(f"sweep orig_prob_ratio=0 k={K} temperature=1 lmbda=0.25 loss=")
    else:
        assert all("k" not in r for r in sw["sweep"]) and lines[3].startswith("sweep orig_prob_ratio=0.3 loss=")
    assert rows[0.3]["score_sum"] == sw["score_sum"]                          # exactly
    assert rows[0.0]["score_sum"] == r0["score_sum"]                          # exactly: the mix at 0 is the GNN branch bit for bit
    sc = eval_lm.cli_main(with_overrides(common, "{'orig_prob_ratio': 0.0, 'short_cut': True}"))
    capsys.readouterr()
    if not knn:                                                               # (with --knnlm a short_cut run also searches with other queries)
        print(f"row at 1: {rows[1.0]['score_sum']:.6f}, short_cut run {sc['score_sum']:.6f}")
        assert abs(rows[1.0]["score_sum"] - sc["score_sum"]) < BAR * n_test
    t06, _ = restated(c, ranges, 0.6, lam)
    assert abs(rows[0.6]["score_sum"] - t06) < 2e-4 * n_test                  # (the bar of the driver tests against the oracle)
    # a sweep runs the base branch even when the run's own ratio is 0, and the run's own figures do not move
    sw0 = eval_lm.cli_main(common + ["--sweep-orig-prob-ratio", "0,0.3,0.6,1"])
    capsys.readouterr()
    assert sw0["score_sum"] == r0["score_sum"] and [r["score_sum"] for r in sw0["sweep"]] == [r["score_sum"] for r in sw["sweep"]]
    if knn:
        # the outer axis of the existing grid
        full = eval_lm.cli_main(with_overrides(common, "{'orig_prob_ratio': 0.3}") +
                                ["--sweep-orig-prob-ratio", "0,0.3", "--sweep-lmbda", "0,0.25", "--sweep-k", "4,8"])
        capsys.readouterr()
        assert [(r["orig_prob_ratio"], r["k"], r["lmbda"]) for r in full["sweep"]] == [(a, k_, l) for a in (0.0, 0.3) for k_ in (4, 8) for l in (0.0, 0.25)]
        at = {(r["orig_prob_ratio"], r["k"], r["lmbda"]): r["score_sum"] for r in full["sweep"]}
        assert at[(0.3, 8, 0.25)] == r03["score_sum"] and at[(0.0, 8, 0.25)] == r0["score_sum"]
        three = eval_lm.cli_main(common + ["--sweep-lmbda", "0,0.25", "--sweep-k", "4,8"])
        capsys.readouterr()
        assert all("orig_prob_ratio" not in r for r in three["sweep"])
        assert [r["score_sum"] for r in three["sweep"]] == [r["score_sum"] for r in full["sweep"][:4]]


def test_eval_lm_ratio_sweep_two_ranks(dev, tmp_path):
    """Two ranks on one GPU over host-staged collectives (as test_eval_lm_sweep_two_ranks runs them): the sums of the ratio axis
    travel in the run's one all_reduce and rank 0 prints the same table as one process."""
    import json
    import subprocess
    import sys
    from test_mirrors_gpu import make_data_dir
    c = make_data_dir(tmp_path, n_test=100, L=1)
    base = with_overrides(c["base"], "{'orig_prob_ratio': 0.3}")
    base[base.index("--max-tokens") + 1] = str(c["T"])
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    knn = ["--knnlm", "--k", "8", "--lmbda", "0.25", "--dstore-dir", str(c["data"] / "train_dstore"),
           "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]
    sweep = ["--sweep-orig-prob-ratio", "0,0.3,1", "--sweep-lmbda", "0,0.25"]

    def run(extra, ranks, port):
        out = str(tmp_path / f"res_{port}.json")
        cmd = [sys.executable] + (["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
                                   "--master-port", str(port)] if ranks > 1 else []) + \
            ["-m", "gnnlm_amd.eval_lm"] + base + knn + sweep + extra + ["--result-json", out]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(env, GNNLM_EVAL_BACKEND="gloo", GNNLM_EVAL_DEVICE="0"))
        assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
        return [l_ for l_ in p.stdout.splitlines() if l_.startswith(("Evaluated", "Loss", "sweep"))], json.load(open(out))
    one_lines, one = run([], 1, 0)
    assert len(one_lines) == 8 and len(one["sweep"]) == 6 and all(l_.startswith("sweep orig_prob_ratio=") for l_ in one_lines[2:])
    for i, extra in enumerate([["--store", "sharded"], ["--store", "replicated"]]):
        lines, res = run(extra, 2, 29790 + i)
        assert lines[1:] == one_lines[1:], (extra, lines, one_lines)
        assert res["world"] == 2 and res["count"] == 100
        for a, b in zip(res["sweep"], one["sweep"]):
            assert (a["orig_prob_ratio"], a["k"], a["lmbda"]) == (b["orig_prob_ratio"], b["k"], b["lmbda"])
            assert abs(a["score_sum"] - b["score_sum"]) <= 1e-12 * abs(b["score_sum"])


def test_alpha_zero_issues_no_new_kernels(dev, tmp_path, monkeypatch):
    """alpha = 0 and no new flag: one softmax call per batch and no mix, as before the feature.  A ratio adds, per batch, exactly
    the launches of one more isolated ``target_log_prob`` call (the base branch, counted on its own here) and one ``logp_mix``, and
    nothing else: the difference of the two runs is held to that sum, by kernel for the library's own and in total for every device
    kernel torch's profiler saw.  So whatever the alpha = 0 run issues besides is what it issued without the feature."""
    from gnnlm_amd import eval_lm, ops
    from gnnlm_amd.adaptive_softmax import AdaptiveSoftmax
    from test_ragged_gpu import count_launches, make_ragged_dir
    c = make_ragged_dir(tmp_path, SENT_SIZES, L=1)
    common = c["base"] + ["--sample-break-mode", "none", "--tokens-per-sample", str(T_BLOCK), "--max-tokens", str(T_BLOCK), "--gcn-context-window", "0",
                          "--batch-blocks", "0"] + knn_args(c, 0.25)
    n_batches = -(-c["n_test"] // T_BLOCK)                          # one block per batch: 7, the last one short
    softmax_calls, mix_calls = [], []
    real_softmax, real_mix = AdaptiveSoftmax.target_log_prob, ops.logp_mix

    def softmax(self, x, target, *a, **kw):
        softmax_calls.append((self, x, target, a, kw))
        return real_softmax(self, x, target, *a, **kw)

    def mix(gnn, base, alphas, *a, **kw):
        mix_calls.append(list(alphas))
        return real_mix(gnn, base, alphas, *a, **kw)

    monkeypatch.setattr(AdaptiveSoftmax, "target_log_prob", softmax)
    monkeypatch.setattr(ops, "logp_mix", mix)
    counts, calls = {}, {}
    for name, args in (("zero", common), ("off", with_overrides(common, "{'orig_prob_ratio': -0.1}")), ("none", with_overrides(common, "{}")),
                       ("ratio", with_overrides(common, "{'orig_prob_ratio': 0.3}"))):
        eval_lm.cli_main(args)                                      # warm-up: one-time allocations and table builds
        del softmax_calls[:], mix_calls[:]
        counts[name] = count_launches(lambda: eval_lm.cli_main(args))
        calls[name] = ([(s_, x.clone(), t.clone(), a, kw) for s_, x, t, a, kw in softmax_calls], list(mix_calls))
        print(name, counts[name], len(calls[name][0]), "softmax calls,", len(calls[name][1]), "mixes")
    # without a ratio: one softmax call per batch, no mix, in every spelling of "off"
    for name in ("zero", "off", "none"):
        assert len(calls[name][0]) == n_batches and calls[name][1] == [], name
        assert counts[name] == counts["zero"], name
    # with a ratio: the GNN branch's call as before, then the base branch's, then one mix at the run's ratio -- per batch
    ratio_calls, ratio_mixes = calls["ratio"]
    assert len(ratio_calls) == 2 * n_batches and ratio_mixes == [[0.3]] * n_batches
    for (_, x0, t0, _, _), (_, x3, t3, _, _) in zip(calls["zero"][0], ratio_calls[0::2]):
        assert torch.equal(x0, x3) and torch.equal(t0, t3)          # the even calls ARE the alpha = 0 run's
    # the base branch's calls, each on its own (same object, same rows, same targets)
    monkeypatch.undo()
    lib_extra, dev_extra = {}, 0
    for self_, x, t, a, kw in ratio_calls[1::2]:
        real_softmax(self_, x, t, *a, **kw)
        lib1, dev1 = count_launches(lambda: real_softmax(self_, x, t, *a, **kw))
        assert dev1 > 0 and set(k_ for k_, v in lib1.items() if v) <= {"gemm_nt_f32_kernel", "row_lse_pick_kernel"}, lib1
        dev_extra += dev1
        for k_, v in lib1.items():
            lib_extra[k_] = lib_extra.get(k_, 0) + v
    g = torch.zeros(T_BLOCK, device=dev)
    lib_mix, dev_mix = count_launches(lambda: real_mix(g, g, [0.3]))
    assert dev_mix == 1 and {k_: v for k_, v in lib_mix.items() if v} == {"misc": 1}       # one launch, in the library's own count as "misc"
    lib0, lib3 = counts["zero"][0], counts["ratio"][0]
    print("base branch alone:", lib_extra, dev_extra, "mix alone:", dev_mix)
    assert counts["ratio"][1] - counts["zero"][1] == dev_extra + n_batches * dev_mix
    for name in set(lib0) | set(lib3):                              # the HGT's, the search's and the interpolation's as often as before
        assert lib3.get(name, 0) - lib0.get(name, 0) == lib_extra.get(name, 0) + (n_batches if name == "misc" else 0), name
