"""Host side of ``orig_prob_ratio`` > 0 (the base-LM / GNN mixture of transformer.py:987-1005,1056-1077): the C ABI's two new
entries, the driver's ``--sweep-orig-prob-ratio``, the model's argument checks, and the fixture against the oracle.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "orig_ratio.npz")
BASE = ["DATA", "--path", "CKPT", "--graph", "--use-precompute-feat"]
KNN = ["--knnlm", "--k", "8", "--lmbda", "0.25", "--temperature", "0.5"]


def parse(extra):
    from gnnlm_amd import eval_lm
    return eval_lm.parse_sweep(eval_lm.get_parser().parse_args(BASE + extra))


def test_header_and_library_export_the_new_entries():
    from gnnlm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gnnlm.h")).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", hdr) and _lib.ABI_VERSION == 12        # additions only
    syms = _lib.exported_symbols()
    assert "gnnlm_logp_mix" in syms and "gnnlm_knn_interp_grid_lm" in syms
    L = _lib.lib()
    assert L.gnnlm_abi_version() == 12
    assert hasattr(L, "gnnlm_logp_mix") and hasattr(L, "gnnlm_knn_interp_grid_lm")
    # each declaration cites the reference lines it replaces
    for name in ("gnnlm_logp_mix", "gnnlm_knn_interp_grid_lm"):
        comment = hdr[:hdr.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "transformer.py:1056-1062" in comment and "Replaces" in comment, name


def test_invalid_arguments_are_refused_on_the_host_side_of_the_library():
    """alpha outside [0, 1], A outside 1 .. 8, n_lm outside 1 .. 8: GNNLM_E_INVALID before anything is launched (no device needed:
    the pointers are never touched)."""
    import ctypes
    from gnnlm_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)                                        # (never dereferenced)
    for alphas in ([-0.1], [1.5], [float("nan")], [], [0.1] * 9):
        arr = (ctypes.c_double * max(1, len(alphas)))(*alphas)
        assert L.gnnlm_logp_mix(one, one, 4, arr, len(alphas), one, None) != 0, alphas
    d = _lib.gnnlm_knn_interp_grid_t()
    for n_lm in (0, 9, -1):
        assert L.gnnlm_knn_interp_grid_lm(ctypes.byref(d), n_lm, 0, None) != 0
        assert b"lm rows" in L.gnnlm_last_error()


def test_parse_sweep_with_the_ratio_axis():
    # alone: accepted without --knnlm
    assert parse(["--sweep-orig-prob-ratio", "0,0.3, 0.6,1"]) == (None, None, None, [0.0, 0.3, 0.6, 1.0])
    # with --knnlm: the outer axis of the grid; a list not given is the run's own value
    assert parse(KNN + ["--sweep-orig-prob-ratio", "0.3"]) == ([8], [0.5], [0.25], [0.3])
    assert parse(KNN + ["--sweep-orig-prob-ratio", "0,0.5", "--sweep-lmbda", "0,0.1", "--sweep-k", "4,8"]) == \
        ([4, 8], [0.5], [0.0, 0.1], [0.0, 0.5])
    # without the flag: exactly as before
    assert parse(KNN + ["--sweep-lmbda", "0,0.1"]) == ([8], [0.5], [0.0, 0.1]) and parse(KNN) is None and parse([]) is None


@pytest.mark.parametrize("extra, msg", [
    (["--sweep-orig-prob-ratio", ",".join(str(j / 16) for j in range(9))], "at most 8"),
    (["--sweep-orig-prob-ratio", "0.1,0.1"], "repeated"),
    (["--sweep-orig-prob-ratio", "1.5"], "0 .. 1"),
    (["--sweep-orig-prob-ratio", "-0.1"], "0 .. 1"),
    (["--sweep-orig-prob-ratio", "nan"], "0 .. 1"),
    (["--sweep-orig-prob-ratio", "0.1,x"], "comma-separated"),
    (["--sweep-orig-prob-ratio", ""], "comma-separated"),
    (["--sweep-orig-prob-ratio", "0.1", "--sweep-lmbda", "0.1"], "need --knnlm"),
    (["--save-knnlm-dstore", "--dstore-mmap", "X", "--sweep-orig-prob-ratio", "0.1"], "--save-knnlm-dstore"),
    (["--knnlm", "--k", "2048", "--sweep-orig-prob-ratio", "0.1"], "1024"),
])
def test_ratio_axis_refused_before_any_device_work(extra, msg):
    with pytest.raises(ValueError, match=msg):
        parse(extra)


def test_grid_points_and_lines_with_the_ratio_axis():
    from gnnlm_amd import eval_lm, ops
    sweep = ([4, 8], [1.0], [0.0, 0.25], [0.0, 0.3, 1.0])
    pts = ops.grid_points(*sweep)
    assert pts == [(a, k, t, l) for a in sweep[3] for k in sweep[0] for t in sweep[1] for l in sweep[2]]      # alpha slowest, lmbda fastest
    assert ops.grid_points(*sweep[:3]) == [p[1:] for p in pts[:4]]                                            # 3-tuples as before
    assert ops.grid_points(None, None, None, [0.0, 0.5]) == [(0.0,), (0.5,)]
    rows = eval_lm.sweep_table(sweep, [-(100.0 + g) for g in range(12)], 41)
    assert [(r["orig_prob_ratio"], r["k"], r["temperature"], r["lmbda"]) for r in rows] == pts
    lines = eval_lm.sweep_lines(rows)
    loss = 100.0 / 41 / math.log(2)
    assert lines[0] == "sweep orig_prob_ratio=0 k=4 temperature=1 lmbda=0 loss={:.4f} ppl={:.2f}  <- best".format(loss, 2 ** loss)
    loss = 105.0 / 41 / math.log(2)
    assert lines[5] == "sweep orig_prob_ratio=0.3 k=4 temperature=1 lmbda=0.25 loss={:.4f} ppl={:.2f}".format(loss, 2 ** loss)
    # the ratio alone
    rows = eval_lm.sweep_table((None, None, None, [0.0, 0.3]), [-100.0, -90.0], 41)
    assert [set(r) for r in rows] == [{"orig_prob_ratio", "score_sum", "loss", "ppl"}] * 2
    loss = 90.0 / 41 / math.log(2)
    assert eval_lm.sweep_lines(rows)[1] == "sweep orig_prob_ratio=0.3 loss={:.4f} ppl={:.2f}  <- best".format(loss, 2 ** loss)
    # without the axis: no such key, the lines as they were
    rows = eval_lm.sweep_table(sweep[:3], [-(100.0 + g) for g in range(4)], 41)
    assert all("orig_prob_ratio" not in r for r in rows)
    assert eval_lm.sweep_lines(rows)[1].startswith("sweep k=4 temperature=1 lmbda=0.25 loss=")


def test_model_accepts_a_ratio_below_one():
    from gnnlm_amd.model import GnnLmModel
    m = GnnLmModel(None, None, None, orig_prob_ratio=0.3)
    assert m.orig_prob_ratio == 0.3
    for bad in (1.0, 1.5):
        with pytest.raises(ValueError, match="math domain error"):          # the reference's math.log(1 - p1_coeff)
            GnnLmModel(None, None, None, orig_prob_ratio=bad)
    assert GnnLmModel(None, None, None, orig_prob_ratio=-0.1).orig_prob_ratio == 0.0           # `> 0` is the reference's test: off
    assert GnnLmModel(None, None, None).orig_prob_ratio == 0.0


def test_engine_signature():
    import inspect
    from gnnlm_amd.engine import GnnLmEngine
    for fn in (GnnLmEngine.score, GnnLmEngine.score_begin):
        p = inspect.signature(fn).parameters["orig_prob_ratio"]
        assert p.default == 0.0


def golden_weights(g, dtype):
    cut = [int(c) for c in g["cutoff"]]
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    return {"cutoff": cut, "emb": [t(g[f"emb{i}"]) for i in range(len(cut))],
            "proj": [None] + [t(g[f"proj{i}"]) for i in range(1, len(cut))], "class_proj": t(g["class_proj"])}


def test_fixture_equals_the_oracle_mixture():
    """Each ``mixed.{alpha}`` the reference returned == float64 logaddexp of the (unchanged) oracle's log-probs of x and of h."""
    from oracle import adaptive_softmax as oasm
    g = np.load(GOLDEN)
    w = golden_weights(g, torch.float64)
    tgt = torch.from_numpy(g["target"]).reshape(-1)
    cut = w["cutoff"]
    assert all(((tgt >= lo) & (tgt < hi)).any() for lo, hi in zip([0] + cut[:-1], cut))                  # every band
    d = g["x"].shape[-1]
    gnn = oasm.target_log_prob(torch.from_numpy(g["x"]).double().reshape(-1, d), tgt, w).numpy()
    base = oasm.target_log_prob(torch.from_numpy(g["h"]).double().reshape(-1, d), tgt, w).numpy()
    assert np.abs(gnn - base).max() > 1.0                                                               # the two branches do differ
    assert [float(a) for a in g["alphas"]] == [0.1, 0.3, 0.5, 0.9]
    for a in g["alphas"]:
        want = np.logaddexp(math.log(a) + base, math.log(1 - a) + gnn)
        err = np.abs(g[f"mixed.{a}"].reshape(-1) - want).max()
        print(f"alpha {a}: max |fixture - oracle| = {err:.2e}")
        assert err < 2e-5
    assert str(g["alpha_1_raises"]) == "math domain error"
