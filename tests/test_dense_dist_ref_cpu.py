"""tests/dense_dist_ref.py (the float64 restatement the GPU tests hold the dense kernels to) pinned to the reference's own dense
outputs, and the CPU-visible surface of the feature: header, struct mirror, ABI version, eval_lm's flags and refusals.  CPU only.

The fixtures were written by running the reference (tests/golden/make_golden.py): ``adaptive_softmax.npz['dense']`` is
``AdaptiveSoftmax.get_log_prob(x, None)``, the sixteen ``knn.npz['*.dense']`` are ``KNNModel.get_knn_prob(targets=None)``,
``combine.npz`` is ``combine_knn_and_vocab_probs``."""
import re

import numpy as np
import pytest

import dense_dist_ref as R

KNN_TAGS = [f"{m}.{c}.t{t}" for m in ("do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2") for c in ("raw", "cos") for t in ("1.0", "0.01")]


def asm_weights(g):
    return {"cutoff": [int(c) for c in g["cutoff"]], "emb": [g[f"emb{i}"] for i in range(3)], "proj": [None, g["proj1"], g["proj2"]],
            "class_proj": g["class_proj"]}


def test_adaptive_restatement_matches_the_reference_dense(golden):
    g = golden("adaptive_softmax")
    x = g["x"].reshape(-1, g["x"].shape[-1])
    dense = R.adaptive_log_probs(x, asm_weights(g))
    np.testing.assert_allclose(dense, g["dense"].reshape(x.shape[0], -1), atol=2e-6, rtol=1e-5)     # test_oracle_golden.py's bar for it
    np.testing.assert_allclose(np.exp(dense).sum(1), 1.0, atol=1e-12)
    t = g["target"].reshape(-1)
    np.testing.assert_allclose(dense[np.arange(len(t)), t], g["target_logp"].reshape(-1), atol=2e-6, rtol=1e-5)


def test_adaptive_restatement_matches_the_oracle(golden):
    import torch
    from oracle import adaptive_softmax as oas
    x, w, _, _ = R.head_inputs(33)
    tw = {"cutoff": w["cutoff"], "emb": [torch.from_numpy(e).double() for e in w["emb"]],
          "proj": [None if p is None else torch.from_numpy(p).double() for p in w["proj"]], "class_proj": torch.from_numpy(w["class_proj"]).double()}
    np.testing.assert_allclose(R.adaptive_log_probs(x, w), oas.dense_log_prob(torch.from_numpy(x).double(), tw).numpy(), atol=1e-12)


def test_plain_restatement_matches_the_reference_targets(golden):
    """dense_head.npz holds the reference's gathered column for every head flavour at ratio 0: the restatement's target column."""
    g = golden("dense_head")
    x, t = g["x"].reshape(-1, g["x"].shape[-1]), g["target"].reshape(-1)
    for share, wkey in (("shared", "embed_tokens"), ("unshared", "embed_out")):
        for bias in (None, g["xl_bias"]):
            dense = R.plain_log_probs(x, g[wkey], bias)
            ref = g[f"logp.{share}.{'nobias' if bias is None else 'bias'}.0.0"].reshape(-1)
            np.testing.assert_allclose(dense[np.arange(len(t)), t], ref, atol=2e-6, rtol=1e-5)


@pytest.mark.parametrize("tag", KNN_TAGS)
def test_knn_restatement_matches_the_reference_dense(golden, tag):
    g = golden("knn")
    t = float(tag.rsplit(".t", 1)[1])
    ids = g[tag + ".ids"]
    labels = R.neighbour_labels(ids, g["vals"])
    assert np.array_equal(labels, g["vals"][ids].astype(np.int64))                                 # numpy's own wrap of -1
    p = R.knn_probs(g[tag + ".sims"], ids, labels, t, 50)
    np.testing.assert_allclose(p, g[tag + ".dense"], rtol=2e-5, atol=1e-7)                         # test_oracle_golden.py's bar for `p`
    np.testing.assert_allclose(p[np.arange(len(ids)), g["targets"]], g[tag + ".p"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-12)


def test_mix_restatement_matches_the_reference_combine(golden):
    g = golden("combine")
    for lm in (0.1, 0.15, 0.2, 0.25):
        np.testing.assert_allclose(R.mix(g["lm_logp"], g["p_knn"], lm), g[f"mix.{lm}"], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(R.mix_f32(g["lm_logp"], g["p_knn"], lm), g[f"mix.{lm}"], rtol=1e-6, atol=1e-6)


def test_topn_and_rank_restatement():
    v, t = R.rank_case()
    ids, vals = R.topn(v, 8)
    rk = R.rank(v, t)
    for r in range(v.shape[0]):
        order = sorted((c for c in range(v.shape[1]) if R.present(v[r, c])), key=lambda c: (-float(v[r, c]), c))
        assert list(ids[r][:len(order[:8])]) == order[:8]
        if 0 <= t[r] < v.shape[1]:
            assert rk[r] == (order.index(int(t[r])) if int(t[r]) in order else len(order))
        else:
            assert rk[r] == -1
    assert rk[7] == 1 and rk[2] == v.shape[1] // 2 and rk[3] == R.present(v[3]).sum()
    # the rank is the target's position in the full list: inside the top-N iff rank < N
    full, _ = R.topn(v, v.shape[1])
    for r in range(v.shape[0]):
        if rk[r] >= 0 and R.present(v[r, t[r]]):
            assert full[r, rk[r]] == t[r]


@pytest.mark.parametrize("pattern", R.MIX_PATTERNS)
@pytest.mark.parametrize("k", R.MIX_KS)
def test_float32_evaluation_of_the_mix_stays_within_1e_5(k, pattern):
    """The GPU test's inputs (|sims| <= 2): a plain float32 numpy evaluation of the formula is within 1e-5 of the float64
    restatement -- so the 2e-5 the kernel is held to is not eaten by the arithmetic the formula itself prescribes."""
    worst = 0.0
    for si, (t, lmbda) in enumerate((t, l) for t in R.MIX_TS for l in R.MIX_LMBDAS):
        case = R.mix_case(k, pattern, seed=100 * k + si)
        assert np.abs(case["sims"]).max() <= 2.0
        p64, out64 = R.mix_expected(case, t, lmbda)
        p32, out32 = R.mix_float32(case, t, lmbda)
        worst = max(worst, float(np.abs(out32 - out64).max()))
        if pattern == "equal":
            assert np.allclose(p64[:, 7], 1.0) and (np.delete(p64, 7, axis=1) == 0).all()
        if pattern == "distinct":
            assert ((p64 > 0).sum(1) == k).all()
        if pattern == "outside":
            assert (p64[1] == 0).all() and p64.sum(1).max() <= 1 + 1e-12
    print(f"k={k} {pattern}: max |float32 - float64| = {worst:.2e}")
    assert worst < 1e-5


# ---------------------------------------------------------------------------------------------------- header, mirror, ABI
def test_header_declares_the_entry_points_and_abi_stays_12():
    from gnnlm_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for fn in ("gnnlm_adaptive_log_probs", "gnnlm_dense_log_probs", "gnnlm_knn_mix_dense", "gnnlm_row_rank",
               "gnnlm_adaptive_log_probs_workspace_bytes"):
        assert re.search(r"\b(int|size_t)\s+" + fn + r"\s*\(", text), fn
        assert fn in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 12 and re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", text)


def test_lib_mirrors_the_mix_descriptor():
    import ctypes
    from gnnlm_amd import _lib
    st = _lib.STRUCTS["gnnlm_knn_mix_dense_t"]
    names = [f[0] for f in st._fields_]
    assert names == ["lm_logp", "ld_lm", "sims", "ids", "vals", "vals_itemsize", "n_store", "row0", "n_local", "knn_vals", "n", "k", "V",
                     "temperature", "lmbda", "out", "ldo", "out_pknn", "ld_pknn"]
    kinds = dict(st._fields_)
    assert kinds["lmbda"] is ctypes.c_double and kinds["temperature"] is ctypes.c_float and kinds["V"] is ctypes.c_int32
    assert kinds["n"] is ctypes.c_int64 and kinds["out"] is ctypes.c_void_p and kinds["ldo"] is ctypes.c_int64
    assert _lib.lib().gnnlm_sizeof(b"gnnlm_knn_mix_dense_t") == ctypes.sizeof(st)
    # additions only: the descriptors the new entries share with the target-column calls are unchanged
    assert ctypes.sizeof(_lib.STRUCTS["gnnlm_knn_interp_t"]) == 152 and ctypes.sizeof(_lib.STRUCTS["gnnlm_dense_softmax_t"]) == 40


# ---------------------------------------------------------------------------------------------------- eval_lm's flags
def _args(*extra):
    from gnnlm_amd import eval_lm
    return eval_lm.get_parser().parse_args(["DATA", "--path", "ckpt.pt", *extra])


def test_eval_lm_parser_accepts_the_flags():
    a = _args("--output-topk", "5", "--topk-out", "f")
    assert a.output_topk == 5 and a.topk_out == "f"
    assert _args().output_topk == 0 and _args().topk_out is None
    from gnnlm_amd import eval_lm
    assert eval_lm.check_output_topk(a, world=1) == 5
    assert eval_lm.check_output_topk(_args(), world=4) == 0                # off: nothing to refuse
    assert eval_lm.check_output_topk(_args("--output-topk", "2048"), world=1) == 2048


@pytest.mark.parametrize("extra,world,word", [
    (("--sweep-lmbda", "0.1,0.2", "--knnlm"), 1, "--sweep"),
    (("--sweep-temperature", "1,0.1", "--knnlm"), 1, "--sweep"),
    (("--sweep-k", "4,8", "--knnlm"), 1, "--sweep"),
    (("--sweep-orig-prob-ratio", "0,0.3"), 1, "--sweep"),
    (("--save-knnlm-dstore", "--dstore-mmap", "x"), 1, "--save-knnlm-dstore"),
    (("--graph-capture",), 1, "--graph-capture"),
    ((), 2, "one process"),
])
def test_eval_lm_refuses_what_topk_cannot_be_combined_with(extra, world, word):
    from gnnlm_amd import eval_lm
    with pytest.raises(ValueError, match=word):
        eval_lm.check_output_topk(_args("--output-topk", "5", *extra), world=world)


def test_eval_lm_refuses_topk_out_of_range(monkeypatch):
    from gnnlm_amd import eval_lm
    for n in ("2049", "-1"):
        with pytest.raises(ValueError, match="2048"):
            eval_lm.check_output_topk(_args("--output-topk", n), world=1)
    with pytest.raises(ValueError, match="--output-topk"):
        eval_lm.check_output_topk(_args("--topk-out", "f"), world=1)
    monkeypatch.setenv("WORLD_SIZE", "2")                                  # the count of processes is read from the launcher's variable
    with pytest.raises(ValueError, match="one process"):
        eval_lm.check_output_topk(_args("--output-topk", "5"))


def test_predict_helpers_refuse_bad_topk():
    from gnnlm_amd import predict
    for bad in (0, -3, 2049, 2.0, True):
        with pytest.raises(ValueError):
            predict.check_topk(bad)
    with pytest.raises(ValueError):
        predict.check_topk(30, V=24)
    assert predict.chunk_rows(267744) == (256 << 20) // (4 * 267744) and predict.chunk_rows(10, chunk_bytes=1) == 1
    assert predict.topk_stats(np.array([0, 4, 5, -1]), 5) == (0.25, 0.5, (1 + 1 / 5 + 1 / 6) / 4)
    assert predict.topk_stats(np.zeros(0), 5) == (0.0, 0.0, 0.0)
