"""The restatement of the base transformer LM (tests/transformer_lm_ref.py) against what the reference computed
(tests/golden/transformer_lm.npz, made by tests/golden/make_transformer_lm.py), and the conditions that make the GPU test's bar
meaningful -- all without a GPU.

Float32 error of the restatement's formulas on the GPU test's own cases, max|f32 - f64| / max|f64| over out, last_inner and
last_ffn_input (computed below, bar FEATURE_BAR / 4 = 1.25e-5): case 1 2.4e-7, case 2 2.7e-7, case 3 3.8e-7.
With float16-rounded GEMM operands on both sides the two evaluations differ by 1.7e-4 (case 1): see
test_float16_operand_rounding_is_reproducible_in_float32 for what that means for the precision-3 bar.
"""
import os
import re

import numpy as np
import pytest
import torch

import transformer_lm_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_SHARE = 0.25                # float32 itself must stay within this share of the feature bar


@pytest.mark.parametrize("name,H,act", [("relu_sin_adaptive", 4, "relu"), ("gelu_learned_norms", 2, "gelu")])
def test_restatement_reproduces_the_reference(golden, name, H, act):
    g = golden("transformer_lm")
    m = tr.golden_model(g, name, H, act, 8.0)                      # sqrt(64)
    tokens = g[f"{name}.tokens"]
    bsz, T = tokens.shape
    f = tr.forward(m, tokens.reshape(-1), np.arange(bsz + 1) * T)
    for key, gk in (("out", "x"), ("last_inner", "last_inner"), ("last_ffn_input", "last_ffn_input")):
        if f"{name}.{gk}" not in g:
            continue
        want = g[f"{name}.{gk}"].reshape(bsz * T, -1).astype(np.float64)
        err = np.abs(f[key] - want)
        print(f"{name}.{key}: max |restatement - reference| = {err.max():.3e} (max |reference| = {np.abs(want).max():.3f})")
        assert (err <= 1e-5 + 1e-6 * np.abs(want)).all(), float(err.max())       # the bar of the sibling *_ref_cpu tests for float32 outputs


def test_adaptive_input_and_positions_match_the_reference(golden):
    g = golden("transformer_lm")
    bands = [(g[f"relu_sin_adaptive.band{b}.emb"], g[f"relu_sin_adaptive.band{b}.proj"]) for b in range(3)]
    rows = g["relu_sin_adaptive.embed_rows"].astype(np.float64)
    assert np.abs(tr.adaptive_table(bands) - rows).max() <= 1e-6
    T = g["relu_sin_adaptive.tokens"].shape[1]
    # the sinusoidal rows pad + 1 .. pad + T, bit for bit; the restatement's table and the product's builder
    assert np.array_equal(tr.sinusoidal_table(tr.PAD + 1 + T, 64)[tr.PAD + 1:], g["relu_sin_adaptive.pos_rows"])
    from gnnlm_amd.transformer_lm import sinusoidal_table
    assert np.array_equal(sinusoidal_table(tr.PAD + 1 + T, 64).numpy()[tr.PAD + 1:], g["relu_sin_adaptive.pos_rows"])
    assert np.array_equal(sinusoidal_table(200, 64).numpy()[:50], sinusoidal_table(50, 64).numpy())     # a longer table extends a shorter
    T = g["gelu_learned_norms.tokens"].shape[1]
    assert np.array_equal(g["gelu_learned_norms.P"][tr.PAD + 1:tr.PAD + 1 + T], g["gelu_learned_norms.pos_rows"])


@pytest.mark.parametrize("name", ["none", "complete", "wide"])
def test_context_windows_match_the_reference_collater(golden, name):
    g = golden("transformer_lm")
    tps, w = (int(v) for v in g[f"ctx.{name}.cfg"])
    lengths = g[f"ctx.{name}.lengths"]
    want = g[f"ctx.{name}.start_indices"]
    assert tr.context_windows(lengths, tps - w, w) == want.tolist()
    from gnnlm_amd.eval_base_lm import context_lengths, shifted_source
    assert context_lengths(lengths, tps - w, w).tolist() == want.tolist()
    # the rows: context + sample tokens, the context being the source tokens right in front of the sample (ids 99 + position)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    assert np.array_equal(g[f"ctx.{name}.row_len"], want + lengths)
    assert np.array_equal(g[f"ctx.{name}.first_src"], 99 + starts - want)
    assert want.max() > 0 and (name == "none" or (want[1:] < w).any())
    src = shifted_source(np.array([5, 6, 7, 8]))
    assert src.tolist() == [2, 5, 6, 7] == tr.shifted_source([5, 6, 7, 8]).tolist()


@pytest.mark.parametrize("case", sorted(tr.GPU_CASES))
def test_float32_stays_within_a_quarter_of_the_feature_bar(case):
    """What makes the GPU bar (FEATURE_BAR against the float64 restatement) meaningful: a float32 evaluation of the same formulas on
    the same cases uses at most a quarter of it."""
    m, tokens, off = tr.gpu_case(case)
    ref = tr.gpu_case_ref(case)
    f32 = tr.forward(m, tokens, off, torch.float32)
    for key in ("out", "last_inner", "last_ffn_input"):
        e = tr.rel_err(f32[key], ref[key])
        print(f"case {case} {key}: max|f32 - f64| / max|f64| = {e:.3e}")
        assert e <= F32_SHARE * tr.FEATURE_BAR


def test_float16_operand_rounding_is_reproducible_in_float32():
    """Under --fp16 a float32 and a float64 evaluation round nearly every GEMM operand to the same float16 value; the few activations
    that fall on the other side of a rounding boundary move the result by a float16 ulp of one product, which is far above the
    float32 noise -- so the feature bar cannot hold against the operand-rounded restatement (measured here: 1.7e-4 of max|ref|
    for float32 arithmetic itself).  The GPU test's precision-3 bar is therefore relative to the EFFECT of the rounding: the distance
    to the operand-rounded float64 restatement, RMS, is at most FP16_SHARE of the distance between that restatement and the
    un-rounded one (an evaluation that rounds nothing sits at 1.0).  Float32 arithmetic on the CPU sits at 0.20 / 0.20 / 0.12."""
    m, tokens, off = tr.gpu_case(1)
    ref, ref64 = tr.gpu_case_ref(1, half_gemm=True), tr.gpu_case_ref(1)
    f32 = tr.forward(m, tokens, off, torch.float32, half_gemm=True)
    for key in ("out", "last_inner", "last_ffn_input"):
        share = tr.rms(f32[key] - ref[key]) / tr.rms(ref64[key] - ref[key])
        print(f"case 1 fp16 operands {key}: rms(f32 - f64) / rms(effect of the rounding) = {share:.3f}; max rel {tr.rel_err(f32[key], ref[key]):.3e}")
        assert share <= tr.FP16_SHARE
    assert tr.rel_err(ref["out"], ref64["out"]) > 1e-4                       # the rounding is really applied


def test_header_is_abi_12_and_declares_the_new_entries():
    text = open(os.path.join(ROOT, "include", "gnnlm.h")).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", text)
    from gnnlm_amd import _lib
    syms = _lib.exported_symbols()
    for s in ("gnnlm_lm_embed", "gnnlm_relu", "gnnlm_transformer_lm_forward", "gnnlm_transformer_lm_workspace_bytes"):
        assert s in syms, s
    for st in ("gnnlm_lm_embed_t", "gnnlm_tlm_layer_t", "gnnlm_tlm_t", "gnnlm_tlm_io_t"):
        assert st in _lib.STRUCTS, st
    assert dict(_lib.STRUCTS["gnnlm_tlm_io_t"]._fields_)["blocks"] is _lib.STRUCTS["gnnlm_ragged_t"]
