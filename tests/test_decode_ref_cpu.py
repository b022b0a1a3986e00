"""The restatements of tests/decode_ref.py held to the ones the suite already trusts (no GPU): the incremental model to
transformer_lm_ref.forward, decode_attn_ref to causal_ref, sample_ref to its definition, and the greedy chains of the generation
test to a top-1 / top-2 gap that float32 cannot flip."""
import numpy as np
import pytest

import causal_ref as cr
import decode_ref as dr
import transformer_lm_ref as tr


def test_header_declares_what_the_restatements_restate():
    """The entries these references stand for exist in include/gnnlm.h and in the library, with mirrors of the C sizes, and the chunk
    the length cases of tests/test_decode_attn_abi_gpu.py are laid around is a whole number of the 64-key passes a wave makes at d_k = 16 (fewer keys per pass at wider heads)."""
    import ctypes
    import re
    from gnnlm_amd import _lib
    L = _lib.lib()
    for name in ("gnnlm_kv_cache_t", "gnnlm_decode_attn_t", "gnnlm_tlm_step_io_t", "gnnlm_sample_topk_t"):
        assert L.gnnlm_sizeof(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0, name
    for name in ("gnnlm_decode_attn", "gnnlm_decode_attn_workspace_bytes", "gnnlm_transformer_lm_prefill", "gnnlm_transformer_lm_step",
                 "gnnlm_transformer_lm_step_workspace_bytes", "gnnlm_sample_topk"):
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    chunk = int(re.search(r"#define\s+GNNLM_DECODE_CHUNK\s+(\d+)", open(_lib.HEADER).read()).group(1))
    assert chunk >= 64 and chunk % 64 == 0
    assert L.gnnlm_decode_attn_workspace_bytes(3, 2, 32, 2 * chunk + 1) == 3 * 2 * 3 * (32 + 4) * 4
    assert L.gnnlm_abi_version() == 12


@pytest.mark.parametrize("case", [1, 2])
def test_incremental_equals_forward(case):
    m, tokens, off = tr.gpu_case(case)
    ref = tr.gpu_case_ref(case)
    for b in range(len(off) - 1):
        s, e = int(off[b]), int(off[b + 1])
        got = dr.incremental_rows(m, tokens[s:e])
        for key in ("out", "last_inner", "last_ffn_input"):
            err = float(np.abs(got[key] - ref[key][s:e]).max())
            assert err <= 1e-12, (case, b, key, err)


@pytest.mark.parametrize("H,dk,n", [(1, 16, 0), (3, 32, 1), (2, 64, 33), (2, 128, 130)])
def test_decode_attn_ref_is_the_last_causal_row(H, dk, n):
    rs = np.random.RandomState(11 + n)
    d = H * dk
    Q, K, V = (rs.randn(n + 1, d) for _ in range(3))
    want = cr.causal_ref(Q, K, V, [n + 1], H, 0)[-1]
    cache_k = np.full((1, n + 3, d), np.nan)
    cache_v = np.full((1, n + 3, d), np.nan)
    cache_k[0, :n], cache_v[0, :n] = K[:n], V[:n]
    got, appended, n_bad = dr.decode_attn_ref(Q[-1:], K[-1:], V[-1:], cache_k, cache_v, [n], H)
    assert appended == [0] and n_bad == 0
    assert float(np.abs(got[0] - want).max()) <= 1e-12
    # done, and the two ends outside the range
    got, appended, n_bad = dr.decode_attn_ref(np.repeat(Q[-1:], 3, 0), np.repeat(K[-1:], 3, 0), np.repeat(V[-1:], 3, 0),
                                              np.repeat(cache_k, 3, 0), np.repeat(cache_v, 3, 0), [n, n + 3, -1], H, done=[1, 0, 0])
    assert appended == [] and n_bad == 2 and not got.any()


def test_adaptive_dense_logp_is_adaptive_logp_of_every_target():
    m, hw = dr.gen_model(301, "adaptive")
    x = np.random.RandomState(3).randn(dr.GEN_MODEL["d"])
    V = dr.GEN_MODEL["V"]
    want = tr.adaptive_logp(np.repeat(x[None], V, 0), np.arange(V), **hw)
    got = dr.adaptive_dense_logp(x, **hw)
    assert np.abs(got - want).max() <= 1e-12 and abs(np.exp(got).sum() - 1) <= 1e-12


def test_sample_ref():
    logp = np.log(np.array([[0.5, 0.25, 0.125, 0.125], [0.5, 0.25, 0.25, 0.0]]))
    ids = np.array([[7, 2, 9, 4], [5, 6, 2, 8]])
    nxt, col, done, n_bad = dr.sample_ref(logp, ids, None)
    assert nxt.tolist() == [7, 5] and col.tolist() == [0, 0] and done.tolist() == [0, 0] and n_bad == 0
    nxt, col, done, n_bad = dr.sample_ref(logp, ids, np.array([0.6, 0.99]))
    assert col.tolist() == [1, 2] and nxt.tolist() == [2, 2] and done.tolist() == [1, 1]       # eos picked; the -inf tail never is
    nxt, col, done, n_bad = dr.sample_ref(logp, ids, np.array([0.0, 0.0]), done=[0, 1])
    assert col.tolist() == [0, -1] and nxt.tolist() == [7, dr.PAD]
    bad = np.array([[-np.inf, -np.inf]])
    nxt, col, done, n_bad = dr.sample_ref(bad, np.array([[-1, -1]]), np.array([0.5]))
    assert nxt.tolist() == [dr.PAD] and done.tolist() == [1] and n_bad == 1


@pytest.mark.parametrize("head", dr.GEN_HEADS)
@pytest.mark.parametrize("seed", dr.GEN_SEEDS)
def test_greedy_chains_have_a_gap(seed, head):
    """The generation test compares tokens exactly: every step's top-1 must lead top-2 by far more than float32 evaluation moves a
    log-prob (2e-5, the README's bar)."""
    for i in range(len(dr.GEN_PROMPT_LENS)):
        toks, lps, gaps, _ = dr.gen_chain(seed, i, head)
        print(f"seed {seed} {head} prompt {i}: {len(toks)} tokens, minimum top-1 / top-2 gap {gaps.min():.3e}")
        assert gaps.min() >= 1e-3
        assert len(toks) == dr.GEN_NEW or toks[-1] == dr.EOS
