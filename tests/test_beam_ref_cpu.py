"""The beam-search restatements against the reference's own results and against their definition (no GPU):

  * beam_search_ref over the toy model of tests/golden/beam_search.npz reproduces every hypothesis the reference's SequenceGenerator
    returned there (tests/golden/make_beam_search.py): tokens and order exact, scores and positional scores within 1e-5 (the
    reference computes them in float32);
  * select_ref on hand-made ties follows the order rule of gnnlm_beam_select;
  * the seeds the GPU end-to-end test uses keep its margin under float64;
  * the header's new structs and entry points are registered.
"""
import json
import os

import numpy as np
import pytest

import beam_ref as br

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_search.npz")
CASES = ["beam1", "beam3_lenpen", "beam5", "beam5_unnormalized_unkpen", "beam3_min_len", "beam5_forced_eos", "beam3_early"]
BAR = 1e-5


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    z = np.load(GOLDEN)
    g = lambda k: z[f"{name}/{k}"]
    s = json.loads(str(g("settings")))
    prompts, P = g("prompts"), g("prompts").shape[1]
    # the stored hypotheses hold the prompt's positions: its cumulative log-probability and its length as the reference counts them
    score0 = [float(g("positional_scores")[i, 0, :P].astype(np.float64).sum()) for i in range(2)]
    lm = br.ToyLM(g("A"), g("B"), g("w"))
    got, info = br.beam_search_ref(lm, [[br.EOS] + [int(t) for t in p] for p in prompts], s["beam"], s["max_len_b"] - P, min_len=s["min_len"],
                                   lenpen=s["lenpen"], unnormalized=s["unnormalized"], unk_penalty=s["unkpen"], score0=score0, len0=[P, P])
    assert not info["surplus"]
    for i in range(2):
        n_h = int(g("counts")[i])
        assert len(got[i]) == n_h
        for f in range(n_h):
            n = int(g("lengths")[i, f])
            want = g("tokens")[i, f, :n]
            assert got[i][f]["tokens"].tolist() == want[P:].tolist(), (name, i, f)
            e_s = abs(got[i][f]["score"] - float(g("scores")[i, f]))
            e_p = float(np.abs(got[i][f]["positional_scores"] - g("positional_scores")[i, f, P:n]).max())
            print(f"{name} sentence {i} hypothesis {f}: {n - P} new tokens, |d score| = {e_s:.2e}, max |d positional| = {e_p:.2e}")
            assert e_s <= BAR and e_p <= BAR
    if name == "beam3_early":
        assert min(int(g("lengths")[i, :int(g("counts")[i])].max()) for i in range(2)) < s["max_len_b"] + 1
    if name == "beam5_forced_eos":
        assert (g("lengths")[:, 0] == s["max_len_b"] + 1).any()


def test_select_ref_orders_ties_by_hypothesis_then_token():
    beam, N = 2, 4
    st = br.new_state(1, beam, 3, [5])
    st["t"][0], st["score"][0] = 1, [-1.0, -2.0]
    # values: hypothesis 0 -> -3 (token 9), -3 (token 7), -4, -5; hypothesis 1 -> -3 (token 4), -4 (token 5), ...
    val = np.asarray([[-2, -2, -3, -4], [-1, -2, -3, -4]], np.float32)
    idx = np.asarray([[9, 7, 11, 12], [4, 5, 6, 8]], np.int64)
    src = np.arange(2)[:, None].repeat(8, 1).astype(np.int32)
    out, tab = br.select_ref(val, idx, st, beam, beam, src=src)
    # order: (-3, j 0, token 7), (-3, j 0, token 9), (-3, j 1, token 4), then -4: (j 0, 11), (j 1, 5)
    assert out["next"].tolist() == [7, 9] and out["parent"].tolist() == [0, 0] and out["score"][0].tolist() == [-3.0, -3.0]
    assert tab[0, :6].tolist() == [0, 0, 0, 0, 0, 0] and tab[1, :6].tolist() == [0, 0, 0, 0, 0, 1] and tab[1, 6] == 1
    assert out["t"][0] == 2 and not out["finished"][0] and st["t"][0] == 1                 # the input is left alone
    # eos first among the ties of hypothesis 1 only by its token id: (-3, j 1, eos = 2) comes after both of hypothesis 0 -> not in the first beam
    idx2 = idx.copy()
    idx2[1, 0] = br.EOS
    out, _ = br.select_ref(val, idx2, st, beam, beam)
    assert out["fin_n"][0] == 0 and out["next"].tolist() == [7, 9]
    # and with eos in hypothesis 0 it is the first candidate: finalized with the parent's history
    idx3 = idx.copy()
    idx3[0, 1] = br.EOS
    st["hist_tok"][0, 0], st["hist_par"][0, 0], st["hist_score"][0, 0] = [15, 16], [0, 0], [-1.0, -2.0]
    out, _ = br.select_ref(val, idx3, st, beam, beam)
    assert out["fin_n"][0] == 1 and out["fin_tok"][0, 0, :2].tolist() == [15, br.EOS] and out["fin_cum"][0, 0, :2].tolist() == [-1.0, -3.0]
    assert out["fin_len"][0, 0] == 2 and out["next"].tolist() == [9, 4] and out["parent"].tolist() == [0, 1]
    # a dead hypothesis: one present candidate only
    val4 = np.full((2, N), -np.inf, np.float32)
    val4[1, 0] = -1
    out, _ = br.select_ref(val4, idx, st, beam, beam)
    assert out["next"].tolist() == [4, br.PAD] and out["parent"].tolist() == [1, 1] and out["score"][0].tolist() == [-3.0, -np.inf]


@pytest.mark.parametrize("head,beam", sorted(br.E2E_SEEDS))
def test_end_to_end_seeds_keep_their_margin(head, beam):
    _, _, prompts, res, info = br.e2e_case(head, beam)
    print(f"{head} beam {beam} seed {br.E2E_SEEDS[head, beam]}: step margin {info['step_margin']:.3e}, final margin {info['final_margin']:.3e}, "
          f"lengths {[len(h['tokens']) for r in res for h in r]}")
    assert info["step_margin"] >= br.E2E_MARGIN and info["final_margin"] >= br.E2E_MARGIN and not info["surplus"]
    assert [len(p) for p in prompts] == [5, 33] and all(len(r) == beam for r in res)


def test_abi_registration():
    import ctypes
    from gnnlm_amd import _lib
    for name in ("gnnlm_beam_attn_t", "gnnlm_beam_select_t"):
        assert name in _lib.STRUCTS
    assert {"gnnlm_beam_attn", "gnnlm_beam_select", "gnnlm_transformer_lm_step_beam"} <= set(_lib.exported_symbols())
    a = _lib.STRUCTS["gnnlm_beam_attn_t"]
    assert ctypes.sizeof(a) == ctypes.sizeof(_lib.STRUCTS["gnnlm_decode_attn_t"]) + 16 and _lib.ABI_VERSION == 12
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        for name in ("gnnlm_beam_attn_t", "gnnlm_beam_select_t"):
            assert L.gnnlm_sizeof(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name])
