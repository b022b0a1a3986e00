"""Nucleus (top-p) sampling without a GPU: the float64 restatement (tests/topp_ref.py) against what the reference's own
``Sampling._sample_topp`` / ``Sampling.step`` kept and returned (tests/golden/sampling_topp.npz), the margins and CDF widths of every
row, p and u the GPU tests use, the ABI, and the two command lines."""
import ctypes
import os
import re

import numpy as np
import pytest

import topp_ref as tp

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gnnlm.h")


@pytest.fixture(scope="module", autouse=True)
def documented_bound():
    """The bound every margin below leans on is the one include/gnnlm.h states for gnnlm_sample_topp: E(V) = 2^-a + 2^(2 ceil(log2 V) - b)."""
    text = " ".join(open(HEADER).read().split())
    m = re.search(r"E\(V\) = 2\^-(\d+) \+ 2\^\(2 ceil\(log2 V\) - (\d+)\)", text.replace(" * ", " "))
    assert m, "include/gnnlm.h does not state gnnlm_sample_topp's error bound"
    a, b = int(m.group(1)), int(m.group(2))
    for V in (1, 2, 65, 70001, 1 << 20, 1 << 24):
        assert tp.E_of(V) == 2.0 ** -a + 2.0 ** (2 * int(np.ceil(np.log2(V))) - b)
    assert tp.E == tp.E_of(1 << 20) <= 1e-4


@pytest.fixture(scope="module")
def g(golden):
    return golden("sampling_topp")


def test_the_restatement_keeps_what_the_reference_kept(g):
    for V in g["sizes"].tolist():
        rows = g[f"rows_{V}"]
        assert np.array_equal(rows, tp.rows_for(V))                               # the GPU tests' rows of that size
        for i, p in enumerate(g["ps"].tolist()):
            for dtype in ("f32", "f64"):
                keep, prob = g[f"keep_{dtype}_{V}_{i}"], g[f"prob_{dtype}_{V}_{i}"]
                for r in range(rows.shape[0]):
                    ids, n, S, margin = tp.nucleus(rows[r], p)
                    kept = keep[r][keep[r] >= 0]
                    assert margin >= 8 * tp.E
                    assert n == kept.size and set(kept.tolist()) == set(ids.tolist()), (V, p, dtype, r)
                    want = tp.masses(rows[r])[kept]
                    assert np.allclose(prob[r][keep[r] >= 0], want, rtol=2.0 ** -22 if dtype == "f32" else 1e-14, atol=0)
                    assert abs(prob[r].sum() - S) <= 1e-5 * S
            idx, score = g[f"step_idx_{V}_{i}"], g[f"step_score_{V}_{i}"]
            for r in range(rows.shape[0]):
                ids = tp.nucleus(rows[r], p)[0]
                assert idx[r] in ids
                # the score is log(exp(lprob)) of the index returned, in float32: the unrenormalised log-prob
                assert abs(float(score[r]) - float(rows[r, idx[r]])) <= 4 * np.spacing(np.abs(rows[r, idx[r]]))


@pytest.mark.parametrize("V", tp.SIZES + (tp.BIG_V,))
def test_margins_and_widths_of_the_gpu_cases(V):
    cases = tp.cases_for(V)
    R = tp.big_rows() if V == tp.BIG_V else tp.rows_for(V)
    ps = (tp.BIG_P,) if V == tp.BIG_V else tp.PS
    assert tp.E_of(V) <= tp.E <= 1e-4 and tp.E_of(1 << 20) == tp.E
    assert {(c["row"], c["p"]) for c in cases} == {(r, p) for r in range(R.shape[0]) for p in ps}     # no row and no p left out
    for c in cases:
        assert c["margin"] >= 8 * tp.E, c
        assert c["width"] >= tp.MIN_WIDTH, c
        assert tp.pick(R[c["row"]], c["p"], np.float32(c["u"])) == c["member"]
    for r in range(R.shape[0]):
        for p in ps:
            ids, n, _, _ = tp.nucleus(R[r], p)
            mine = {c["member"] for c in cases if c["row"] == r and c["p"] == p}
            assert {int(ids[0]), int(ids[-1])} <= mine                            # the smallest and the largest id of the nucleus
            if V > 256 and n >= 8:                                                # both sides of every place the chunk edge can be
                assert set(tp.EDGE_IDS) <= mine
            for p_end in (1.5, 1e-9):
                assert tp.nucleus(R[r], p_end)[3] >= 8 * tp.E


def test_the_rows_with_forty_equal_masses_need_p_between_multiples():
    """Forty equal heavy masses of 0.02: p = 0.3 lands on the fifteenth prefix sum, so the margin there is rounding noise -- which is
    why tests/topp_ref.py's heavy masses all differ and its p are not multiples of one."""
    m = np.full(1000, 0.2 / 960)
    m[::25] = 0.02
    lp = np.log(m).astype(np.float32)
    assert tp.nucleus(lp, 0.3)[3] < 1e-6 and tp.nucleus(lp, 0.31)[3] >= 8 * tp.E


def test_last_digit_rows_and_the_flat_row():
    R, ps, tied = tp.last_digit_rows()
    head = np.sort(R[0])[::-1][:12]
    assert (np.diff(head.view(np.int32)) == 1).all()                              # consecutive float32 numbers (negative: bits ascend)
    ids, n, _, margin = tp.nucleus(R[0], ps[0])
    assert n == 7 and margin >= 8 * tp.E and set(R[0][ids].tolist()) == set(head[:7].tolist())
    ids, n, _, margin = tp.nucleus(R[1], ps[1])
    assert n == 6 and margin >= 8 * tp.E and ids.tolist() == [1] + tied[:5].tolist() and len(set(R[1][tied].tolist())) == 1
    row = tp.flat_row()
    assert tp.nucleus(row, 0.9)[1] > 10000


def test_done_bad_and_eos_of_the_restatement():
    R = np.stack([tp.small_row(9, s) for s in range(5)])
    R[1, :] = -np.inf
    R[2, 3] = np.nan
    R[3, 0] = np.inf
    nxt, col, done, n_bad, n_keep, mass = tp.sample_ref(R, 0.5, np.full(5, 0.25), done=[0, 0, 0, 0, 1])
    assert nxt[1:].tolist() == [tp.PAD] * 4 and done.tolist() == [0 if nxt[0] != tp.EOS else 1, 1, 1, 1, 1] and n_bad == 3
    assert n_keep[0] == tp.nucleus(R[0], 0.5)[1] and (n_keep[1:] == 0).all()
    assert tp.nucleus(R[0], float("inf"))[1] == 9 and tp.nucleus(R[0], 1e-9)[0].tolist() == [int(R[0].argmax())]
    z = np.array([0.0, -0.0, -1.0], np.float32)                                   # -0 equals +0: the smaller id first
    assert tp.order(z).tolist() == [0, 1, 2]


def test_abi():
    from gnnlm_amd import _lib
    assert _lib.ABI_VERSION == 12
    assert "gnnlm_sample_topp" in _lib.exported_symbols()
    st = _lib.gnnlm_sample_topp_t
    names = [f[0] for f in st._fields_]
    assert names == ["logp", "ld", "B", "V", "topp", "u", "pad", "eos", "next", "next_logp", "done", "n_bad", "n_keep", "keep_mass"]
    assert dict(st._fields_)["topp"] is ctypes.c_double and ctypes.sizeof(st) == 104
    L = _lib.lib()
    assert L.gnnlm_sample_topp is not None and L.gnnlm_sizeof(b"gnnlm_sample_topp_t") == 104


def parse(driver, flags):
    return driver.get_parser().parse_args(["D", "--path", "p", "--max-len-b", "4"] + flags)


def test_the_command_lines():
    from gnnlm_amd import beam_search, generate
    for flags in (["--sampling", "--sampling-topp", "0.9"], ["--sampling", "--sampling-topp", "1.5"], ["--sampling", "--sampling-topp", "inf"],
                  ["--sampling", "--sampling-topk", "5", "--sampling-topp", "0"], ["--sampling-topp", "-1"], ["--sampling-topp", "0"]):
        generate.check_args(parse(generate, flags))
    refused = [(["--sampling", "--sampling-topk", "5", "--sampling-topp", "0.9"], "--sampling-topp"),
               (["--sampling"], "--sampling-topk"), (["--sampling"], "--sampling-topp"),
               (["--sampling", "--sampling-topk", "2049"], "--sampling-topk"),
               (["--sampling-topp", "0.9"], "requires --sampling"), (["--sampling", "--sampling-topp", "nan"], "--sampling-topp"),
               (["--sampling-topp", "nan"], "--sampling-topp")]
    for flags, word in refused:
        with pytest.raises(ValueError, match=word):
            generate.check_args(parse(generate, flags))
    for flags in (["--sampling-topp", "0.9"], ["--sampling-topp", "nan"]):
        with pytest.raises(ValueError, match="--sampling-topp"):
            beam_search.check_args(parse(beam_search, flags))
    beam_search.check_args(parse(beam_search, ["--sampling-topp", "-1"]))
    assert generate.Generator.check(4, True, -1, 1.0, 50, 0.9) == 1
    with pytest.raises(ValueError, match="--sampling-topk"):
        generate.Generator.check(4, True, -1, 1.0, 50)
    assert "sampling_topp" in generate.Generator.generate.__code__.co_varnames
