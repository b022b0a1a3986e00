"""The diverse beam-search restatements against the reference's own results, and the driver's argument rules (no GPU):

  * diverse_beam_search_ref over the toy model of tests/golden/diverse_beam.npz reproduces every hypothesis the reference's
    SequenceGenerator returned there with DiverseBeamSearch / DiverseSiblingsSearch (tests/golden/make_diverse_beam.py): tokens,
    lengths and order exact, scores and positional scores within 1e-5 (the bar of tests/test_beam_ref_cpu.py: the reference computes
    them in float32);
  * the cases are what they are meant to be: the groups differ from plain beam search even at strength 0, an eos leaves group 0
    mid-run and the survivors shift, siblings at rate 0 is plain beam search;
  * select_diverse_ref on hand-made arrays: the interleave, the count of a token chosen twice, groups 1 / rate 0 equal to select_ref;
  * beam_search.check_args: the reference's two messages, the penalties' signs, a namespace without the new names;
  * the header's new struct and entry point are registered.
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import beam_ref as br
import diverse_beam_ref as db

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diverse_beam.npz")
CASES = ["groups2", "groups3_strength1", "groups4", "groups2_strength0", "groups2_eos_shift", "siblings", "siblings_rate0"]
BAR = 1e-5
MARGIN = 1e-4                                        # the fixture's own condition on the reference's candidates


def load(name):
    z = np.load(GOLDEN)
    g = lambda k: z[f"{name}/{k}"]
    s = json.loads(str(g("settings")))
    prompts = [[br.EOS] + [int(t) for t in p] for p in g("prompts")]
    return g, s, prompts, br.ToyLM(g("A"), g("B"), g("w"))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    g, s, prompts, lm = load(name)
    groups, rate = max(s["groups"], 1), max(s["rate"], 0.0)
    got, info = db.diverse_beam_search_ref(lm, prompts, s["beam"], s["max_new"], groups=groups, strength=s["strength"], rate=rate, lenpen=s["lenpen"])
    print(f"{name}: step margin {info['step_margin']:.3e}, final margin {info['final_margin']:.3e}, survivors out of their group's place {info['shift']}")
    assert info["step_margin"] >= MARGIN
    for i in range(2):
        n_h = int(g("counts")[i])
        assert len(got[i]) == n_h == s["beam"]
        for f in range(n_h):
            n = int(g("lengths")[i, f])
            assert got[i][f]["tokens"].tolist() == g("tokens")[i, f, :n].tolist(), (name, i, f)
            e_s = abs(got[i][f]["score"] - float(g("scores")[i, f]))
            e_p = float(np.abs(got[i][f]["positional_scores"] - g("positional_scores")[i, f, :n]).max())
            print(f"{name} sentence {i} hypothesis {f}: {n} tokens, |d score| = {e_s:.2e}, max |d positional| = {e_p:.2e}")
            assert e_s <= BAR and e_p <= BAR
    plain, _ = br.beam_search_ref(lm, prompts, s["beam"], s["max_new"], lenpen=s["lenpen"])
    same = all([h["tokens"].tolist() for h in got[i]] == [h["tokens"].tolist() for h in plain[i]] for i in range(2))
    if name == "siblings_rate0":
        assert same and all(abs(a["score"] - b["score"]) <= 1e-12 for i in range(2) for a, b in zip(got[i], plain[i]))
    else:
        assert not same
    if name == "groups2_eos_shift":
        assert info["shift"] > 0 and min(int(g("lengths")[i].min()) for i in range(2)) < s["max_new"] + 1


def _state(beam, score, t=1, max_new=3):
    st = br.new_state(1, beam, max_new, [5])
    st["t"][0], st["score"][0] = t, score
    return st


def test_select_diverse_ref_by_hand():
    beam, N = 4, 8
    st = _state(beam, [-1.0, -1.0, -2.0, -2.0])
    # group 0 = hypotheses 0, 2; group 1 = hypotheses 1, 3.  Token 7 is the best of hypotheses 0, 1 and 2.
    val = np.tile(-np.arange(N, dtype=np.float32) / 8, (beam, 1))
    idx = np.asarray([[7, 10, 11, 12, 13, 14, 15, 16], [7, 20, 21, 22, 23, 24, 25, 26], [7, 30, 31, 32, 33, 34, 35, 36],
                      [40, 41, 42, 43, 44, 45, 46, 47]], np.int64)
    out, _ = db.select_diverse_ref(val, idx, st, beam, beam, groups=2, strength=0.5)
    # group 0 (2 * beam_g = 4): (0, 7) -1, (0, 10) -1.125, (0, 11) -1.25, (0, 12) -1.375 -- hypothesis 2 starts at -2
    # group 1: token 7 was chosen once -> (1, 7) = -1 - 0.5; (1, 20) -1.125, (1, 21) -1.25, (1, 22) -1.375, then (1, 7) at -1.5: not chosen
    # the list: places 0, 2, 4, 6 = group 0's, places 1, 3, 5, 7 = group 1's; the first beam = 4 places survive (no eos)
    assert out["next"].tolist() == [7, 20, 10, 21] and out["parent"].tolist() == [0, 1, 0, 1]
    assert out["score"][0].tolist() == [-1.0, -1.125, -1.125, -1.25]
    # strength 0: the groups are independent, group 1 takes token 7 first
    out, _ = db.select_diverse_ref(val, idx, st, beam, beam, groups=2, strength=0.0)
    assert out["next"].tolist() == [7, 7, 10, 20] and out["score"][0].tolist() == [-1.0, -1.0, -1.125, -1.125]
    # a token chosen twice by group 0 costs group 1 two strengths: hypothesis 2 now as good as hypothesis 0
    st2 = _state(beam, [-1.0, -1.0, -1.0, -2.0])
    out, _ = db.select_diverse_ref(val, idx, st2, beam, beam, groups=2, strength=0.5)
    # group 0: (0, 7) -1, (2, 7) -1, (0, 10) -1.125, (2, 30) -1.125; group 1: (1, 7) = -1 - 2 * 0.5 = -2, so (1, 20) .. (1, 23) lead
    assert out["next"].tolist() == [7, 20, 7, 21] and out["parent"].tolist() == [0, 1, 2, 1]
    # an eos first in group 0: finalized, and its survivor's place goes to group 1's candidate
    idx3 = idx.copy()
    idx3[0, 0] = br.EOS
    st["hist_tok"][0, 0], st["hist_par"][0, 0], st["hist_score"][0, 0] = [15, 16, 17, 18], [0, 0, 0, 0], [-1.0, -1.0, -2.0, -2.0]
    out, _ = db.select_diverse_ref(val, idx3, st, beam, beam, groups=2, strength=0.5)
    assert out["fin_n"][0] == 1 and out["fin_tok"][0, 0, :2].tolist() == [15, br.EOS] and out["fin_score"][0, 0] == -1.0
    assert out["next"].tolist() == [7, 10, 20, 11] and out["parent"].tolist() == [1, 0, 1, 0]          # hypothesis 0 continues group 1's
    # siblings: ranks by hand, beam 3, rate 0.25
    st3 = _state(3, [0.0, -0.25, -3.0])
    val3 = np.tile(-np.arange(6, dtype=np.float32) / 8, (3, 1))
    idx3 = np.asarray([[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25], [30, 31, 32, 33, 34, 35]], np.int64)
    out, _ = db.select_diverse_ref(val3, idx3, st3, 3, 3, rate=0.25)
    # hypothesis 0: -0.25, -0.625, -1.0, ..; hypothesis 1: -0.5, -0.875, -1.25, ..: merged -0.25, -0.5, -0.625, -0.875, -1.0, -1.25
    assert out["next"].tolist() == [10, 20, 11] and out["score"][0].tolist() == [-0.25, -0.5, -0.625]
    # groups 1 / rate 0 is select_ref, and so is the first selection under a rate
    for kw, bin_ in ((dict(), 4), (dict(rate=0.5), 1)):
        a, _ = db.select_diverse_ref(val[:bin_], idx[:bin_], st, beam, bin_, **kw)
        b, _ = br.select_ref(val[:bin_], idx[:bin_], st, beam, bin_)
        assert all(np.array_equal(a[k], b[k]) for k in br.STATE_KEYS)


def test_check_args():
    from gnnlm_amd import beam_search as bs
    parsed = bs.get_parser().parse_args(["DATA", "--path", "x.pt"])
    # a flag that is not given leaves no name behind (the namespace of a plain run is unchanged); the reference's defaults
    # -1 / 0.5 / -1.0 are what check_args and diverse_args read then, as for a namespace built by hand without the names
    assert not {"diverse_beam_groups", "diverse_beam_strength", "diversity_rate"} & set(vars(parsed))
    for args in (parsed, SimpleNamespace(**vars(parsed)), SimpleNamespace(**dict(vars(parsed), diverse_beam_groups=-1, diverse_beam_strength=0.5, diversity_rate=-1.0))):
        bs.check_args(args)
        assert bs.diverse_args(args) == (1, 0.5, 0.0)

    def parse(*flags):
        return bs.get_parser().parse_args(["DATA", "--path", "x.pt", "--beam", "4"] + list(flags))

    with pytest.raises(ValueError, match="Provided Search parameters are mutually exclusive."):
        bs.check_args(parse("--diverse-beam-groups", "2", "--diversity-rate", "0.5"))
    with pytest.raises(ValueError, match="DiverseBeamSearch requires --beam to be divisible by the number of groups"):
        bs.check_args(parse("--diverse-beam-groups", "3"))
    with pytest.raises(ValueError, match="--diverse-beam-strength"):
        bs.check_args(parse("--diverse-beam-groups", "2", "--diverse-beam-strength", "-0.5"))
    with pytest.raises(ValueError, match="--diversity-rate"):
        bs.check_args(parse("--diversity-rate", "-0.5"))
    for flags, want in ((("--diverse-beam-groups", "2"), (2, 0.5, 0.0)), (("--diverse-beam-groups", "4", "--diverse-beam-strength", "0"), (4, 0.0, 0.0)),
                        (("--diversity-rate", "0.5"), (1, 0.5, 0.5)), (("--diversity-rate", "0"), (1, 0.5, 0.0)), (("--diversity-rate", "-1"), (1, 0.5, 0.0)),
                        (("--diversity-rate", "-2"), (1, 0.5, 0.0)), (("--diverse-beam-groups", "2", "--diversity-rate", "0"), (2, 0.5, 0.0))):
        a = parse(*flags)
        bs.check_args(a)
        assert bs.diverse_args(a) == want, flags
    from gnnlm_amd import generate
    with pytest.raises(SystemExit):
        generate.get_parser().parse_args(["DATA", "--path", "x.pt", "--diverse-beam-groups", "2"])


def test_generate_refuses_bad_penalties_before_any_device_work():
    from gnnlm_amd.beam_search import BeamGenerator
    for kw, word in ((dict(groups=3), "divisible"), (dict(groups=0), "divisible"), (dict(groups=2, strength=-1.0), "not negative"),
                     (dict(diversity_rate=-0.5), "not negative"), (dict(groups=2, diversity_rate=0.5), "mutually exclusive")):
        with pytest.raises(ValueError, match=word):
            BeamGenerator.check_diverse(4, **dict(dict(groups=1, strength=0.5, diversity_rate=0.0), **kw))
    BeamGenerator.check_diverse(4, 1, 0.5, 0.0)
    BeamGenerator.check_diverse(6, 3, 0.0, 0.0)


def test_abi_registration():
    import ctypes
    from gnnlm_amd import _lib
    st = _lib.STRUCTS["gnnlm_beam_select_diverse_t"]
    assert "gnnlm_beam_select_diverse" in _lib.exported_symbols() and _lib.ABI_VERSION == 12
    assert ctypes.sizeof(st) == ctypes.sizeof(_lib.STRUCTS["gnnlm_beam_select_t"]) + 16
    assert [f[0] for f in st._fields_] == ["sel", "groups", "strength", "rate", "reserved"]
    if os.path.exists(_lib.LIB_PATH):
        assert _lib.lib().gnnlm_sizeof(b"gnnlm_beam_select_diverse_t") == ctypes.sizeof(st)
        assert hasattr(_lib.lib(), "gnnlm_beam_select_diverse")
