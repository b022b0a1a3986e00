"""Diverse beam search from the base LM end to end: BeamGenerator.generate(groups=..) / (diversity_rate=..) against
diverse_beam_search_ref (tests/diverse_beam_ref.py) driven by the device's own log-probabilities -- every history the restatement asks
for is prefilled on the device and its last row's log-probs read back -- tokens and order exact, raw scores within steps x 2e-5 (the
bar of tests/test_beam_search_gpu.py: a prefilled row and the beam step's row may differ by the log-prob bar, accumulated over the
hypothesis).  The restatement ranks every token of the vocabulary, the device each hypothesis's best 2 * beam, so agreement also
shows that 2 * beam columns are enough.  The seeds are ones whose float64 run keeps every deciding pair of values 2e-3 apart; the
run here asserts its own margin.  groups 1 / rate 0 is the plain call; the command line runs through the driver.  GPU only."""
import numpy as np
import pytest
import torch

import beam_ref as br
import decode_ref as dr
import diverse_beam_ref as db
import test_beam_search_gpu as e2e
from test_beam_search_gpu import cli, dev  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LOGP_BAR = e2e.LOGP_BAR
# (head, groups, rate) -> the seed of decode_ref.gen_model / gen_prompts: float64 runs with margins >= 2e-3; in (dense, 2) one sentence
# finalizes a hypothesis early, in (adaptive, 2) eos is finalized out of the groups' places at most steps and the survivors shift
SEEDS = {("dense", 2, 0.0): 302, ("adaptive", 2, 0.0): 304, ("dense", 1, 0.5): 330}
BEAM = 4


class DeviceLprobs:
    """``lprobs_fn`` of the restatement: the history is prefilled on the device, the last row's log-probs are the device's (before the
    unk penalty, which the restatement applies)."""

    def __init__(self, g, dev):
        self.g, self.dev, self.memo = g, dev, {}

    def __call__(self, hist):
        key = tuple(hist)
        if key not in self.memo:
            lm = self.g.lm
            cache = lm.new_cache(1, len(hist) + 1)
            x, _ = lm.prefill(e2e.t(np.asarray(hist, np.int64), self.dev), np.asarray([0, len(hist)]), cache)
            self.memo[key] = self.g.next_log_probs(x[len(hist) - 1:len(hist)], {}, 1.0, 0.0)[0].double().cpu().numpy()
        return self.memo[key]


@pytest.mark.parametrize("head,groups,rate", sorted(SEEDS))
def test_diverse_beam_search_against_the_restatement_on_the_devices_log_probs(dev, head, groups, rate):
    from gnnlm_amd.beam_search import BeamGenerator
    seed = SEEDS[head, groups, rate]
    g = BeamGenerator(e2e.gen_lm(seed, head, dev))
    prompts = dr.gen_prompts(seed)[1:]
    kw = dict(lenpen=br.E2E["lenpen"], min_len=br.E2E["min_len"], unk_penalty=br.E2E["unk_penalty"])
    got = g.generate(prompts, br.E2E["max_new"], beam=BEAM, groups=groups, strength=0.5, diversity_rate=rate, **kw)
    want, info = db.diverse_beam_search_ref(DeviceLprobs(g, dev), prompts, BEAM, br.E2E["max_new"], groups=groups, strength=0.5, rate=rate, **kw)
    print(f"{head} groups {groups} rate {rate} seed {seed}: step margin {info['step_margin']:.3e}, final margin {info['final_margin']:.3e}, "
          f"shifted survivors {info['shift']}, lengths {[len(h['tokens']) for r in want for h in r]}")
    assert min(info["step_margin"], info["final_margin"]) >= br.E2E_MARGIN
    plain = g.generate(prompts, br.E2E["max_new"], beam=BEAM, **kw)
    assert [[h["tokens"].tolist() for h in r] for r in got] != [[h["tokens"].tolist() for h in r] for r in plain]
    if groups > 1:
        assert info["shift"] > 0
    for i in range(len(prompts)):
        assert [h["tokens"].tolist() for h in got[i]] == [h["tokens"].tolist() for h in want[i]], (i, got[i], want[i])
        for f, (a, b) in enumerate(zip(got[i], want[i])):
            n = len(a["tokens"])
            e_raw, e_score = abs(a["raw"] - b["raw"]), abs(a["score"] - b["score"])
            e_pos = float(np.abs(a["positional_scores"] - b["positional_scores"]).max())
            print(f"  prompt {i} hypothesis {f}: {n} tokens, |d raw| = {e_raw:.2e}, |d score| = {e_score:.2e}, max |d positional| = {e_pos:.2e} "
                  f"(bar {n * LOGP_BAR:.1e})")
            assert e_raw <= n * LOGP_BAR and e_score <= n * LOGP_BAR and e_pos <= 2 * n * LOGP_BAR


def test_one_group_and_no_rate_is_the_plain_call(dev):
    from gnnlm_amd.beam_search import BeamGenerator
    seed = br.E2E_SEEDS["dense", 5]
    g = BeamGenerator(e2e.gen_lm(seed, "dense", dev))
    prompts = dr.gen_prompts(seed)[1:]
    a = g.generate(prompts, 8, beam=5, lenpen=0.7)
    b = g.generate(prompts, 8, beam=5, lenpen=0.7, groups=1, diversity_rate=0)
    c = g.generate(prompts, 8, beam=5, lenpen=0.7, groups=1, strength=3.0, diversity_rate=0.0)
    for x in (b, c):
        for ra, rx in zip(a, x):
            assert len(ra) == len(rx) == 5
            for ha, hx in zip(ra, rx):
                assert ha["tokens"].tolist() == hx["tokens"].tolist() and ha["score"] == hx["score"] and ha["raw"] == hx["raw"]
                assert np.array_equal(ha["positional_scores"], hx["positional_scores"])
    for kw in (dict(groups=2), dict(groups=0), dict(groups=5, strength=-1.0), dict(diversity_rate=-0.5), dict(groups=5, diversity_rate=0.5)):
        with pytest.raises(ValueError):
            g.generate(prompts, 8, beam=5, **kw)


def test_command_line(dev, cli, tmp_path):
    out = tmp_path / "diverse.npz"
    flags = ["--n-prompts", "2", "--prompt-len", "8", "--max-len-b", "6", "--beam", "4", "--nbest", "4"]
    res, lines = e2e.drive(cli, flags + ["--diverse-beam-groups", "2", "--diverse-beam-strength", "0.5", "--out", str(out)])
    assert [l.split("\t")[0] for l in lines] == ["S-0"] + ["H-0", "P-0"] * 4 + ["S-1"] + ["H-1", "P-1"] * 4
    z = np.load(out)
    assert z["tokens"].shape == (2, 4, 7)
    for i in range(2):
        hs = res["hypotheses"][i]
        assert len(hs) == 4 and all(hs[f]["score"] >= hs[f + 1]["score"] for f in range(3))
        for f, h in enumerate(hs):
            _, score, text = lines[9 * i + 1 + 2 * f].split("\t")
            assert text.split() == [str(int(v)) for v in h["tokens"]] and abs(float(score) - h["score"]) <= 1e-9
            n = int(z["lengths"][i, f])
            assert z["tokens"][i, f, :n].tolist() == h["tokens"].tolist() and float(z["scores"][i, f]) == np.float32(h["score"])
    plain, _ = e2e.drive(cli, flags)
    tokens = lambda r: [[h["tokens"].tolist() for h in hs] for hs in r["hypotheses"]]
    assert tokens(res) != tokens(plain)
    # the flags work with the ones that act before the candidates or after the selection; the sibling rate through the same driver
    res_s, lines = e2e.drive(cli, flags + ["--diversity-rate", "0.5", "--fp16", "--temperature", "0.8", "--unkpen", "0.5", "--min-len", "3", "--lenpen", "0.7"])
    assert len(lines) == 18 and all(len(h["tokens"]) >= 3 and np.isfinite(h["score"]) for hs in res_s["hypotheses"] for h in hs)
    res_0, _ = e2e.drive(cli, flags + ["--diversity-rate", "0"])
    assert tokens(res_0) == tokens(plain)
    for bad, word in ((["--diverse-beam-groups", "3"], "divisible"), (["--diverse-beam-groups", "2", "--diversity-rate", "0.5"], "mutually exclusive"),
                      (["--diverse-beam-groups", "2", "--diverse-beam-strength", "-1"], "--diverse-beam-strength"), (["--diversity-rate", "-0.5"], "--diversity-rate")):
        with pytest.raises(ValueError, match=word):
            e2e.drive(cli, flags + bad)
