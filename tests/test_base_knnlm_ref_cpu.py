"""The float64 restatement of kNN-LM on the base LM (tests/base_knnlm_ref.py) against what the reference's own
``SequenceScorer.generate`` + ``KNNModel.get_knn_prob`` returned (tests/golden/base_knnlm.npz, made by tests/golden/make_base_knnlm.py),
and the fixture's condition: the k = 8 neighbour sets are separated by more than 1e-3, so a float32 search picks the float64 set."""
import numpy as np
import pytest

import base_knnlm_ref as kr
import transformer_lm_ref as tr


def fixture_model(g):
    m = tr.make_model(pos_rows=128, **kr.MODEL)
    assert np.array_equal(m["E"], g["E"]) and np.array_equal(m["layers"][1]["w2"], g["layer1.w2"])      # the fixture stores its own weights
    return m


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("base_knnlm")
    return {"g": g, "m": fixture_model(g), "cache": {}}


def scored(fx, cfg, keytype, cosine, k, t, lmbda=0.25):
    key = (cfg, keytype, cosine, k, t, lmbda)
    if key not in fx["cache"]:
        g = fx["g"]
        samples = [(int(s), int(e)) for s, e in g[f"{cfg}.samples"]]
        fx["cache"][key] = kr.score(fx["m"], g["tokens"], samples, g[f"{cfg}.ctx"].tolist(), g["keys"], g["vals"], keytype, cosine, k, t, lmbda)
    return fx["cache"][key]


def test_fixture_samples_are_the_drivers(fx):
    from gnnlm_amd.token_blocks import slice_indices
    g = fx["g"]
    assert g["sizes"].tolist() == kr.SIZES and len(g["tokens"]) == sum(kr.SIZES) and g["keys"].shape == (kr.N_KEYS, kr.MODEL["d"])
    for cfg, (mode, tps, w, _) in kr.CONFIGS.items():
        samples = [(int(s), int(e)) for s, e in slice_indices(kr.SIZES, mode, tps - w)]
        assert samples == [tuple(r) for r in g[f"{cfg}.samples"].tolist()]
        ctx = tr.context_windows([e - s for s, e in samples], tps - w, w) if w else [0] * len(samples)
        assert ctx == g[f"{cfg}.ctx"].tolist()
    assert sum(g["none+ctx.ctx"]) > 0


@pytest.mark.parametrize("cfg", sorted(kr.CONFIGS))
def test_restatement_against_the_reference(fx, cfg):
    g = fx["g"]
    lm = scored(fx, cfg, None, False, 40, 1.0, 0.0)["lm"]
    want = g[f"{cfg}.lm"].astype(np.float64)
    assert (np.abs(lm - want) <= 1e-5 + 1e-6 * np.abs(want)).all()
    worst = 0.0
    for cosine in (False, True):
        for keytype in (None, "last_ffn_input"):
            for k in (40, 8):
                for t in (1.0, 0.1):
                    tag = f"{cfg}.{'cosine' if cosine else 'ip'}.{keytype or 'inner'}.k{k}.t{t}"
                    r = scored(fx, cfg, keytype, cosine, k, t)
                    want = g[tag + ".pos"].astype(np.float64)
                    err = np.abs(r["mixed"] - want)
                    worst = max(worst, float(err.max()))
                    assert (err <= 1e-5 + 1e-6 * np.abs(want)).all(), (tag, float(err.max()))       # the bar of test_transformer_lm_ref_cpu.py
                    assert np.array_equal(r["recall"], g[tag + ".recall"]), tag
    print(f"{cfg}: max |restatement - reference| over the cases = {worst:.3e}")
    assert not np.allclose(scored(fx, cfg, None, True, 8, 0.1)["mixed"], lm, atol=1e-3)                 # the kNN term moves the scores


def test_k8_neighbour_sets_are_separated(fx):
    """For every k = 8 query the 8th and the 9th similarity differ by more than 1e-3 in float64."""
    worst = np.inf
    for cfg in kr.CONFIGS:
        for cosine in (False, True):
            for keytype in (None, "last_ffn_input"):
                gap = kr.margin(scored(fx, cfg, keytype, cosine, 8, 1.0)["sims"], 8)
                worst = min(worst, float(gap.min()))
                assert (gap > kr.MARGIN).all(), (cfg, cosine, keytype, float(gap.min()))
    print(f"smallest gap between the 8th and the 9th similarity: {worst:.3e}")
    recall = scored(fx, "none+ctx", None, False, 40, 1.0)["recall"]
    assert recall.max() >= 1 and recall.min() == 0                                                       # the recall is neither all 0 nor all hits
