"""tests/reinit_nfeat_ref.py (the float64 restatement of ``--reinit-nfeat``: table + oracle graph + oracle HGT) is pinned to
tests/golden/reinit_nfeat.npz -- what the reference's own AdaptiveInput / nn.Embedding, extract_graph_features, new_build_graph
(quant_neighbor_feats = None) and HGT returned -- at the bar tests/test_oracle_golden.py holds hgt.npz to.  No GPU."""
import numpy as np
import pytest
import torch

import reinit_nfeat_ref as ref

ATOL, RTOL = 2e-5, 1e-4            # the bar of tests/test_oracle_golden.py::test_hgt_layers


def test_fixture_contents(golden):
    """What the issue requires of the fixture: the three bands and the padding id, -1 ids, a token without neighbours, centres at rows
    0 and N - 1, a repeated centre, one plain-embedding case, (l, r) x L x H."""
    g = golden("reinit_nfeat")
    cases = ref.fixture_cases(g)
    vals, cut, pad = g["vals"], list(g["cutoff"]), int(g["pad"])
    N = len(vals)
    assert {(c[2], c[3]) for c in cases} == {(0, 0), (1, 1), (2, 2)}
    assert {c[4] for c in cases} == {1, 2, 3} and {c[5] for c in cases} == {2, 8}
    assert sum(c[6] == "plain" for c in cases) == 1
    for tag in ("l0r0", "l1r1", "l2r2"):
        nb = g[tag + ".nb"]
        lab = vals[nb[nb >= 0]]
        assert (lab < cut[0]).any() and ((lab >= cut[0]) & (lab < cut[1])).any() and (lab >= cut[1]).any() and (lab == pad).any()
        assert (nb == -1).any() and (nb[3] == -1).all() and (nb == 0).any() and (nb == N - 1).any()
        flat = nb[nb >= 0]
        assert len(np.unique(flat)) < len(flat)


def test_table_is_the_reference_embedding(golden):
    """ntgt_in is what the reference's embed_tokens returned for the graph's labels: the per-band table reproduces it (float32
    rounding of one short dot product), the padding row is zero, and skipping band 0's projection gives another table."""
    g = golden("reinit_nfeat")
    for key, tag, l, r, L, H, kind in ref.fixture_cases(g):
        E = ref.fixture_table(g, kind)
        labels = g[tag + ".ntgt_labels"].reshape(-1)
        np.testing.assert_allclose(E[labels], g[key + ".ntgt_in"], atol=1e-6, rtol=1e-6)
        if kind == "plain":
            assert np.array_equal(E.astype(np.float32)[labels], g[key + ".ntgt_in"])          # the weight itself
    E = ref.fixture_table(g)
    assert not E[int(g["pad"])].any()
    wrong = ref.fixture_table(g, skip_band0_proj=True)
    band0 = g["l2r2.ntgt_labels"].reshape(-1) < g["cutoff"][0]
    assert band0.any() and np.abs(wrong[: g["cutoff"][0]] - E[: g["cutoff"][0]]).max() > 0.1


@pytest.mark.parametrize("skip_band0", [False, True])
def test_forward_matches_the_reference(golden, skip_band0):
    """Every case and every layer, tgt and ntgt; with band 0's projection skipped the same comparison must FAIL on the adaptive
    cases (the fixture can tell the two tables apart)."""
    g = golden("reinit_nfeat")
    vals, N = g["vals"], len(g["vals"])
    worst = 0.0
    for key, tag, l, r, L, H, kind in ref.fixture_cases(g):
        if skip_band0 and kind == "plain":
            continue
        E = ref.fixture_table(g, kind, skip_band0_proj=skip_band0)
        outs, gr = ref.forward(E, vals, g[tag + ".nb"], N, l, r, ref.fixture_sd(g, L, H), L, H, g[key + ".tgt_in"], all_layers=True)
        assert np.array_equal(vals[gr["ntgt_offsets"]], g[tag + ".ntgt_labels"].reshape(-1))    # node order and labels
        for i, h in enumerate(outs):
            for nt in ("tgt", "ntgt"):
                got, want = h[nt].numpy(), g[key + f".{nt}_out{i}"]
                if skip_band0:
                    worst = max(worst, float(np.abs(got - want).max()))
                else:
                    np.testing.assert_allclose(got, want, atol=ATOL, rtol=RTOL)
    if skip_band0:
        assert worst > 100 * ATOL, f"the fixture cannot tell a skipped band-0 projection: worst difference {worst}"


def test_slot_restatement_agrees_with_the_graph(golden):
    """token_gather's padded slots, compacted by validity, are the graph's ntgt nodes in reference order."""
    g = golden("reinit_nfeat")
    vals, N = g["vals"], len(g["vals"])
    E = ref.fixture_table(g)
    for tag, l, r in (("l0r0", 0, 0), ("l1r1", 1, 1), ("l2r2", 2, 2)):
        nb = g[tag + ".nb"]
        x, lab, valid = ref.token_gather(E, vals, nb.reshape(-1), l, r, N)
        assert np.array_equal(lab[valid.astype(bool)], g[tag + ".ntgt_labels"].reshape(-1))
        assert np.array_equal(x[valid.astype(bool)], E[g[tag + ".ntgt_labels"].reshape(-1)])
        assert not x[~valid.astype(bool)].any()
        nl = ref.neighbor_labels(nb, vals, N, E.shape[0])
        assert np.array_equal(nl.reshape(-1), lab.reshape(-1, 1 + l + r)[:, 0])
