"""The identity that incremental decoding through the HGT rests on, pinned on the float64 oracle; and the restated chain itself.  No GPU.

In the implicit graph ntgt nodes never receive from tgt nodes, a token's star edges read its own neighbours' context groups only, and
the ('tgt','intra','tgt') edges are u -> w for u <= w: so the last row of hgt_forward over a prefix of length n equals row n - 1 of
hgt_forward over ANY longer prefix with the same per-token neighbours."""
import numpy as np
import pytest

import decode_ref as dr
import gnn_decode_ref as gr
from oracle import hgt as ohgt


@pytest.mark.parametrize("L", [1, 2, 3])
def test_last_row_of_a_prefix_is_that_row_of_every_longer_prefix(L):
    d, H, M, dsub, kg, l, r, n_store, N = 32, 2, 4, 4, 4, 1, 2, 60, 14
    rs = np.random.RandomState(50 + L)
    codes = rs.randint(0, 256, size=(n_store, M)).astype(np.uint8)
    cen = (rs.randn(M, 256, dsub) * 0.5).astype(np.float32)
    A = (rs.randn(M * dsub, d) / 4).astype(np.float32)
    b = (rs.randn(M * dsub) * 0.1).astype(np.float32)
    sd = {k: v.numpy() for k, v in ohgt.init_hgt_weights(L, d, H, seed=L).items()}
    nb = rs.randint(0, n_store, size=(N, kg)).astype(np.int64)
    nb[rs.rand(N, kg) < 0.1] = -1
    nb[4] = -1                                              # a token without any neighbour
    nb[0, 0], nb[1, 0] = 0, n_store - 1
    nb[7] = nb[2]                                           # two tokens with the same neighbours: merged groups change nothing
    tgt = rs.randn(N, d)
    full = gr.hgt_rows(sd, L, H, tgt, nb, codes, cen, A, b, n_store, l, r)
    for n in (1, 2, 5, 8, N - 1):
        part = gr.hgt_rows(sd, L, H, tgt[:n], nb[:n], codes, cen, A, b, n_store, l, r)
        assert np.abs(part - full[:n]).max() < 1e-12, (L, n)
    # ... and it does depend on what the step keeps: an earlier token's row, and the token's own neighbours
    other = tgt.copy()
    other[3] += 1.0
    assert np.abs(gr.hgt_rows(sd, L, H, other, nb, codes, cen, A, b, n_store, l, r)[-1] - full[-1]).max() > 1e-6
    nb2 = nb.copy()
    nb2[-1] = (nb[-1] + 1) % n_store
    assert np.abs(gr.hgt_rows(sd, L, H, tgt, nb2, codes, cen, A, b, n_store, l, r)[-1] - full[-1]).max() > 1e-6
    assert np.abs(gr.hgt_rows(sd, L, H, tgt, nb2, codes, cen, A, b, n_store, l, r)[:-1] - full[:-1]).max() < 1e-12


def test_neighbour_ties_go_to_the_lower_id():
    keys = np.zeros((6, 4))
    keys[[1, 3, 4], 0] = 1.0
    keys[2, 0] = 2.0
    ids, gap = gr.top_neighbours(keys, np.asarray([1.0, 0, 0, 0]), 3)
    assert ids.tolist() == [2, 1, 3] and gap == 0.0


def test_the_chain_is_a_greedy_walk_of_its_own_distributions():
    """The shortest prompt's chain, dense head: every token is the argmax of the log-probs of the prefix before it, recomputed here
    from the chain's own record (neighbour rows included)."""
    c = gr.gnn_chain(0, "dense")
    m, hw = dr.gen_model(gr.GNN_SEED, "dense")
    st, prompt = gr.gnn_store(), gr.gnn_prompts()[0]
    n = len(c["tokens"])
    assert 1 <= n <= gr.GNN_NEW and c["ids"].shape == (len(prompt) + n - 1, gr.GNN_KG)
    xs = dr.incremental_rows(m, prompt + c["tokens"][:2])["out"]
    for s in range(3):
        rows = gr.hgt_rows(st["sd"], gr.GNN_LAYERS, st["H"], xs[:len(prompt) + s], c["ids"][:len(prompt) + s], st["codes"], st["cen"],
                           st["A"], st["b"], gr.GNN_KEYS, gr.GNN_LEFT, gr.GNN_RIGHT)
        lp = gr.head_logp(m, hw, rows[-1])
        lp[dr.PAD] = -np.inf
        assert int(np.argmax(lp)) == c["tokens"][s] and abs(lp.max() - c["logp"][s]) < 1e-12
