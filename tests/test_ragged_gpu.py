"""Batches of blocks of unequal length (--sample-break-mode eos / complete / complete_doc) on the GPU: the varlen causal
attention kernel alone, HGT.forward / the engine / the scorer / the driver on ragged batches, each against the float64 oracle
evaluated BLOCK BY BLOCK (the blocks of a batch are independent in the reference: dgl.batch is a disjoint union).

Bounds.  Kernel (tests 4, 6): the existing path's own error against the same float64 result on each block run alone is the
yardstick -- ``ops.causal_attn`` where it applies (T = 256, d_k = 128), else GEMM + ``causal_softmax_`` + GEMM; the new kernel
may be at most twice that per block (two float32 evaluations of the same sums in different orders), with 1e-6 absolute as the
floor.  HGT: ``tests/test_hgt_gpu.py``'s TOL = 5e-5.  Log-probs: 2e-5 (README "Parity").  Driver: 0.02 perplexity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import graph as og
from oracle import hgt as ohgt
from oracle import pq as opq

TOL = 5e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ the kernel alone
def attn_f64(Q, K, V, lengths, H, max_ctx):
    """float64 restatement: out[w, h] = sum_{u in block(w), u <= w, w - u < max_ctx} softmax_u(Q_w . K_u) V_u."""
    Q, K, V = (a.astype(np.float64) for a in (Q, K, V))
    out, dk, r0 = np.zeros_like(Q), Q.shape[1] // H, 0
    for n in lengths:
        w, u = np.arange(n)[:, None], np.arange(n)[None, :]
        ok = (u <= w) & ((w - u < max_ctx) if max_ctx > 0 else True)
        for h in range(H):
            c = slice(h * dk, (h + 1) * dk)
            s = np.where(ok, Q[r0:r0 + n, c] @ K[r0:r0 + n, c].T, -np.inf)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[r0:r0 + n, c] = (p / p.sum(axis=1, keepdims=True)) @ V[r0:r0 + n, c]
        r0 += n
    return out


def existing_path(Q, K, V, T, H, max_ctx):
    """One block of T tokens through what the equal-length path runs: the fused kernel at its shape, else GEMM + softmax + GEMM."""
    from gnnlm_amd import ops
    dk = Q.shape[1] // H
    if T == 256 and dk == 128:
        return ops.causal_attn(Q, K, V, 1, T, H, max_ctx)
    out = torch.empty_like(Q)
    Tp = (T + 3) & ~3
    for h in range(H):
        c = slice(h * dk, (h + 1) * dk)
        S = torch.zeros(1, T, Tp, device=Q.device)
        ops.gemm_nt(Q[:, c], K[:, c], out=S[0, :, :T])
        ops.causal_softmax_(S, T, max_ctx)
        Vt = torch.zeros(dk, Tp, device=Q.device)
        Vt[:, :T] = V[:, c].t()
        out[:, c] = ops.gemm_nt(S[0], Vt)
    return out


def qkv(rs, n, H, dk, dev):
    Q = rs.randn(n, H * dk).astype(np.float32)
    K = (rs.randn(n, H * dk) / np.sqrt(dk)).astype(np.float32) * 2.0       # (the score scale is folded into K')
    V = rs.randn(n, H * dk).astype(np.float32)
    return (Q, K, V), tuple(torch.from_numpy(a).to(dev) for a in (Q, K, V))


def check_blocks(got, host, devt, lengths, H, max_ctx, tag):
    ref = attn_f64(*host, lengths, H, max_ctx)
    r0, pairs = 0, []
    for n in lengths:
        sl = slice(r0, r0 + n)
        old = existing_path(*(t[sl].contiguous() for t in devt), n, H, max_ctx).cpu().numpy()
        e_old, e_new = np.abs(old - ref[sl]).max(), np.abs(got[sl] - ref[sl]).max()
        pairs.append((n, e_old, e_new))
        r0 += n
    print(tag, " ".join(f"{n}:{a:.2e}/{b:.2e}" for n, a, b in pairs))
    for n, e_old, e_new in pairs:
        assert e_new <= max(2.0 * e_old, 1e-6), (tag, n, e_old, e_new)


LENGTHS = [1, 2, 31, 32, 33, 64, 65, 200, 257, 700]


@pytest.mark.parametrize("max_ctx", [0, 5])
@pytest.mark.parametrize("dk", [16, 32, 64, 128])
@pytest.mark.parametrize("H", [2, 8])
def test_varlen_kernel_vs_float64(dev, H, dk, max_ctx):
    from gnnlm_amd import ops
    rs = np.random.RandomState(1000 * H + 10 * dk + max_ctx)
    for lengths in (LENGTHS, list(rs.permutation(LENGTHS))):
        host, devt = qkv(rs, sum(lengths), H, dk, dev)
        off = np.concatenate([[0], np.cumsum(lengths)])
        got = ops.causal_attn_varlen(*devt, off, H, max_ctx)
        again = ops.causal_attn_varlen(*devt, off, H, max_ctx)
        assert torch.equal(got, again)                                           # two runs: the same bits
        check_blocks(got.cpu().numpy(), host, devt, lengths, H, max_ctx, f"H={H} dk={dk} ctx={max_ctx}")


def test_varlen_blocks_do_not_see_each_other(dev):
    """Overwriting one block's Q / K / V rows leaves every other block's output bit-identical (NaN included: a row that is read
    across a boundary would poison its reader)."""
    from gnnlm_amd import ops
    rs = np.random.RandomState(5)
    lengths = [33, 1, 64, 7, 257, 31]
    off = np.concatenate([[0], np.cumsum(lengths)])
    H, dk = 4, 64
    _, devt = qkv(rs, int(off[-1]), H, dk, dev)
    base = ops.causal_attn_varlen(*devt, off, H, 0)
    for b in range(len(lengths)):
        for fill in (7.5, float("nan")):
            mod = [t.clone() for t in devt]
            for t in mod:
                t[off[b]:off[b + 1]] = fill
            got = ops.causal_attn_varlen(*mod, off, H, 0)
            keep = torch.ones(int(off[-1]), dtype=torch.bool, device=dev)
            keep[off[b]:off[b + 1]] = False
            assert torch.equal(got[keep], base[keep]), (b, fill)


def test_varlen_strided_view_and_table_views(dev):
    """Operands as column views of one [n, 3 d] buffer (how the forward hands them over) and batches as views into ONE table."""
    from gnnlm_amd import ops
    from gnnlm_amd.ragged import BlockTable
    rs = np.random.RandomState(6)
    lengths = [5, 40, 1, 90, 33, 64, 2, 17]
    H, dk = 2, 32
    table = BlockTable(lengths, dev, batches=[(0, 3), (3, 6), (6, 8)])
    r0 = 0
    for i in range(len(table)):
        rb = table.batch(i)
        host, devt = qkv(rs, rb.n_tok, H, dk, dev)
        buf = torch.cat(devt, dim=1).contiguous()
        views = [buf[:, j * H * dk:(j + 1) * H * dk] for j in range(3)]
        got = ops.causal_attn_varlen(*views, rb, H, 0).cpu().numpy()
        ref = attn_f64(*host, list(rb.lengths), H, 0)
        assert np.abs(got - ref).max() < 2e-5
        assert torch.equal(rb.segment_ids.cpu(), torch.repeat_interleave(torch.arange(rb.n_blocks), torch.as_tensor(rb.lengths)))
        r0 += rb.n_tok


def test_varlen_refuses_other_head_widths(dev):
    from gnnlm_amd import _lib, ops
    x = torch.zeros(8, 2 * 24, device=dev)
    with pytest.raises(_lib.GnnlmError, match="d_k must be"):
        ops.causal_attn_varlen(x, x, x, [0, 8], 2, 0)


def test_varlen_long_block_beside_short_ones(dev):
    """One block of 300 and one of 40 tokens, H = 8: at d = 128 (d_k = 16) and at the recipe's head width (d_k = 128)."""
    from gnnlm_amd import ops
    for H, dk in ((8, 16), (8, 128)):
        rs = np.random.RandomState(dk)
        lengths = [300, 40]
        host, devt = qkv(rs, 340, H, dk, dev)
        got = ops.causal_attn_varlen(*devt, [0, 300, 340], H, 0).cpu().numpy()
        check_blocks(got, host, devt, lengths, H, 0, f"300+40 H={H} dk={dk}")


# ------------------------------------------------------------------------------------------------ HGT.forward
def make_store(dev, codes, cen, A, b, vals=None):
    from gnnlm_amd.hgt import CodeStore
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return CodeStore(codes=t(codes), centroids=t(cen), n_store=codes.shape[0], vals=t(vals), A=t(A), b=t(b))


def oracle_hgt(sd, L, H, tgt, nb, codes, cen, A, b, n_store, l, r):
    """One block through oracle/hgt.py in float64 (as tests/test_hgt_gpu.py does): a block of any length as it is."""
    gr = og.build_graph(nb, np.zeros(nb.shape[0], np.int64), n_store, l, r)
    ntgt = opq.pq_lookup(codes[gr["ntgt_offsets"]], cen).astype(np.float64)
    if A is not None:
        ntgt = (ntgt - (b.astype(np.float64) if b is not None else 0)) @ A.astype(np.float64)
    feats = {"tgt": torch.from_numpy(tgt.astype(np.float64)), "ntgt": torch.from_numpy(ntgt)}
    return ohgt.hgt_forward({k: torch.as_tensor(v).to(torch.float64) for k, v in sd.items()}, L, H, feats, gr)


def oracle_blocks(sd, L, H, tgt, nb, lengths, codes, cen, A, b, n_store, l, r):
    ref_t, ref_n, r0 = [], [], 0
    for n in lengths:
        sl = slice(r0, r0 + n)
        h = oracle_hgt(sd, L, H, tgt[sl], nb[sl], codes, cen, A, b, n_store, l, r)
        ref_t.append(h["tgt"].numpy())
        ref_n.append(h["ntgt"].numpy())
        r0 += n
    return np.concatenate(ref_t), np.concatenate(ref_n)


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("cfg", [dict(d=128, H=8, M=16, dsub=8, opq=True, kg=6, l=2, r=2),
                                 dict(d=64, H=2, M=8, dsub=4, opq=True, kg=5, l=1, r=0),
                                 dict(d=64, H=4, M=16, dsub=4, opq=False, kg=3, l=0, r=3),
                                 dict(d=512, H=8, M=64, dsub=8, opq=True, kg=12, l=2, r=2)])
def test_hgt_ragged_vs_oracle(dev, L, cfg):
    """The configurations of tests/test_hgt_gpu.py::test_hgt_vs_oracle on a ragged batch, the oracle block by block."""
    from gnnlm_amd.hgt import HGT, NeighborGraph
    d, H, M, dsub, kg, l, r = (cfg[k] for k in ("d", "H", "M", "dsub", "kg", "l", "r"))
    rs = np.random.RandomState(L * 100 + d + 1)
    lengths = [int(v) for v in rs.randint(1, 25, size=5)] + [1, 24]
    lengths = [lengths[i] for i in rs.permutation(len(lengths))]
    n, off = sum(lengths), np.concatenate([[0], np.cumsum(lengths)])
    n_store, dpq = 500, M * dsub
    codes = rs.randint(0, 256, size=(n_store, M)).astype(np.uint8)
    cen = (rs.randn(M, 256, dsub) * 0.5).astype(np.float32)
    A = (rs.randn(dpq, d) / np.sqrt(dpq)).astype(np.float32) if cfg["opq"] else None
    b = (rs.randn(dpq) * 0.1).astype(np.float32) if cfg["opq"] else None
    sd = {k: v.numpy() for k, v in ohgt.init_hgt_weights(L, d, H, seed=L).items()}
    nb = rs.randint(0, n_store, size=(n, kg)).astype(np.int64)
    nb[rs.rand(*nb.shape) < 0.05] = -1
    nb[3] = -1
    nb[0, 0], nb[1, 0] = 0, n_store - 1
    nb[n // 2:n // 2 + 4] = nb[:4]                        # repeated rows: something for the group merge to merge
    tgt = rs.randn(n, d).astype(np.float16).astype(np.float32)
    store = make_store(dev, codes, cen, A, b)
    ref_t, ref_n = oracle_blocks(sd, L, H, tgt, nb, lengths, codes, cen, A, b, n_store, l, r)
    model = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=L, n_heads=H)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    G = NeighborGraph(ids=torch.from_numpy(nb).to(dev), n_blocks=len(lengths), T=0, left=l, right=r, store=store, block_off=off)
    feats = {"tgt": torch.from_numpy(tgt).to(dev)}
    out = model(G, features=feats, return_ntgt=True)
    assert np.abs(out["tgt"].cpu().numpy() - ref_t).max() < TOL
    assert np.abs(out["ntgt"].cpu().numpy() - ref_n).max() < TOL
    # the eval path, with the context-group merge / the row-keyed layer-0 K, V / the centre-state cache on and off: the same numbers
    outs = []
    for dedup, rows, slots in ((False, False, None), (True, False, None), (True, True, None), (True, True, 4096)):
        model.dedup_groups, model.dedup_rows, model.state_cache, model.state_cache_slots = dedup, rows, None, slots
        model.state_cache_gib = 1.0 if slots else 0.0
        outs.append(model(G, features=feats)["tgt"])
        if slots:
            outs.append(model(G, features=feats)["tgt"])                    # second call: every group is a cache hit
    assert torch.equal(outs[0], out["tgt"])
    for o in outs[1:]:
        assert torch.equal(o, outs[0])


def test_hgt_ragged_long_and_short_block(dev):
    """One block of 300 and one of 40 tokens at d = 128, H = 8 through HGT.forward: each block's output is what the equal-length
    path gives for that block run alone, to twice that path's own error against the float64 oracle (floor 1e-6)."""
    from gnnlm_amd.hgt import HGT, NeighborGraph
    d, H, M, dsub, kg, l, r, L = 128, 8, 16, 8, 4, 1, 1, 1
    rs = np.random.RandomState(77)
    lengths, n_store = [300, 40], 400
    n = sum(lengths)
    codes = rs.randint(0, 256, size=(n_store, M)).astype(np.uint8)
    cen = (rs.randn(M, 256, dsub) * 0.5).astype(np.float32)
    A = (rs.randn(M * dsub, d) / np.sqrt(M * dsub)).astype(np.float32)
    b = (rs.randn(M * dsub) * 0.1).astype(np.float32)
    sd = {k: v.numpy() for k, v in ohgt.init_hgt_weights(L, d, H, seed=3).items()}
    nb = rs.randint(0, n_store, size=(n, kg)).astype(np.int64)
    nb[rs.rand(*nb.shape) < 0.05] = -1
    tgt = rs.randn(n, d).astype(np.float16).astype(np.float32)
    store = make_store(dev, codes, cen, A, b)
    model = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=L, n_heads=H)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    ids, x = torch.from_numpy(nb).to(dev), torch.from_numpy(tgt).to(dev)
    got = model(NeighborGraph(ids=ids, n_blocks=2, T=0, left=l, right=r, store=store, block_off=[0, 300, 340]), features={"tgt": x})["tgt"].cpu().numpy()
    r0 = 0
    for T in lengths:
        sl = slice(r0, r0 + T)
        ref = oracle_hgt(sd, L, H, tgt[sl], nb[sl], codes, cen, A, b, n_store, l, r)["tgt"].numpy()
        old = model(NeighborGraph(ids=ids[sl].contiguous(), n_blocks=1, T=T, left=l, right=r, store=store), features={"tgt": x[sl].contiguous()})["tgt"].cpu().numpy()
        e_old, e_new = np.abs(old - ref).max(), np.abs(got[sl] - ref).max()
        print(f"block of {T}: existing path {e_old:.2e}, ragged {e_new:.2e}")
        assert e_new <= max(2.0 * e_old, 1e-6), (T, e_old, e_new)
        r0 += T


def test_hgt_ragged_refuses_mismatched_table_and_capture(dev):
    from gnnlm_amd.hgt import HGT, NeighborGraph
    rs = np.random.RandomState(1)
    d, H, M, dsub = 64, 4, 16, 4
    store = make_store(dev, rs.randint(0, 256, size=(50, M)).astype(np.uint8), (rs.randn(M, 256, dsub) * 0.5).astype(np.float32), None, None)
    model = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=1, n_heads=H)
    ids = torch.from_numpy(rs.randint(0, 50, size=(10, 3)).astype(np.int64)).to(dev)
    x = torch.randn(10, d, device=dev)
    with pytest.raises(ValueError, match="block_off describes"):
        model(NeighborGraph(ids=ids, n_blocks=2, T=0, left=0, right=0, store=store, block_off=[0, 4, 9]), features={"tgt": x})
    model24 = HGT(in_dim=48, hidden_dim=48, out_dim=48, n_layers=1, n_heads=2)          # d_k = 24: no varlen kernel, an error
    store24 = make_store(dev, rs.randint(0, 256, size=(50, 12)).astype(np.uint8), (rs.randn(12, 256, 4) * 0.5).astype(np.float32), None, None)
    from gnnlm_amd import _lib
    with pytest.raises(_lib.GnnlmError, match="ragged batches need"):
        model24(NeighborGraph(ids=ids, n_blocks=2, T=0, left=0, right=0, store=store24, block_off=[0, 4, 10]), features={"tgt": torch.randn(10, 48, device=dev)})


# ------------------------------------------------------------------------------------------------ engine / scorer
def test_engine_ragged_score_and_sweep_vs_oracle(dev):
    """GnnLmEngine.score on a ragged batch with lmbda > 0 and a tuning sweep: the log-probs of oracle/pipeline.py::eval_block
    run block by block, within the project's 2e-5."""
    import dataclasses
    from gnnlm_amd import ops
    from gnnlm_amd.synthetic import build_engine, make_problem, to_batch
    from oracle import pipeline
    lengths = [7, 1, 33, 12, 24, 2, 40]
    n, k = sum(lengths), 16
    prob = make_problem(n_store=3000, d=64, n_heads=4, M=16, dsub=4, vocab=600, cutoff=[100, 300], T=n, kg=8,
                        left=2, right=2, n_layers=2, k=k, seed=21)
    eng = build_engine(prob, dev)
    off = np.concatenate([[0], np.cumsum(lengths)])
    batch = dataclasses.replace(to_batch(prob["block"], dev), n_blocks=len(lengths), T=0, block_off=off)
    sweep = ([4, 16], [1.0, 0.5], [0.1, 0.25])
    lam, temp = 0.25, 1.0
    out = eng.score(batch, lam, temp, sweep=sweep)
    torch.cuda.synchronize()
    blk = prob["block"]
    model = {"sd": dict(prob["sd"]), "n_layers": prob["n_layers"], "n_heads": prob["n_heads"], "centroids": prob["cen"], "A": prob["A"],
             "b": prob["b"], "codes": prob["codes"], "vals": prob["vals"], "n_store": prob["n_store"], "left": 2, "right": 2, "asm": prob["asm"]}

    def oracle(k_, t_, l_):
        outs = []
        for b in range(len(lengths)):
            sl = slice(off[b], off[b + 1])
            one = {"neighbor_idxs": blk["ids"][sl], "tgt_feats": blk["tgt_feats"][sl], "targets": blk["targets"][sl],
                   "knn_sims": blk["knn_sims"][sl, :k_], "knn_ids": blk["knn_ids"][sl, :k_]}
            outs.append(pipeline.eval_block(one, model, l_, t_))
        return {key: torch.cat([o[key] for o in outs]).numpy() for key in ("lm_logp", "logp", "gcn_feat")}

    ref = oracle(k, temp, lam)
    assert np.abs(out["lm_logp"].cpu().numpy() - ref["lm_logp"]).max() < 2e-5
    assert np.abs(out["logp"].cpu().numpy() - ref["logp"]).max() < 2e-5
    grid = out["sweep_logp"].cpu().numpy()
    points = ops.grid_points(*sweep)
    assert grid.shape == (len(points), n)
    for g, (k_, t_, l_) in enumerate(points):
        assert np.abs(grid[g] - oracle(k_, t_, l_)["logp"]).max() < 2e-5, (k_, t_, l_)
    # the same tokens as ONE block give other numbers (the causal edges cross the boundaries): the table is being read
    whole = eng.score(dataclasses.replace(batch, n_blocks=1, T=n, block_off=None), lam, temp)["lm_logp"]
    assert (whole - out["lm_logp"]).abs().max().item() > 1e-3


# ------------------------------------------------------------------------------------------------ the driver
def write_idx_bin(data, split, sizes, tokens):
    """fairseq's mmap index + token file (MMapIndexedDataset, fairseq/data/indexed_dataset.py:350-420), int32 tokens."""
    import struct
    sizes = np.asarray(sizes, dtype=np.int32)
    with open(str(data / (split + ".idx")), "wb") as f:
        f.write(b"MMIDIDX\x00\x00" + struct.pack("<QBQ", 1, 4, len(sizes)))
        f.write(sizes.tobytes())
        f.write(np.concatenate([[0], np.cumsum(sizes.astype(np.int64) * 4)[:-1]]).astype(np.int64).tobytes())
    np.asarray(tokens, dtype=np.int32).tofile(str(data / (split + ".bin")))


def make_ragged_dir(tmp_path, sizes, L=2, seed=3, with_idx=True):
    """A synthetic data directory in the reference's on-disk formats (as tests/test_mirrors_gpu.py builds one) whose test split
    is cut into sentences of ``sizes`` tokens, + a reference-style checkpoint."""
    import json
    import os
    from argparse import Namespace
    from gnnlm_amd.synthetic import make_problem
    d, H, M, dsub, V, kg = 64, 4, 16, 4, 600, 6
    n_train, n_test = 2000, int(np.sum(sizes))
    prob = make_problem(n_store=n_train, d=d, n_heads=H, M=M, dsub=dsub, vocab=V, cutoff=[100, 300], T=n_test, kg=kg,
                        left=2, right=2, n_layers=L, k=8, seed=seed)
    data = tmp_path / "data-bin"

    def write_dstore(path, keys, vals):
        os.makedirs(path, exist_ok=True)
        keys.tofile(os.path.join(path, "keys.npy"))
        vals.tofile(os.path.join(path, "vals.npy"))
        json.dump({"dstore_size": len(vals), "hidden_size": keys.shape[1], "vocab_size": V, "dstore_fp16": True, "val_size": 1},
                  open(os.path.join(path, "info.json"), "w"))

    rs = np.random.RandomState(0)
    train_keys = rs.randn(n_train, d).astype(np.float16)
    write_dstore(str(data / "train_dstore"), train_keys, prob["vals"].astype(np.int16))
    np.save(str(data / "train_dstore" / "quantized-keys.npy"), prob["codes"])
    blk = prob["block"]
    blk["targets"] = np.maximum(blk["targets"], 4)        # ids 0-3 are fairseq's specials
    write_dstore(str(data / "test_dstore"), blk["tgt_feats"], blk["targets"].astype(np.int16))
    blk["ids"].tofile(str(data / "test_dstore" / f"neighbors.mmap.{kg}"))
    if with_idx:
        write_idx_bin(data, "test", sizes, blk["targets"])
    sd = {"decoder.hgt_decoder." + k: v for k, v in prob["sd"].items()}
    w = prob["asm"]
    for i, e in enumerate(w["emb"]):
        sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = e
        if i:
            sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = w["proj"][i]
    sd["decoder.adaptive_softmax.head.class_proj.weight"] = w["class_proj"]
    sd["decoder.tgt_quantizer.centroids_torch"] = torch.from_numpy(prob["cen"])
    sd["decoder.tgt_quantizer.A"] = torch.from_numpy(prob["A"])
    sd["decoder.tgt_quantizer.b"] = torch.from_numpy(prob["b"])
    margs = Namespace(decoder_embed_dim=d, decoder_attention_heads=H, graph_layer=L, decoder_gcn_dim=d,
                      adaptive_softmax_cutoff="100,300", orig_prob_ratio=0.0, short_cut=False, quantizer_path="")
    torch.save({"args": margs, "model": sd}, str(tmp_path / "ckpt.pt"))
    base = [str(data), "--path", str(tmp_path / "ckpt.pt"), "--gen-subset", "test", "--graph", "--neighbor-context", "2",
            "--gcn-k", str(kg), "--use-precompute-feat", "--knn-keytype", "gcn_feat", "--model-overrides", "{'orig_prob_ratio': 0.0}"]
    model = {"sd": prob["sd"], "n_layers": L, "n_heads": H, "centroids": prob["cen"], "A": prob["A"], "b": prob["b"],
             "codes": prob["codes"], "vals": prob["vals"], "n_store": n_train, "left": 2, "right": 2, "asm": w}
    return dict(prob=prob, blk=blk, data=data, base=base, model=model, train_keys=train_keys, n_test=n_test)


def oracle_run(c, ranges, lam, temp, k):
    """Sum of the scored tokens' log-probs over (context_start, start, end) blocks: eval_block per block + exact kNN."""
    from oracle import knn as oknn_, pipeline
    blk, total, count = c["blk"], 0.0, 0
    for cs, s, e in ranges:
        one = {"neighbor_idxs": blk["ids"][cs:e], "tgt_feats": blk["tgt_feats"][cs:e], "targets": blk["targets"][cs:e],
               "knn_sims": None, "knn_ids": None}
        o = pipeline.eval_block(one, c["model"], 0.0, 1.0)
        q = oknn_.normalize_queries(o["gcn_feat"].float(), True).numpy()
        dd, ii = oknn_.brute_force_search(q, c["train_keys"], k, "ip", cosine=True)
        p, _ = oknn_.knn_target_prob(dd, ii, c["prob"]["vals"], blk["targets"][cs:e], temp)
        mix = oknn_.combine_knn_and_vocab_probs(p, o["lm_logp"], lam)
        total += mix[s - cs:].double().sum().item()
        count += e - s
    return total, count


SENT_SIZES = [17, 1, 60, 5, 33, 1, 1, 48, 9, 26, 2, 41, 13, 1, 55, 30, 7, 22, 1, 38, 12, 19]


@pytest.mark.parametrize("mode,ctx", [("eos", 0), ("complete", 0), ("complete_doc", 0), ("eos", 8)])
def test_eval_lm_break_modes_end_to_end(dev, tmp_path, mode, ctx):
    """eval_lm.main with --knnlm on a split of sentences: the printed loss / perplexity against the oracle over the slices the
    reference cuts (token_blocks.py, pinned to the reference's own output by tests/test_break_modes_cpu.py), within the 0.02
    perplexity of the existing driver tests; the scored tokens are exactly what those slices cover."""
    from gnnlm_amd import eval_lm, token_blocks
    c = make_ragged_dir(tmp_path, SENT_SIZES)
    T, lam, temp, k = 64, 0.25, 1.0, 8
    ranges = token_blocks.block_ranges(SENT_SIZES, mode, T, ctx)
    sl = token_blocks.slice_indices(SENT_SIZES, mode, T)
    assert [(s, e) for _, s, e in ranges] == [tuple(r) for r in sl.tolist()]
    total, count = oracle_run(c, ranges, lam, temp, k)
    assert count == int((sl[:, 1] - sl[:, 0]).sum()) and (count == c["n_test"]) == (mode != "complete_doc")
    args = c["base"] + ["--sample-break-mode", mode, "--tokens-per-sample", str(T), "--max-tokens", str(2 * T), "--gcn-context-window", str(ctx),
                        "--knnlm", "--k", str(k), "--lmbda", str(lam), "--dstore-dir", str(c["data"] / "train_dstore"),
                        "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", str(temp), "--knn-sim-func", "ip"]
    res = eval_lm.cli_main(args)
    ref_ppl = 2 ** (-total / count / np.log(2))
    print(f"{mode} ctx={ctx}: {count} tokens, ppl {res['ppl']:.4f} (oracle {ref_ppl:.4f}), score_sum {res['score_sum']:.5f} (oracle {total:.5f})")
    assert res["count"] == count
    assert abs(res["ppl"] - ref_ppl) < 0.02
    assert abs(res["score_sum"] - total) < 2e-4 * count
    # the float32 per-hypothesis sums (the reference's accumulation order) describe the same total
    assert abs(res["score_sum_f32_order"] - res["score_sum"]) < 1e-3 * count ** 0.5 + 1e-2


def test_eval_lm_ragged_options(dev, tmp_path):
    """--sample-break-mode none prints what the run without the flag prints; a sweep, one lane / two lanes, --first, --num-shards,
    the single-rank forced exchange of --store sharded and the word outputs run on ragged batches; --graph-capture and
    --save-knnlm-dstore with complete_doc are refused."""
    from gnnlm_amd import eval_lm
    c = make_ragged_dir(tmp_path, SENT_SIZES, L=1)
    T, k = 64, 8
    common = ["--tokens-per-sample", str(T), "--max-tokens", str(2 * T), "--gcn-context-window", "0"]
    plain = eval_lm.cli_main(c["base"] + common)
    none = eval_lm.cli_main(c["base"] + common + ["--sample-break-mode", "none"])
    assert (plain["score_sum"], plain["count"], plain["ppl"]) == (none["score_sum"], none["count"], none["ppl"])
    knn = ["--knnlm", "--k", str(k), "--lmbda", "0.25", "--dstore-dir", str(c["data"] / "train_dstore"),
           "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--knn-sim-func", "ip"]
    eos = c["base"] + common + ["--sample-break-mode", "eos"]
    one = eval_lm.cli_main(eos + knn + ["--streams", "1"])
    two = eval_lm.cli_main(eos + knn + ["--streams", "2"])
    assert one["count"] == two["count"] == c["n_test"] and abs(one["score_sum"] - two["score_sum"]) < 1e-6 * c["n_test"]
    sw = eval_lm.cli_main(eos + knn + ["--sweep-lmbda", "0.1,0.25", "--sweep-k", "4,8"])
    rows = {(r["k"], r["lmbda"]): r["score_sum"] for r in sw["sweep"]}
    assert abs(rows[(8, 0.25)] - one["score_sum"]) < 1e-6 * c["n_test"] and len(rows) == 4
    first = eval_lm.cli_main(eos + ["--first", "5"])
    assert first["count"] == sum(SENT_SIZES[:5])
    halves = [eval_lm.cli_main(eos + ["--num-shards", "2", "--shard-id", str(i)]) for i in range(2)]
    lm = eval_lm.cli_main(eos)
    assert halves[0]["count"] + halves[1]["count"] == c["n_test"]
    assert abs(halves[0]["score_sum"] + halves[1]["score_sum"] - lm["score_sum"]) < 1e-6 * c["n_test"]
    # --store sharded on one rank (the forced-exchange switch): every code row goes through the bucketing and the all-to-all of
    # a one-rank group (gloo, host-staged: a test transport), per token as on equal-length batches
    import os
    import torch.distributed as dist
    saved_env = {k_: os.environ.get(k_) for k_ in ("GNNLM_EVAL_FORCE_EXCHANGE", "GNNLM_TEST_HOST_STAGED")}
    os.environ.update(GNNLM_EVAL_FORCE_EXCHANGE="1", GNNLM_TEST_HOST_STAGED="1")
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        sh = eval_lm.cli_main(eos + ["--store", "sharded"])
    finally:
        dist.destroy_process_group()
        for k_, v in saved_env.items():
            os.environ.pop(k_, None) if v is None else os.environ.__setitem__(k_, v)
    assert sh["store"] == "sharded" and sh["count"] == c["n_test"] and abs(sh["score_sum"] - lm["score_sum"]) < 1e-6 * c["n_test"]
    words = eval_lm.cli_main(eos + knn + ["--output-word-stats", "--output-knn-recall"])
    assert sum(w.count for w in words["word_stats"].values()) == c["n_test"]
    with pytest.raises(ValueError, match="graph-capture"):
        eval_lm.cli_main(eos + ["--graph-capture"])
    with pytest.raises(ValueError, match="complete_doc"):
        eval_lm.cli_main(c["base"] + common + ["--sample-break-mode", "complete_doc", "--save-knnlm-dstore", "--dstore-mmap", str(tmp_path / "out")])
    saved = eval_lm.cli_main(eos + ["--save-knnlm-dstore", "--dstore-mmap", str(tmp_path / "out")])
    vals = np.memmap(str(tmp_path / "out" / "test_dstore-gcn_feat" / "vals.npy"), dtype=np.int32, mode="r")
    assert saved["count"] == c["n_test"] and np.array_equal(np.asarray(vals).reshape(-1), c["blk"]["targets"].astype(np.int32))


def count_launches(fn):
    """(launches of the library's kernels by name, device kernels torch's profiler saw) while fn() runs."""
    from gnnlm_amd import _lib
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    _lib.profile_begin()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
    finally:
        lib_counts = {k: v["launches"] for k, v in _lib.profile_end().items()}
    kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    return lib_counts, kernels


def test_eval_lm_launches_do_not_grow_with_blocks(dev, tmp_path):
    """Two splits of the same 800 tokens, one cut into 40 sentences and one into 400, each scored as ONE batch: the same number
    of launches (the library's own, by kernel, and every device kernel torch's profiler sees)."""
    from gnnlm_amd import eval_lm
    runs = []
    for name, sizes in (("a", [20] * 40), ("b", [2] * 400)):
        (tmp_path / name).mkdir()
        c = make_ragged_dir(tmp_path / name, sizes, L=2)
        args = c["base"] + ["--sample-break-mode", "eos", "--tokens-per-sample", "800", "--max-tokens", "800", "--gcn-context-window", "0",
                            "--knnlm", "--k", "8", "--lmbda", "0.25", "--dstore-dir", str(c["data"] / "train_dstore"),
                            "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--knn-sim-func", "ip"]
        eval_lm.cli_main(args)                                     # warm-up: one-time allocations and table builds
        res = {}
        counts = count_launches(lambda: res.update(eval_lm.cli_main(args)))
        assert res["count"] == 800
        runs.append(counts)
        print(name, len(sizes), "blocks:", counts)
    assert runs[0][0] == runs[1][0]
    assert runs[0][1] == runs[1][1]
