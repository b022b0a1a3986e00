"""Incremental HGT (gnnlm_hgt_prefill / gnnlm_hgt_step through HGT.prefill / HGT.step) against HGT.forward and the float64 oracle.

The step is exact: the output row of token w depends on its own input row, its own neighbour ids and the K' / V' rows of the
tokens before it in its block (tests/test_gnn_decode_ref_cpu.py pins that on the oracle).  So every prefill row and every step row
is held to the oracle over the FULL sequence, at the bar the forward itself is held to (TOL of tests/test_hgt_gpu.py).
Prompt lengths [1, 31, 127, 130] + 5 steps cross GNNLM_DECODE_CHUNK = 128 from both sides."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import hgt as ohgt
from tests.test_hgt_gpu import TOL, make_store, oracle_hgt

CFGS = [dict(d=128, H=8, M=16, dsub=8, opq=True, kg=6, l=2, r=2),
        dict(d=64, H=2, M=8, dsub=4, opq=True, kg=5, l=1, r=0),
        dict(d=64, H=4, M=16, dsub=4, opq=False, kg=3, l=0, r=3)]
N_STORE, B, LENS, STEPS, CAP = 500, 4, [1, 31, 127, 130], 5, 136


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(ci, L):
    """Seeded inputs of (cfg, L) and the oracle's tgt rows of every full sequence (prompt + steps), computed once."""
    cfg = CFGS[ci]
    d, H, M, dsub, kg, l, r = (cfg[k] for k in ("d", "H", "M", "dsub", "kg", "l", "r"))
    rs = np.random.RandomState(L * 100 + d + ci)
    dpq = M * dsub
    codes = rs.randint(0, 256, size=(N_STORE, M)).astype(np.uint8)
    cen = (rs.randn(M, 256, dsub) * 0.5).astype(np.float32)
    A = (rs.randn(dpq, d) / np.sqrt(dpq)).astype(np.float32) if cfg["opq"] else None
    b = (rs.randn(dpq) * 0.1).astype(np.float32) if cfg["opq"] else None
    sd = {k: v.numpy() for k, v in ohgt.init_hgt_weights(L, d, H, seed=L).items()}
    nbs, tgts, refs = [], [], []
    for s, n in enumerate(LENS):
        nb = rs.randint(0, N_STORE, size=(n + STEPS, kg)).astype(np.int64)
        nb[rs.rand(*nb.shape) < 0.05] = -1
        nb[n + 1] = -1                                  # one STEP token without any neighbour (and, sequence 0, a prompt one below)
        if s == 1:
            nb[3] = -1
        nb[0, 0], nb[n, 0] = 0, N_STORE - 1             # the store's first and last row: in the prompt and in the first step
        tgt = rs.randn(n + STEPS, d).astype(np.float16).astype(np.float32)
        nbs.append(nb), tgts.append(tgt)
        refs.append(oracle_hgt(sd, L, H, tgt, nb, codes, cen, A, b, N_STORE, l, r)["tgt"].numpy())
    return dict(cfg=cfg, L=L, codes=codes, cen=cen, A=A, b=b, sd=sd, nb=nbs, tgt=tgts, ref=refs)


def build(c, dev):
    from gnnlm_amd.hgt import HGT
    cfg = c["cfg"]
    model = HGT(in_dim=cfg["d"], hidden_dim=cfg["d"], out_dim=cfg["d"], n_layers=c["L"], n_heads=cfg["H"])
    model.load_state_dict({k: torch.as_tensor(v) for k, v in c["sd"].items()}, strict=True)
    return model, make_store(dev, c["codes"], c["cen"], c["A"], c["b"])


def prompt_graph(c, store, dev):
    from gnnlm_amd.hgt import NeighborGraph
    ids = torch.from_numpy(np.concatenate([nb[:n] for nb, n in zip(c["nb"], LENS)])).to(dev)
    x = torch.from_numpy(np.concatenate([t[:n] for t, n in zip(c["tgt"], LENS)])).to(dev)
    off = np.concatenate([[0], np.cumsum(LENS)])
    G = NeighborGraph(ids=ids, n_blocks=B, T=0, left=c["cfg"]["l"], right=c["cfg"]["r"], store=store, block_off=off)
    return G, x


def step_inputs(c, s, dev):
    ids = torch.from_numpy(np.stack([nb[n + s] for nb, n in zip(c["nb"], LENS)])).to(dev)
    x = torch.from_numpy(np.stack([t[n + s] for t, n in zip(c["tgt"], LENS)])).to(dev)
    return ids, x


def step_graph(c, store, ids):
    from gnnlm_amd.hgt import NeighborGraph
    return NeighborGraph(ids=ids, n_blocks=B, T=1, left=c["cfg"]["l"], right=c["cfg"]["r"], store=store)


def run_steps(c, model, store, dev, cache, first=0, last=STEPS):
    outs = []
    for s in range(first, last):
        ids, x = step_inputs(c, s, dev)
        outs.append(model.step(step_graph(c, store, ids), {"tgt": x}, cache)["tgt"])
    return outs


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("ci", [0, 1, 2])
def test_prefill_and_steps_vs_forward_and_oracle(dev, ci, L):
    c = case(ci, L)
    model, store = build(c, dev)
    G, x = prompt_graph(c, store, dev)
    fwd = model(G, features={"tgt": x})["tgt"]
    cache = model.new_cache(B, CAP, device=dev)
    pre = model.prefill(G, {"tgt": x}, cache)["tgt"]
    assert torch.equal(pre, fwd)                                        # the same launches: the same bits
    ref_prompt = np.concatenate([r[:n] for r, n in zip(c["ref"], LENS)])
    err = float(np.abs(pre.cpu().numpy() - ref_prompt).max())
    print(f"cfg {ci} L {L}: prefill |err| = {err:.2e}")
    assert err < TOL
    assert cache.len.tolist() == LENS and cache.steps == max(LENS)
    outs = run_steps(c, model, store, dev, cache)
    for s, o in enumerate(outs):
        ref = np.stack([r[n + s] for r, n in zip(c["ref"], LENS)])
        err = float(np.abs(o.cpu().numpy() - ref).max())
        print(f"cfg {ci} L {L}: step {s} |err| = {err:.2e}")
        assert err < TOL, (s, err)
    assert cache.len.tolist() == [n + STEPS for n in LENS]
    assert int(cache.n_bad.item()) == 0
    # HGT.forward(incremental_state=...) keeps refusing
    with pytest.raises(NotImplementedError):
        model(G, features={"tgt": x}, incremental_state={})


def test_done_and_out_of_range_rows(dev):
    """A done row appends nothing and keeps its len; a row whose len left [0, cap) is counted once (not once per layer) and appends
    nothing; the other rows are the bits of an undisturbed run."""
    c = case(1, 2)
    model, store = build(c, dev)
    G, x = prompt_graph(c, store, dev)
    clean = model.new_cache(B, CAP, device=dev)
    model.prefill(G, {"tgt": x}, clean)
    want = run_steps(c, model, store, dev, clean, 0, 1)[0]
    cache = model.new_cache(B, CAP, device=dev)
    cache.k.fill_(7.0), cache.v.fill_(7.0)
    model.prefill(G, {"tgt": x}, cache)
    cache.done[1] = 1
    cache.len[2] = CAP                                                  # outside [0, cap)
    k0, v0 = cache.k.clone(), cache.v.clone()
    got = run_steps(c, model, store, dev, cache, 0, 1)[0]
    assert cache.len.tolist() == [LENS[0] + 1, LENS[1], CAP, LENS[3] + 1]
    assert int(cache.n_bad.item()) == 1
    assert torch.equal(got[[0, 3]], want[[0, 3]])
    for b_ in (1, 2):                                                   # nothing of these sequences was written, in any layer
        assert torch.equal(cache.k[:, b_], k0[:, b_]) and torch.equal(cache.v[:, b_], v0[:, b_])
    for b_ in (0, 3):                                                   # exactly row len of the others was
        n = LENS[b_]
        assert not torch.equal(cache.k[:, b_, n], k0[:, b_, n])
        assert torch.equal(cache.k[:, b_, n + 1:], k0[:, b_, n + 1:]) and torch.equal(cache.k[:, b_, :n], k0[:, b_, :n])


@pytest.mark.parametrize("L", [2, 3])
def test_merge_variants_give_the_same_bits(dev, L):
    """Multi-layer: the centre-state cache, the within-batch merge table alone and no merge at all -- the same bits, as in forward."""
    c = case(0, L)
    runs = []
    for dedup, slots in ((True, None), (False, None), (True, 64)):
        model, store = build(c, dev)
        model.dedup_groups, model.state_cache, model.state_cache_slots = dedup, None, slots
        model.state_cache_gib = 1.0 if slots else 0.0
        G, x = prompt_graph(c, store, dev)
        cache = model.new_cache(B, CAP, device=dev)
        pre = model.prefill(G, {"tgt": x}, cache)["tgt"]
        runs.append([pre] + run_steps(c, model, store, dev, cache))
        if slots:
            assert model.state_cache is not None and model.state_cache.stats["lookups"] >= STEPS    # the steps went through the cache
    for other in runs[1:]:
        for a, o in zip(runs[0], other):
            assert torch.equal(a, o)


def test_step_captured_in_a_hip_graph(dev):
    """HGT.step on fixed buffers, captured once and replayed for 3 steps: the bits of the eager steps; len advances on the device."""
    c = case(0, 2)
    model, store = build(c, dev)
    G, x = prompt_graph(c, store, dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):                       # one stream throughout: merge tables and workspaces are per stream
        eager_cache = model.new_cache(B, CAP, device=dev)
        model.prefill(G, {"tgt": x}, eager_cache)
        eager = run_steps(c, model, store, dev, eager_cache, 0, 4)
        cache = model.new_cache(B, CAP, device=dev)
        model.prefill(G, {"tgt": x}, cache)
        first = run_steps(c, model, store, dev, cache, 0, 1)[0]
        assert torch.equal(first, eager[0])
        ids, feats = step_inputs(c, 1, dev)
        Gs = step_graph(c, store, ids)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = model.step(Gs, {"tgt": feats}, cache, max_len=max(LENS) + STEPS)["tgt"]
        assert cache.len.tolist() == [n + 1 for n in LENS]              # a capture enqueues nothing
        for s in (1, 2, 3):
            i2, f2 = step_inputs(c, s, dev)
            ids.copy_(i2), feats.copy_(f2)
            g.replay()
            side.synchronize()
            assert torch.equal(out, eager[s]), s
            assert cache.len.tolist() == [n + 1 + s for n in LENS]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _c_entry(model, store, dev, cache_desc, mutate, B_=B, kg=6, l=2, r=2, max_len=CAP, prefill_off=None):
    """gnnlm_hgt_step (or, with prefill_off, gnnlm_hgt_prefill) on hand-made descriptors -> (rc, last error, out_tgt, sentinel)."""
    from gnnlm_amd import _lib
    from gnnlm_amd.ragged import as_ragged
    Lb = _lib.lib()
    m = type(model.prepare(store, dev)["model"]).from_buffer_copy(model.prepare(store, dev)["model"])
    m.left, m.right, m.max_intra_context, m.gemm_precision = l, r, 0, 0
    d = model.hidden_dim
    n = B_ if prefill_off is None else int(prefill_off[-1])
    feats = torch.zeros(2 * n, d, device=dev)
    ids = torch.full((2 * n, kg), -1, dtype=torch.int64, device=dev)
    out = torch.full((2 * n, d), 123.0, device=dev)
    spare = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)         # something real for a pointer that must not be followed
    io = _lib.gnnlm_hgt_io_t()
    io.n_blocks, io.T, io.kg = (B_, 1, kg) if prefill_off is None else (1, n, kg)
    io.tgt_feats, io.ids, io.out_tgt = feats.data_ptr(), ids.data_ptr(), out.data_ptr()
    mutate(m, io, cache_desc, spare.data_ptr())
    ws = torch.empty(1 << 26, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    if prefill_off is None:
        rc = Lb.gnnlm_hgt_step(ctypes.byref(m), ctypes.byref(io), ctypes.byref(cache_desc), max_len, _lib.ptr(ws), ws.numel(), _lib.stream())
    else:
        rb = as_ragged(prefill_off, dev)                                # (kept alive: the descriptor points into its tables)
        rd = rb.desc()
        rc = Lb.gnnlm_hgt_prefill(ctypes.byref(m), ctypes.byref(io), ctypes.byref(rd), ctypes.byref(cache_desc), _lib.ptr(ws), ws.numel(),
                                  _lib.stream())
    torch.cuda.synchronize()
    return rc, Lb.gnnlm_last_error().decode(), out


STEP_REFUSALS = {
    "io->T": lambda m, io, c, p: setattr(io, "T", 2),
    "io->n_blocks": lambda m, io, c, p: setattr(io, "n_blocks", B + 1),
    "max_intra_context": lambda m, io, c, p: setattr(m, "max_intra_context", 4),
    "ntgt_feats": lambda m, io, c, p: (setattr(io, "ntgt_feats", p), setattr(io, "ntgt_valid", p), setattr(io, "ld_ntgt", m.d)),
    "fetched_codes": lambda m, io, c, p: (setattr(io, "fetched_codes", p), setattr(io, "fetched_valid", p)),
    "shards": lambda m, io, c, p: setattr(m, "shards", p),
    "token_embed": lambda m, io, c, p: (setattr(m, "token_embed", p), setattr(m, "ld_token_embed", m.d), setattr(m, "n_vocab", 8),
                                         setattr(m, "vals", p), setattr(m, "vals_itemsize", 4)),
    "out_ntgt": lambda m, io, c, p: setattr(io, "out_ntgt", p),
    "cache->d": lambda m, io, c, p: (setattr(c, "d", m.d - 4)),
    "cache->L": lambda m, io, c, p: setattr(c, "L", m.n_layers + 1),
    "kv_cache": lambda m, io, c, p: setattr(c, "ld_row", c.ld_row - 4),
    "len": lambda m, io, c, p: setattr(c, "len", None),
}


@pytest.mark.parametrize("field", sorted(STEP_REFUSALS))
def test_step_refusals_name_the_field_and_launch_nothing(dev, field):
    c = case(0, 2)
    model, store = build(c, dev)
    cache = model.new_cache(B, CAP, device=dev)
    cache.len.fill_(3)
    rc, msg, out = _c_entry(model, store, dev, cache.desc(), STEP_REFUSALS[field])
    assert rc != 0 and field in msg, (rc, msg)
    assert bool((out == 123.0).all()) and cache.len.tolist() == [3] * B and int(cache.n_bad.item()) == 0


@pytest.mark.parametrize("max_len", [0, CAP + 1])
def test_step_refuses_max_len_outside_the_cache(dev, max_len):
    c = case(0, 1)
    model, store = build(c, dev)
    cache = model.new_cache(B, CAP, device=dev)
    rc, msg, out = _c_entry(model, store, dev, cache.desc(), lambda *a: None, max_len=max_len)
    assert rc != 0 and "max_len" in msg and bool((out == 123.0).all()) and cache.len.tolist() == [0] * B
    rc, msg, out = _c_entry(model, store, dev, cache.desc(), lambda *a: None)      # the same call with a sound bound runs
    assert rc == 0, msg
    assert cache.len.tolist() == [1] * B and not bool((out[:B] == 123.0).any()) and bool((out[B:] == 123.0).all())


def test_step_refuses_an_unbuilt_head_width(dev):
    from gnnlm_amd.hgt import HGT
    c = case(1, 1)                                                      # d = 64: 8 heads of 8 columns
    model = HGT(in_dim=64, hidden_dim=64, out_dim=64, n_layers=1, n_heads=8)
    store = make_store(dev, c["codes"], c["cen"], c["A"], c["b"])
    cache = model.new_cache(B, CAP, device=dev)
    rc, msg, out = _c_entry(model, store, dev, cache.desc(), lambda *a: None, kg=5, l=1, r=0)
    assert rc != 0 and "n_heads" in msg and bool((out == 123.0).all()) and cache.len.tolist() == [0] * B
    from gnnlm_amd.hgt import NeighborGraph
    G = NeighborGraph(ids=torch.full((B, 5), -1, dtype=torch.int64, device=dev), n_blocks=B, T=1, left=1, right=0, store=store)
    with pytest.raises(ValueError, match="n_heads"):
        model.step(G, {"tgt": torch.zeros(B, 64, device=dev)}, cache)


def test_prefill_refusals(dev):
    c = case(0, 2)
    model, store = build(c, dev)
    off = np.concatenate([[0], np.cumsum(LENS)])
    cache = model.new_cache(B, CAP, device=dev)
    for field, mut in (("cache->B", lambda m, io, cd, p: setattr(cd, "B", B - 1)),
                       ("cache->d", STEP_REFUSALS["cache->d"]), ("cache->L", STEP_REFUSALS["cache->L"]),
                       ("kv_cache", STEP_REFUSALS["kv_cache"])):
        rc, msg, out = _c_entry(model, store, dev, cache.desc(), mut, prefill_off=off)
        assert rc != 0 and field in msg, (field, rc, msg)
        assert bool((out == 123.0).all()) and cache.len.tolist() == [0] * B
    small = model.new_cache(B, 64, device=dev)                          # 289 tokens in 4 blocks: one holds at least 73 > 64
    rc, msg, out = _c_entry(model, store, dev, small.desc(), lambda *a: None, prefill_off=off)
    assert rc != 0 and "cap" in msg and bool((out == 123.0).all()) and small.len.tolist() == [0] * B
    # the host mirror knows the lengths themselves, and refuses the rest by name before its prelude enqueues anything
    G, x = prompt_graph(c, store, dev)
    with pytest.raises(ValueError, match="cap"):
        model.prefill(G, {"tgt": x}, model.new_cache(B, 129, device=dev))
    with pytest.raises(ValueError, match="n_blocks"):
        model.prefill(G, {"tgt": x}, model.new_cache(B + 1, CAP, device=dev))
    import dataclasses
    with pytest.raises(NotImplementedError, match="max_intra_context"):
        model.prefill(dataclasses.replace(G, max_intra_context=8), {"tgt": x}, cache)
    ids, xs = step_inputs(c, 0, dev)
    with pytest.raises(ValueError, match="io->T"):
        model.step(dataclasses.replace(step_graph(c, store, ids), T=2), {"tgt": xs}, cache)
    with pytest.raises(ValueError, match="max_len"):
        model.step(step_graph(c, store, ids), {"tgt": xs}, cache, max_len=CAP + 1)
    assert cache.len.tolist() == [0] * B
