"""``--reinit-nfeat`` on the GPU: the token-gather kernels at the descriptor level (bit for bit: rows are copies), the table
build, the HGT forward on a token store against tests/golden/reinit_nfeat.npz (what the reference returned) and against the
float64 restatement tests/reinit_nfeat_ref.py, the exactness of merge / cache / ragged, the workspace condition, and the driver.
The restatement itself is pinned to the fixture by tests/test_reinit_nfeat_ref_cpu.py."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

import reinit_nfeat_ref as ref
from oracle import adaptive_softmax as oas
from oracle import knn as oknn

pytestmark = pytest.mark.gpu

TOL = 5e-5                  # the bar of tests/test_hgt_gpu.py on the fixture (atol, with rtol 1e-4)
SENT = 123.25               # what the output buffers hold before a call


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def up(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------ 1. gnnlm_token_gather, hand-filled descriptor
N_STORE = 50


def gather_inputs(d, itemsize, seed=0):
    rs = np.random.RandomState(seed)
    V = 40
    E = rs.randn(V, d).astype(np.float32)
    vals = rs.randint(0, V, size=N_STORE).astype(np.int16 if itemsize == 2 else np.int32)
    vals[0], vals[49], vals[7], vals[20] = 3, V - 1, V - 2, V - 1
    ids = np.array([-1, 0, 49, 50, 7, 20, 48, 1, 25, 25, 2, 51, 52, 53, -1, 33, 10], dtype=np.int64)
    return E, vals, ids, V


GATHER_CASES = [(d, lr, isz, "") for d in (32, 1024) for lr in ((0, 0), (2, 2), (3, 1)) for isz in (2, 4)] + \
    [(32, (2, 2), 4, a) for a in ("x", "labels", "valid")] + \
    [(32, (40, 30), 4, ""), (32, (70, 64), 2, "")]                      # more than 64 slots per group: the kernel's second / third label trip


@pytest.mark.parametrize("d,lr,itemsize,absent", GATHER_CASES)
def test_token_gather_descriptor(dev, d, lr, itemsize, absent):
    """Every field of gnnlm_token_gather_t: ids -1 / 0 / 49 / 50 and beyond, both label widths, ld_x > d, a device-side group count
    below n_groups (the rows beyond it untouched), each optional output absent in turn, labels >= n_vocab (n_vocab two below the
    table's rows).  Bit for bit against the restatement."""
    from gnnlm_amd import _lib
    l, r = lr
    n_g = 1 + l + r
    E, vals, ids, V = gather_inputs(d, itemsize)
    n_vocab = V - 2                                           # labels V - 2 and V - 1 (rows 7, 20, 49) are outside the vocabulary
    G, n_dev = len(ids), len(ids) - 3
    ld_x = d + 8
    want_x, want_lab, want_valid = ref.token_gather(E, vals, ids, l, r, N_STORE, n_vocab)
    assert want_valid.any() and not want_valid.all() and (want_lab.reshape(-1, n_g)[ids == 49, 0] == -1).all()
    Ed, vd, idd = up(dev, E), up(dev, vals), up(dev, ids)
    cnt = torch.tensor([n_dev], dtype=torch.int32, device=dev)
    S = G * n_g
    out_x = torch.full((S, ld_x), SENT, device=dev)
    out_l = torch.full((S,), -77, dtype=torch.int32, device=dev)
    out_v = torch.full((S,), 9, dtype=torch.uint8, device=dev)
    t = _lib.gnnlm_token_gather_t()
    t.ids, t.n_groups, t.left, t.right, t.n_store = idd.data_ptr(), G, l, r, N_STORE
    t.vals, t.vals_itemsize, t.n_vocab, t.d = vd.data_ptr(), itemsize, n_vocab, d
    t.embed, t.ld_embed = Ed.data_ptr(), d
    if absent != "x":
        t.out_x, t.ld_x = out_x.data_ptr(), ld_x
    if absent != "labels":
        t.out_labels = out_l.data_ptr()
    if absent != "valid":
        t.out_valid = out_v.data_ptr()
    t.n_groups_dev = cnt.data_ptr()
    assert _lib.lib().gnnlm_sizeof(b"gnnlm_token_gather_t") == ctypes.sizeof(t)
    _lib.call_desc("gnnlm_token_gather", t)
    torch.cuda.synchronize()
    gx, gl, gv = out_x.cpu().numpy(), out_l.cpu().numpy(), out_v.cpu().numpy()
    P = n_dev * n_g                                           # slots of the groups the device count admits
    if absent != "x":
        assert np.array_equal(gx[:P, :d].view(np.uint32), want_x[:P].view(np.uint32))
        assert (gx[:P, d:] == SENT).all() and (gx[P:] == SENT).all()
    else:
        assert (gx == SENT).all()
    assert np.array_equal(gl[:P], want_lab[:P]) and (gl[P:] == -77).all() if absent != "labels" else (gl == -77).all()
    assert np.array_equal(gv[:P], want_valid[:P]) and (gv[P:] == 9).all() if absent != "valid" else (gv == 9).all()


def test_token_gather_many_groups(dev):
    """More groups than the launch has waves (4 x 4096): the grid-stride loop, through ops.token_gather.  Bit for bit."""
    from gnnlm_amd import ops
    E, vals, _, V = gather_inputs(32, 4)
    ids = np.random.RandomState(8).randint(-2, N_STORE + 3, size=20011).astype(np.int64)
    for l, r in ((0, 0), (1, 0)):
        got = ops.token_gather(up(dev, E), up(dev, vals), up(dev, ids), l, r, n_store=N_STORE, n_vocab=V - 2, want_labels=True)
        want_x, want_lab, want_valid = ref.token_gather(E, vals, ids, l, r, N_STORE, V - 2)
        assert np.array_equal(got["x"].cpu().numpy().view(np.uint32), want_x.view(np.uint32))
        assert np.array_equal(got["labels"].cpu().numpy(), want_lab) and np.array_equal(got["valid"].cpu().numpy(), want_valid)


def test_token_gather_refusals(dev):
    from gnnlm_amd import _lib, ops
    E, vals, ids, V = gather_inputs(32, 4)
    Ed, vd, idd = up(dev, E), up(dev, vals), up(dev, ids)
    with pytest.raises(TypeError):
        ops.token_gather(Ed, vd.long(), idd)
    with pytest.raises(ValueError, match="n_store"):
        ops.token_gather(Ed, vd, idd, n_store=N_STORE + 1)
    t = _lib.gnnlm_token_gather_t()
    t.ids, t.n_groups, t.n_store, t.vals, t.vals_itemsize, t.n_vocab, t.d = idd.data_ptr(), len(ids), N_STORE, vd.data_ptr(), 3, V, 32
    with pytest.raises(_lib.GnnlmError, match="int16 or int32"):
        _lib.call_desc("gnnlm_token_gather", t)
    t.vals_itemsize, t.d = 4, 30
    x = torch.empty(len(ids), 32, device=dev)
    t.embed, t.ld_embed, t.out_x, t.ld_x = Ed.data_ptr(), 32, x.data_ptr(), 32
    with pytest.raises(_lib.GnnlmError, match="d % 4"):
        _lib.call_desc("gnnlm_token_gather", t)


@pytest.mark.parametrize("itemsize", [2, 4])
def test_neighbor_labels(dev, itemsize):
    from gnnlm_amd import ops
    E, vals, ids, V = gather_inputs(32, itemsize)
    rs = np.random.RandomState(5)
    nb = rs.randint(-3, N_STORE + 3, size=(37, 5)).astype(np.int64)
    nb[0, :4] = [-1, 0, 49, 50]
    got = ops.neighbor_labels(up(dev, nb), up(dev, vals), n_store=N_STORE, n_vocab=V - 2).cpu().numpy()
    want = ref.neighbor_labels(nb, vals, N_STORE, V - 2)
    assert got.dtype == np.int32 and np.array_equal(got, want) and (want == -1).any() and (want >= 0).any()


# ------------------------------------------------------------------------------------------ 2. the table
def _bands_sd(bands):
    sd = {}
    for i, (e, p) in enumerate(bands):
        sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = torch.as_tensor(e)
        sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = torch.as_tensor(p)
    return sd


@pytest.mark.parametrize("which", ["fixture", "random"])
def test_table_build(dev, golden, which):
    """TokenEmbedding.from_state_dict against the float64 table: error relative to sum |a||b| + 1 below 5e-7 (the bar of
    tests/test_gemm_abi_gpu.py for float32 random data); under fp16 the same bar against the operands rounded to half on the host
    (its precision-3 bar).  The plain-embedding table is the weight, bit for bit."""
    from gnnlm_amd.token_embed import TokenEmbedding
    if which == "fixture":
        g = golden("reinit_nfeat")
        bands = [(g[f"emb{i}"], g[f"proj{i}"]) for i in range(3)]
    else:
        rs = np.random.RandomState(2)
        bands = [(rs.randn(n, k).astype(np.float32), rs.randn(64, k).astype(np.float32)) for n, k in ((300, 64), (501, 16), (130, 6))]
    for prec, rnd in ((0, lambda a: np.asarray(a, np.float64)), (3, lambda a: torch.as_tensor(a).half().double().numpy())):
        te = TokenEmbedding.from_state_dict(_bands_sd(bands), None, dev, precision=prec)
        got = te.table.cpu().numpy().astype(np.float64)
        want = ref.embed_table([(rnd(e), rnd(p)) for e, p in bands])
        scale = np.concatenate([np.abs(rnd(e)) @ np.abs(rnd(p)).T for e, p in bands]) + 1.0
        err = float((np.abs(got - want) / scale).max())
        print(f"table {which} precision {prec}: max err / (sum|a||b| + 1) = {err:.3e}")
        assert te.kind == "adaptive" and got.shape == want.shape and te.table.dtype == torch.float32
        assert err < 5e-7
    w = np.random.RandomState(3).randn(77, 32).astype(np.float32)
    te = TokenEmbedding.from_state_dict({"decoder.embed_tokens.weight": torch.from_numpy(w)}, None, dev, precision=3)
    assert te.kind == "plain" and np.array_equal(te.table.cpu().numpy().view(np.uint32), w.view(np.uint32))


# ------------------------------------------------------------------------------------------ 3. forward
def token_store(dev, E, vals):
    from gnnlm_amd.hgt import TokenStore
    return TokenStore(embed=up(dev, np.asarray(E, np.float32)), vals=up(dev, vals), n_store=len(vals))


def make_model(sd, L, H, d):
    from gnnlm_amd.hgt import HGT
    model = HGT(in_dim=d, hidden_dim=d, out_dim=d, n_layers=L, n_heads=H)
    model.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return model


def run_hip(dev, model, store, nb, n_blocks, T, l, r, tgt, return_ntgt=False, block_off=None):
    from gnnlm_amd.hgt import NeighborGraph
    G = NeighborGraph(ids=up(dev, nb), n_blocks=n_blocks, T=T, left=l, right=r, store=store, block_off=block_off)
    out = model(G, features={"tgt": up(dev, tgt)}, return_ntgt=return_ntgt)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def fixture_E(dev, g, kind):
    """The table as the product builds it (HIP GEMM per band / the weight)."""
    from gnnlm_amd.token_embed import TokenEmbedding
    sd = {"decoder.embed_tokens.weight": torch.from_numpy(g["plain_weight"])} if kind == "plain" else \
        _bands_sd([(g[f"emb{i}"], g[f"proj{i}"]) for i in range(3)])
    return TokenEmbedding.from_state_dict(sd, None, dev).table


def test_forward_fixture(dev, golden):
    """Every case of the fixture, with and without return_ntgt (the elided and the full ntgt update), at the bar of test_hgt_gpu.py."""
    from gnnlm_amd.hgt import TokenStore
    g = golden("reinit_nfeat")
    cases = ref.fixture_cases(g)
    assert len(cases) == 12
    tables = {k: fixture_E(dev, g, k) for k in ("adaptive", "plain")}
    for key, tag, l, r, L, H, kind in cases:
        store = TokenStore(embed=tables[kind], vals=up(dev, g["vals"]), n_store=len(g["vals"]))
        model = make_model(ref.fixture_sd(g, L, H), L, H, 32)
        nb = g[tag + ".nb"]
        out = run_hip(dev, model, store, nb, 1, nb.shape[0], l, r, g[key + ".tgt_in"], return_ntgt=True)
        np.testing.assert_allclose(out["tgt"], g[key + f".tgt_out{L - 1}"], atol=TOL, rtol=1e-4, err_msg=key)
        np.testing.assert_allclose(out["ntgt"], g[key + f".ntgt_out{L - 1}"], atol=TOL, rtol=1e-4, err_msg=key)
        out = run_hip(dev, model, store, nb, 1, nb.shape[0], l, r, g[key + ".tgt_in"])
        np.testing.assert_allclose(out["tgt"], g[key + f".tgt_out{L - 1}"], atol=TOL, rtol=1e-4, err_msg=key)


def problem(L, H=4, d=64, V=90, n_store=1500, T=24, n_blocks=3, kg=6, seed=0):
    from oracle import hgt as ohgt
    rs = np.random.RandomState(seed)
    E = (rs.randn(V, d) * 0.5).astype(np.float32)
    vals = rs.randint(0, V, size=n_store).astype(np.int32)
    nb = rs.randint(0, 60, size=(n_blocks * T, kg)).astype(np.int64)          # few distinct rows: groups repeat within and across blocks
    nb[rs.rand(*nb.shape) < 0.1] = -1
    nb[5] = -1
    nb[0, 0], nb[1, 0], nb[2, 0] = 0, n_store - 1, n_store - 2            # (a row >= n_store is an IndexError in the reference: descriptor tests cover it)
    tgt = rs.randn(n_blocks * T, d).astype(np.float16).astype(np.float32)
    sd = ohgt.init_hgt_weights(L, d, H, seed=seed + 1)
    return dict(E=E, vals=vals, nb=nb, tgt=tgt, sd=sd, L=L, H=H, d=d, T=T, n_blocks=n_blocks, n_store=n_store)


def oracle_blocks(p, l, r):
    outs = []
    for b in range(p["n_blocks"]):
        sl = slice(b * p["T"], (b + 1) * p["T"])
        h, _ = ref.forward(p["E"].astype(np.float64), p["vals"], p["nb"][sl], p["n_store"], l, r, p["sd"], p["L"], p["H"], p["tgt"][sl])
        outs.append(h["tgt"].numpy())
    return np.concatenate(outs)


@pytest.mark.parametrize("L", [2, 3])
def test_merge_cache_ragged_are_exact(dev, L):
    """Merged == un-merged, cache on == cache off (a second pass served from the cache included): bit for bit, as for a code
    store; and within 1e-4 of the float64 restatement."""
    p = problem(L)
    l, r = 2, 2
    store = token_store(dev, p["E"], p["vals"])
    want = oracle_blocks(p, l, r)

    def run(dedup, cache_slots, passes=1):
        model = make_model(p["sd"], L, p["H"], p["d"])
        model.dedup_groups = dedup
        model.state_cache_gib = 1.0 if cache_slots else 0.0
        model.state_cache_slots = cache_slots or None
        for _ in range(passes):
            out = run_hip(dev, model, store, p["nb"], p["n_blocks"], p["T"], l, r, p["tgt"])["tgt"]
        return out, model

    plain, _ = run(False, 0)
    merged, m1 = run(True, 0)
    assert m1.last_groups is not None and m1.last_groups[1] < m1.last_groups[0]            # groups did merge
    cached, m2 = run(True, 4096, passes=2)
    assert m2.state_cache is not None and m2.state_cache.used > 0 and m2.last_groups[1] == 0      # the second pass computed nothing anew
    assert np.abs(plain - want).max() < 1e-4
    assert np.array_equal(merged.view(np.uint32), plain.view(np.uint32))
    assert np.array_equal(cached.view(np.uint32), plain.view(np.uint32))


@pytest.mark.parametrize("L", [1, 2])
def test_route_shapes(dev, L):
    """d = 1024, H = 8, T = 256: the fused causal branch, the one-pass dense star kernel on the embedding table (layer 0) and on
    the ntgt states (layer 1), 4-KB rows in the token gather.  k_g = 8, l = r = 2, one block; one token in four has neighbours
    (the float64 restatement stays a few seconds).  Within 1e-4 of the restatement, the bar of test_hgt_gpu.py."""
    from oracle import hgt as ohgt
    rs = np.random.RandomState(11)
    d, H, T, kg, V, n_store = 1024, 8, 256, 8, 64, 300
    E = (rs.randn(V, d) * 0.5).astype(np.float32)
    vals = rs.randint(0, V, size=n_store).astype(np.int16)
    nb = rs.randint(0, n_store, size=(T, kg)).astype(np.int64)
    nb[np.arange(T) % 4 != 0] = -1
    nb[0, :3] = [0, n_store - 1, -1]
    tgt = rs.randn(T, d).astype(np.float16).astype(np.float32)
    sd = ohgt.init_hgt_weights(L, d, H, seed=4)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    want, _ = ref.forward(E.astype(np.float64), vals, nb, n_store, 2, 2, sd, L, H, tgt)
    got = run_hip(dev, make_model(sd, L, H, d), token_store(dev, E, vals), nb, 1, T, 2, 2, tgt)["tgt"]
    err = float(np.abs(got - want["tgt"].numpy()).max())
    print(f"route shapes L={L}: max |err| = {err:.3e}")
    assert err < 1e-4


@pytest.mark.parametrize("L", [2, 3])
def test_ragged_equals_equal_length(dev, L):
    """Equal-length blocks through the ragged entry and through the equal-length one.  The two entries run DIFFERENT kernels on the
    causal branch (varlen / GEMM + softmax or the fused T = 256 kernel), for a token store as for a code store, so their sums
    associate differently and bits cannot agree.  The bar is the one tests/test_ragged_gpu.py holds this comparison to on a code
    store: per block, the ragged entry's error against float64 is at most twice the equal-length entry's own (floor 1e-6).
    Everything the token store adds is per slot and identical in both: the ragged result is bit-equal with the group merge on and
    off and with the centre-state cache on (a second pass served from it included) and off."""
    T, nbk = 32, 2
    p = problem(L, T=T, n_blocks=nbk, seed=6)
    store = token_store(dev, p["E"], p["vals"])
    off = np.arange(nbk + 1, dtype=np.int64) * T
    want = oracle_blocks(p, 1, 1)

    def run(dedup, cache_slots, ragged, passes=1):
        model = make_model(p["sd"], L, p["H"], p["d"])
        model.dedup_groups = dedup
        model.state_cache_gib = 1.0 if cache_slots else 0.0
        model.state_cache_slots = cache_slots or None
        for _ in range(passes):
            out = run_hip(dev, model, store, p["nb"], nbk, T, 1, 1, p["tgt"], block_off=off if ragged else None)["tgt"]
        return out, model

    eq, _ = run(True, 0, False)
    rag, _ = run(True, 0, True)
    for b in range(nbk):
        sl = slice(b * T, (b + 1) * T)
        e_eq, e_rag = float(np.abs(eq[sl] - want[sl]).max()), float(np.abs(rag[sl] - want[sl]).max())
        print(f"L={L} block {b}: equal-length {e_eq:.2e}, ragged {e_rag:.2e}, bits equal: {np.array_equal(rag[sl], eq[sl])}")
        assert e_rag <= max(2.0 * e_eq, 1e-6), (b, e_eq, e_rag)
    rag_plain, _ = run(False, 0, True)
    rag_cached, mc = run(True, 4096, True, passes=2)
    assert mc.state_cache is not None and mc.state_cache.used > 0 and mc.last_groups[1] == 0
    assert np.array_equal(rag.view(np.uint32), rag_plain.view(np.uint32))
    assert np.array_equal(rag.view(np.uint32), rag_cached.view(np.uint32))


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, dtype=np.float64)))))


def test_forward_fp16_vs_half_reference(dev, golden):
    """gemm_precision 3 on a token store, table built at that precision, against an INDEPENDENT reference, at the bar of
    tests/test_fp16_gpu.py::test_hgt_fp16_vs_reference_half: ours may not be further (RMS) from the float64 run than a model.half()
    run is.  The half run is the restatement evaluated in torch.float16 on the host -- weights, inputs and the embedding module
    rounded as model.half() rounds them (per band emb.half() @ proj.half().T in half) and every intermediate in half -- and the
    float64 run is the restatement of the fixture.  The (2, 2) cases of the fixture, the plain-embedding one included."""
    from gnnlm_amd.hgt import TokenStore
    from gnnlm_amd.token_embed import TokenEmbedding
    g = golden("reinit_nfeat")
    vals, N = g["vals"], len(g["vals"])
    bands = [(g[f"emb{i}"], g[f"proj{i}"]) for i in range(3)]
    sd_plain = {"decoder.embed_tokens.weight": torch.from_numpy(g["plain_weight"])}
    half = lambda a: torch.as_tensor(np.asarray(a)).half()
    E_half = {"adaptive": torch.cat([half(e) @ half(p).t() for e, p in bands]).numpy(), "plain": half(g["plain_weight"]).numpy()}
    h64 = lambda a: half(a).double().numpy() if np.asarray(a).dtype.kind == "f" else a
    n = 0
    for key, tag, l, r, L, H, kind in ref.fixture_cases(g):
        if (l, r) != (2, 2):
            continue
        n += 1
        nb, tgt, sd = g[tag + ".nb"], g[key + ".tgt_in"], ref.fixture_sd(g, L, H)
        ref64 = ref.forward(ref.fixture_table(g, kind), vals, nb, N, l, r, sd, L, H, tgt)[0]["tgt"].numpy()
        ref_half = ref.forward(E_half[kind], vals, nb, N, l, r, sd, L, H, tgt, dtype=torch.float16)[0]["tgt"].double().numpy()
        ref64_rounded = ref.forward(h64(E_half[kind]), vals, nb, N, l, r, {k: h64(v) for k, v in sd.items()}, L, H, h64(tgt))[0]["tgt"].numpy()
        outs = {}
        for prec in (0, 3):
            te = TokenEmbedding.from_state_dict(sd_plain if kind == "plain" else _bands_sd(bands), None, dev, precision=prec)
            model = make_model(sd, L, H, 32)
            model.gemm_precision, model.state_cache_gib = prec, 0.0
            outs[prec] = run_hip(dev, model, TokenStore(embed=te.table, vals=up(dev, vals), n_store=N), nb, 1, nb.shape[0], l, r, tgt)["tgt"]
        e_ours, e_ref, e_f32 = rms(outs[3] - ref64), rms(ref_half - ref64), float(np.abs(outs[0] - ref64).max())
        print(f"{key}: rms(ours fp16 - f64) = {e_ours:.3e}, rms(half restatement - f64) = {e_ref:.3e}, max|ours f32 - f64| = {e_f32:.3e}; "
              f"against float64 on half-rounded weights and table: ours {rms(outs[3] - ref64_rounded):.3e}, half {rms(ref_half - ref64_rounded):.3e}")
        assert e_f32 < 5e-5                                                # the yardstick is sound
        assert not np.array_equal(outs[3], outs[0])                        # the mode is really taken
        assert e_ours <= e_ref                                             # never further from float64 than a model.half() run
    assert n == 6


def test_input_adapters_on_a_token_store(dev, golden):
    """in_dim != hidden_dim (the adapters of hgt.py:476-479,505-507; weights of tests/golden/hgt_adapt.npz): the slots' embedding rows are
    gathered explicitly (ops.token_gather), pass the adapter and its GELU, and enter the forward as dense layer-0 states.  Against the
    float64 restatement at the bar of test_hgt_gpu.py."""
    from gnnlm_amd.hgt import HGT
    g = golden("hgt_adapt")
    cases = [k.split(".")[0] for k in g.files if k.endswith(".cfg")]
    adapted = 0
    for key in sorted(cases):
        d_in, d_hid, d_out, L, H, T, k, l, r = (int(v) for v in g[key + ".cfg"])
        adapted += d_in != d_hid                               # (the fourth case has only the output Linear)
        rs = np.random.RandomState(d_in + L)
        n_store, V = g["codes"].shape[0], 30
        E = (rs.randn(V, d_in) * 0.5).astype(np.float32)
        vals = rs.randint(0, V, size=n_store).astype(np.int32)
        sd = {kk[len(key) + 4:]: g[kk] for kk in g.files if kk.startswith(key + ".sd.")}
        nb, tgt = g[key + ".nb"], g[key + ".tgt_in"]
        want, _ = ref.forward(E.astype(np.float64), vals, nb, n_store, l, r, sd, L, H, tgt)
        model = HGT(in_dim=d_in, hidden_dim=d_hid, out_dim=d_out, n_layers=L, n_heads=H)
        model.load_state_dict({k_: torch.as_tensor(v) for k_, v in sd.items()}, strict=True)
        out = run_hip(dev, model, token_store(dev, E, vals), nb, 1, T, l, r, tgt, return_ntgt=True)
        np.testing.assert_allclose(out["tgt"], want["tgt"].numpy(), atol=TOL, rtol=1e-4, err_msg=key)
        np.testing.assert_allclose(out["ntgt"], want["ntgt"].numpy(), atol=TOL, rtol=1e-4, err_msg=key)
    assert adapted == 3


def test_workspace_condition(dev):
    """At L = 1 and k_g <= d the token store needs no more workspace than a code store at the same io: no [n_slots, d] buffer (the
    star edges read the table through the label index, which lives in a buffer layer 0 has not written yet)."""
    from gnnlm_amd import _lib
    L = _lib.lib()
    for d, H, T, nbk, kg in ((1024, 8, 256, 4, 1024), (32, 2, 8, 1, 4), (64, 4, 100, 3, 64)):
        io = _lib.gnnlm_hgt_io_t()
        io.n_blocks, io.T, io.kg = nbk, T, kg
        code, tok = _lib.gnnlm_hgt_t(), _lib.gnnlm_hgt_t()
        for m in (code, tok):
            m.d, m.n_heads, m.n_layers, m.left, m.right = d, H, 1, 2, 2
        code.M, code.dsub = d // 4, 4
        tok.token_embed, tok.ld_token_embed, tok.n_vocab = 4096, d, 100           # (sizes only: nothing is dereferenced)
        a, b = L.gnnlm_hgt_workspace_bytes(ctypes.byref(tok), ctypes.byref(io)), L.gnnlm_hgt_workspace_bytes(ctypes.byref(code), ctypes.byref(io))
        assert 0 < a <= b, (d, a, b)
        assert a < nbk * T * kg * 5 * d * 4 or kg * 5 < 16                        # nowhere near an [n_slots, d] buffer
    # k_g > d (no recipe): the label index cannot hide in that buffer and gets n_tok * k_g * 4 bytes of its own -- and nothing more
    io = _lib.gnnlm_hgt_io_t()
    io.n_blocks, io.T, io.kg = 2, 16, 48
    code, tok = _lib.gnnlm_hgt_t(), _lib.gnnlm_hgt_t()
    for m in (code, tok):
        m.d, m.n_heads, m.n_layers, m.left, m.right = 32, 2, 1, 2, 2
    code.M, code.dsub = 8, 4
    tok.token_embed, tok.ld_token_embed, tok.n_vocab = 4096, 32, 100
    a, b = L.gnnlm_hgt_workspace_bytes(ctypes.byref(tok), ctypes.byref(io)), L.gnnlm_hgt_workspace_bytes(ctypes.byref(code), ctypes.byref(io))
    assert b < a <= b + 2 * 16 * 48 * 4 + 256


def test_one_layer_forward_refuses_what_it_cannot_do(dev):
    from gnnlm_amd import _lib
    from gnnlm_amd.hgt import NeighborGraph
    p = problem(1)
    store = token_store(dev, p["E"], p["vals"])
    model = make_model(p["sd"], 1, p["H"], p["d"])
    G = NeighborGraph(ids=up(dev, p["nb"]), n_blocks=p["n_blocks"], T=p["T"], left=1, right=1, store=store, fetcher=object())
    with pytest.raises(ValueError, match="token store"):
        model(G, features={"tgt": up(dev, p["tgt"])})
    bad = dataclasses.replace(store, embed=store.embed[:, :32].contiguous())
    with pytest.raises(ValueError, match="embedding dimension"):
        model(dataclasses.replace(G, store=bad, fetcher=None), features={"tgt": up(dev, p["tgt"])})


# ------------------------------------------------------------------------------------------ 4. the driver
SENT_SIZES = [17, 1, 60, 5, 33, 1, 1, 48, 9, 26, 2, 41, 13, 1, 55, 30, 7, 22, 1, 38, 12, 19]


def make_dir(tmp_path, L):
    """tests/test_ragged_gpu.py::make_ragged_dir (the data directory of the driver tests, with sentence sizes) WITHOUT
    quantized-keys.npy and WITHOUT tgt_quantizer.*, the checkpoint completed with band 0's projection."""
    from test_ragged_gpu import make_ragged_dir
    c = make_ragged_dir(tmp_path, SENT_SIZES, L=L)
    os.remove(str(c["data"] / "train_dstore" / "quantized-keys.npy"))
    ck = torch.load(str(tmp_path / "ckpt.pt"), weights_only=False)
    sd = {k: v for k, v in ck["model"].items() if "tgt_quantizer" not in k}
    d = ck["args"].decoder_embed_dim
    proj0 = torch.from_numpy((np.random.RandomState(9).randn(d, d) / np.sqrt(d)).astype(np.float32))
    sd["decoder.embed_tokens.embeddings.0.1.weight"] = proj0
    ck["args"].adaptive_input_cutoff = "100,300"
    torch.save({"args": ck["args"], "model": sd}, str(tmp_path / "ckpt.pt"))
    w = c["prob"]["asm"]
    c["E64"] = ref.embed_table([(np.asarray(w["emb"][0]), proj0.numpy())] + [(np.asarray(w["emb"][i]), np.asarray(w["proj"][i])) for i in (1, 2)])
    c["L"] = L
    return c


def restated_run(c, ranges, lam=0.0, temp=1.0, k=8):
    """Per scored token, in corpus order: the float64 table + graph + HGT, the oracle's adaptive softmax, the exact kNN mix."""
    blk, m = c["blk"], c["model"]
    asm = {kk: ([None if e is None else torch.as_tensor(np.asarray(e)).double() for e in v] if isinstance(v, list) and kk != "cutoff"
                else (v.double() if torch.is_tensor(v) else v)) for kk, v in m["asm"].items()}
    out = []
    for cs, s, e in ranges:
        h, _ = ref.forward(c["E64"], m["vals"], blk["ids"][cs:e], m["n_store"], m["left"], m["right"], m["sd"], m["n_layers"], m["n_heads"],
                           np.asarray(blk["tgt_feats"][cs:e], dtype=np.float32))
        tgt = torch.as_tensor(blk["targets"][cs:e]).long()
        lm = oas.target_log_prob(h["tgt"], tgt, asm)
        if lam > 0:
            q = oknn.normalize_queries(h["tgt"].float(), True).numpy()
            dd, ii = oknn.brute_force_search(q, c["train_keys"], k, "ip", cosine=True)
            pk, _ = oknn.knn_target_prob(dd, ii, c["prob"]["vals"], blk["targets"][cs:e], temp)
            lm = oknn.combine_knn_and_vocab_probs(pk, lm.float(), lam)
        out.append(lm.double()[s - cs:])
    return torch.cat(out).numpy()


def check_run(res, scores, want):
    ppl = 2 ** (-want.sum() / len(want) / np.log(2))
    err = float(np.abs(scores - want).max())
    print(f"ppl {res['ppl']:.5f} (restated {ppl:.5f}), max per-token |d logp| = {err:.3e}")
    assert res["count"] == len(want) == len(scores)
    assert abs(res["ppl"] - ppl) < 0.02
    assert err < 2e-5


@pytest.mark.parametrize("case", ["plain", "knnlm", "eos", "layers3"])
def test_eval_lm_reinit_nfeat(dev, tmp_path, monkeypatch, case):
    """eval_lm.cli_main --reinit-nfeat on a data directory without quantized-keys.npy and a checkpoint without a quantizer: ppl
    within 0.02 and every token's log-prob within 2e-5 of the restated pipeline."""
    from test_fp16_gpu import _Recorder
    from gnnlm_amd import eval_lm, token_blocks
    c = make_dir(tmp_path, 3 if case == "layers3" else 2)
    T, n = 64, c["n_test"]
    args = c["base"] + ["--reinit-nfeat", "--tokens-per-sample", str(T), "--max-tokens", str(2 * T), "--streams", "1"]
    ranges = [(s, s, min(n, s + T)) for s in range(0, n, T)]
    lam = 0.0
    if case == "knnlm":
        lam = 0.25
        args[args.index("--max-tokens") + 1] = str(T)             # one block per batch, as in the recipe (the scorer's kNN pairing)
        args += ["--knnlm", "--k", "8", "--lmbda", str(lam), "--dstore-dir", str(c["data"] / "train_dstore"),
                 "--index-file", str(c["data"] / "train_dstore" / "faiss_store.cosine"), "--temperature", "1.0", "--knn-sim-func", "ip"]
    if case == "eos":
        args += ["--sample-break-mode", "eos"]
        ranges = token_blocks.block_ranges(SENT_SIZES, "eos", T, 0)
    rec = _Recorder(monkeypatch)
    res = eval_lm.cli_main(args)
    scores = torch.cat([b["scores"] for b in rec.take()]).cpu().numpy().astype(np.float64)
    check_run(res, scores, restated_run(c, ranges, lam))
    # without the flag the same directory cannot be scored: no code table, no quantizer
    with pytest.raises((FileNotFoundError, ValueError)):
        eval_lm.cli_main([a for a in args if a != "--reinit-nfeat"])


def test_eval_lm_reinit_nfeat_refusals(dev, tmp_path):
    from gnnlm_amd import eval_lm
    c = make_dir(tmp_path, 1)
    args = c["base"] + ["--reinit-nfeat", "--tokens-per-sample", "64", "--max-tokens", "128"]
    with pytest.raises(ValueError, match="--store sharded with --reinit-nfeat"):
        eval_lm.cli_main(args + ["--store", "sharded"])
    vals = np.fromfile(str(c["data"] / "train_dstore" / "vals.npy"), dtype=np.int16)
    vals[1234] = 600
    vals.tofile(str(c["data"] / "train_dstore" / "vals.npy"))
    with pytest.raises(ValueError, match="row 1234 = 600"):
        eval_lm.cli_main(args)


def test_eval_lm_reinit_nfeat_graph_capture_and_fp16(dev, tmp_path, monkeypatch, caplog):
    """--graph-capture replays the same launches: the score sum of the eager run (the bar of the code-store driver test).  --fp16
    at the bar tests/test_fp16_gpu.py::test_eval_lm_fp16 holds its driver case to: the run's per-token scores are bit-equal to
    GnnLmEngine.score with the precision set programmatically on the same batches and a table built at that precision, and differ
    from the f32 run's."""
    import logging
    from test_fp16_gpu import _Recorder
    from gnnlm_amd import eval_lm
    from gnnlm_amd.engine import BlockBatch, GnnLmEngine
    from gnnlm_amd.model import GnnLmModel
    c = make_dir(tmp_path, 2)
    one = c["base"] + ["--reinit-nfeat", "--tokens-per-sample", "64", "--max-tokens", "64", "--batch-blocks", "0", "--streams", "1"]
    eager = eval_lm.cli_main(one)
    cap = eval_lm.cli_main(one + ["--graph-capture"])
    assert cap["count"] == eager["count"] == c["n_test"]
    assert abs(cap["score_sum"] - eager["score_sum"]) <= 1e-12 * abs(eager["score_sum"])
    args = c["base"] + ["--reinit-nfeat", "--tokens-per-sample", "64", "--max-tokens", "128", "--streams", "1"]
    rec = _Recorder(monkeypatch)
    runs = {}
    for prec, flag in (("f32", []), ("fp16", ["--fp16"])):
        with caplog.at_level(logging.INFO):
            caplog.clear()
            res = eval_lm.cli_main(args + flag)
        assert any("token-embedding table adaptive" in r_.getMessage() for r_ in caplog.records)          # the table's size is logged
        assert res["precision"] == prec
        runs[prec] = rec.take()
    for prec in ("f32", "fp16"):
        model, _ = GnnLmModel.from_checkpoint(str(tmp_path / "ckpt.pt"), dev, vocab_size=600, reinit_nfeat=True, precision=prec)
        for b in runs[prec]:
            G = b["graph"]
            store = model.make_store(None, G.store.n_store, dev, vals=G.store.vals)
            assert torch.equal(store.embed, G.store.embed)
            eng = GnnLmEngine(model.hgt_decoder, model.adaptive_softmax, store, G.left, G.right, G.max_intra_context, precision=prec)
            o = eng.score(BlockBatch(ids=G.ids, tgt_feats=G.tgt_h, targets=b["target"].reshape(-1), n_blocks=G.n_blocks, T=G.T, block_off=G.block_off))
            assert torch.equal(o["lm_logp"].reshape(-1), b["scores"].reshape(-1))
    a, b_ = (torch.cat([b["scores"] for b in runs[p_]]) for p_ in ("f32", "fp16"))
    assert not torch.equal(a, b_) and (a - b_).abs().max() < 0.05
