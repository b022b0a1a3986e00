"""gnnlm_decode_attn at the descriptor level (include/gnnlm.h): every d_k and two head counts, lengths on both sides of every chunk
and tile boundary, padded strides with NaN behind them, a done row and the two ends outside the range -- against the float64
restatement (tests/decode_ref.py) at the bar of tests/causal_ref.py: TOL on the flat profile, max(TOL, MARGIN * e32) on the key-bias
profiles that need the running maximum carried across chunks, e32 the error of causal_f32 on the same data.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import causal_ref as cr
import decode_ref as dr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
LAYERS, LAYER = 2, 1
PROFILES = ["flat", "rising", "falling", "saw"]
DKS, HS = [16, 32, 64, 128], [1, 3]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def chunk():
    from gnnlm_amd import _lib
    import re
    return int(re.search(r"#define\s+GNNLM_DECODE_CHUNK\s+(\d+)", open(_lib.HEADER).read()).group(1))


def len_values():
    C = chunk()
    return [0, 1, 31, 32, 33, C - 1, C, C + 1, 2 * C + 5]


def make_case(dk, H, profile, index):
    """Five live rows whose lengths walk the value list (so neighbours differ and every value meets every d_k), then a done row, a
    row with len = cap and a row with len = -1.  -> dict of host arrays; the cache rows above len and every pad column are NaN."""
    vals = len_values()
    cap = 2 * chunk() + 8
    lens = [vals[(index * 5 + j) % len(vals)] for j in range(5)] + [7, cap, -1]
    done = [0, 0, 0, 0, 0, 1, 0, 0]
    B, d = len(lens), H * dk
    rs = np.random.RandomState(1000 * dk + 10 * H + PROFILES.index(profile))
    ld, ld_row = 3 * d + 8, d + 8
    ld_seq, ldo = cap * ld_row + 12, d + 4
    ld_layer = B * ld_seq + 4
    qkv = np.full((B + 2, ld), np.nan, np.float32)
    K = np.full((LAYERS, ld_layer), np.nan, np.float32)
    V = np.full((LAYERS, ld_layer), np.nan, np.float32)
    blocks, e32 = [], 0.0
    for b in range(B):
        n = lens[b] if 0 <= lens[b] < cap else 3                      # (rows that take no part still carry finite inputs)
        Kb = (0.3 * np.sqrt(128.0 / dk) * rs.randn(n + 1, d)).astype(np.float32)
        Vb = rs.randn(n + 1, d).astype(np.float32)
        q = (0.3 * rs.randn(d)).astype(np.float32)
        if cr.PROFILES[profile] is not None:
            q[::dk] = cr.PROFILES[profile][0]
            Kb[:, ::dk] = cr._bias(profile, n + 1)[:, None]
        qkv[b, :d], qkv[b, d:2 * d], qkv[b, 2 * d:3 * d] = q, Kb[n], Vb[n]
        if 0 <= lens[b] < cap:
            for u in range(n):
                o = b * ld_seq + u * ld_row
                K[LAYER, o:o + d], V[LAYER, o:o + d] = Kb[u], Vb[u]
            if not done[b]:
                Qb = np.repeat(q[None], n + 1, 0)
                e32 = max(e32, float(np.abs(cr.causal_f32(Qb, Kb, Vb, [n + 1], H, 0)[-1].astype(np.float64)
                                            - cr.causal_ref(Qb, Kb, Vb, [n + 1], H, 0)[-1]).max()))
        blocks.append((q, Kb, Vb))
    return dict(dk=dk, H=H, d=d, B=B, cap=cap, lens=np.asarray(lens, np.int32), done=np.asarray(done, np.int32), qkv=qkv, K=K, V=V, ld=ld,
                ld_row=ld_row, ld_seq=ld_seq, ld_layer=ld_layer, ldo=ldo, blocks=blocks, e32=e32,
                bar=cr.TOL if profile == "flat" else max(cr.TOL, cr.MARGIN * e32))


def reference(c):
    """float64 out [B, d] and what the call must leave in the cache (bit for bit)."""
    B, d = c["B"], c["d"]
    Kc = np.zeros((B, c["cap"], d))
    Vc = np.zeros((B, c["cap"], d))
    for b, (q, Kb, Vb) in enumerate(c["blocks"]):
        n = Kb.shape[0] - 1
        Kc[b, :n], Vc[b, :n] = Kb[:n], Vb[:n]
    q, kn, vn = (c["qkv"][:B, j * d:(j + 1) * d] for j in range(3))
    out, appended, n_bad = dr.decode_attn_ref(q, kn, vn, Kc, Vc, c["lens"], c["H"], c["done"])
    K2, V2 = c["K"].copy(), c["V"].copy()
    for b in appended:
        o = b * c["ld_seq"] + int(c["lens"][b]) * c["ld_row"]
        K2[LAYER, o:o + d], V2[LAYER, o:o + d] = kn[b], vn[b]
    return out, K2, V2, n_bad


class Call:
    """The device buffers of a case and a descriptor over them; fields can be edited before ``run``."""

    def __init__(self, c, dev):
        from gnnlm_amd import _lib
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.c = c
        self.qkv, self.K, self.V = t(c["qkv"]), t(c["K"]), t(c["V"])
        self.lens, self.done = t(c["lens"]), t(c["done"])
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = torch.full((c["B"], c["ldo"]), SENTINEL, device=dev)
        L = _lib.lib()
        need = L.gnnlm_decode_attn_workspace_bytes(c["B"], c["H"], c["dk"], c["cap"])
        assert need == c["B"] * c["H"] * -(-c["cap"] // chunk()) * (c["dk"] + 4) * 4
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        a = _lib.gnnlm_decode_attn_t()
        d = c["d"]
        a.q, a.k_new, a.v_new, a.ld = self.qkv.data_ptr(), self.qkv.data_ptr() + 4 * d, self.qkv.data_ptr() + 8 * d, c["ld"]
        a.out, a.ldo = self.out.data_ptr(), c["ldo"]
        a.cache.k, a.cache.v = self.K.data_ptr(), self.V.data_ptr()
        a.cache.ld_row, a.cache.ld_seq, a.cache.ld_layer = c["ld_row"], c["ld_seq"], c["ld_layer"]
        a.cache.L, a.cache.B, a.cache.cap, a.cache.d = LAYERS, c["B"], c["cap"], d
        a.cache.len, a.cache.done, a.cache.n_bad = self.lens.data_ptr(), self.done.data_ptr(), self.n_bad.data_ptr()
        a.layer, a.H, a.dk, a.max_len = LAYER, c["H"], c["dk"], 0
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), need
        self.desc = a

    def run(self):
        from gnnlm_amd import _lib
        rc = _lib.lib().gnnlm_decode_attn(ctypes.byref(self.desc), _lib.stream())
        torch.cuda.synchronize()
        return rc

    def result(self):
        return self.out.cpu().numpy(), self.K.cpu().numpy(), self.V.cpu().numpy(), int(self.n_bad.item())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = [(dk, H, p) for dk in DKS for H in HS for p in PROFILES]


@pytest.mark.parametrize("index", range(len(CASES)), ids=[f"dk{dk}-H{H}-{p}" for dk, H, p in CASES])
def test_decode_attn_against_restatement(dev, index):
    dk, H, profile = CASES[index]
    c = make_case(dk, H, profile, index)
    want, K2, V2, n_bad = reference(c)
    call = Call(c, dev)
    assert call.run() == 0
    out, K, V, bad = call.result()
    d, B = c["d"], c["B"]
    live = [b for b in range(B) if not c["done"][b] and 0 <= c["lens"][b] < c["cap"]]
    err = float(np.abs(out[live, :d].astype(np.float64) - want[live]).max())
    print(f"dk {dk} H {H} {profile} lens {c['lens'][:5].tolist()}: max|dev - ref64| = {err:.3e}, e32 = {c['e32']:.3e}, bar {c['bar']:.3e}")
    assert np.isfinite(out[:, :d]).all()
    assert err <= c["bar"]
    # done and out-of-range rows are zero; n_bad counts the out-of-range rows, not the done row; the pad columns are untouched
    dead = [b for b in range(B) if b not in live]
    assert len(dead) == 3 and not out[dead, :d].any()
    assert bad == n_bad == 2
    assert (out[:, d:] == SENTINEL).all()
    # the appended rows bit for bit, no other cache byte changed; len and done unchanged
    assert np.array_equal(bits(K), bits(K2)) and np.array_equal(bits(V), bits(V2))
    assert np.array_equal(call.lens.cpu().numpy(), c["lens"]) and np.array_equal(call.done.cpu().numpy(), c["done"])
    # a second run (the row is appended again: the same bits) gives the same bits
    assert call.run() == 0
    out2, K3, V3, _ = call.result()
    assert np.array_equal(bits(out2), bits(out)) and np.array_equal(bits(K3), bits(K2)) and np.array_equal(bits(V3), bits(V2))
    # row b alone, B = 1, another cap, contiguous strides, max_len given: the same bits as inside the batch
    for b in live:
        n = int(c["lens"][b])
        q, Kb, Vb = c["blocks"][b]
        cap1 = n + 1 if b % 2 else n + 70
        K1 = np.full((LAYERS, cap1 * d), np.nan, np.float32)
        V1 = np.full((LAYERS, cap1 * d), np.nan, np.float32)
        K1[LAYER, :n * d], V1[LAYER, :n * d] = Kb[:n].reshape(-1), Vb[:n].reshape(-1)
        c1 = dict(c, B=1, cap=cap1, lens=np.asarray([n], np.int32), done=np.zeros(1, np.int32), qkv=c["qkv"][b:b + 1], K=K1, V=V1,
                  ld_row=d, ld_seq=cap1 * d, ld_layer=cap1 * d)
        one = Call(c1, dev)
        one.desc.max_len = n + 1
        assert one.run() == 0
        assert np.array_equal(bits(one.result()[0][0, :d]), bits(out[b, :d])), (b, n)


def test_decode_attn_refusals(dev):
    from gnnlm_amd import _lib
    c = make_case(32, 3, "flat", 0)
    _, K0, V0, _ = Call(c, dev).result()

    def refused(edit, match):
        call = Call(c, dev)
        edit(call.desc)
        assert call.run() == -22
        assert match in _lib.lib().gnnlm_last_error().decode()
        out, K, V, bad = call.result()
        assert (out == SENTINEL).all() and bad == 0 and np.array_equal(bits(K), bits(K0)) and np.array_equal(bits(V), bits(V0))

    def set_(**kw):
        def edit(a):
            for k, v in kw.items():
                obj = a.cache if k.startswith("cache_") else a
                setattr(obj, k.replace("cache_", ""), v)
        return edit

    refused(set_(dk=24, H=4), "d_k must be 16, 32, 64 or 128")
    refused(set_(H=2), "H * d_k")
    refused(set_(layer=LAYERS), "layer")
    refused(set_(layer=-1), "layer")
    refused(set_(max_len=c["cap"] + 1), "max_len")
    refused(set_(cache_ld_row=c["d"] + 2), "ld_row")
    refused(set_(cache_ld_row=c["d"] - 4), "ld_row")
    refused(set_(cache_ld_seq=c["cap"] * c["ld_row"] - 4), "ld_seq")
    refused(set_(cache_ld_layer=c["B"] * c["ld_seq"] - 4), "ld_layer")
    refused(set_(cache_len=None), "len")
    refused(set_(ld=c["d"] - 4), "ld")
    refused(lambda a: setattr(a, "q", a.q + 4), "16-byte")
    refused(lambda a: setattr(a.cache, "k", a.cache.k + 8), "16-byte")
    refused(set_(workspace_bytes=15), "workspace")
    refused(set_(workspace=None), "workspace")
    assert _lib.lib().gnnlm_decode_attn(None, _lib.stream()) == -22
    # B = 0 is accepted and touches nothing
    call = Call(c, dev)
    call.desc.cache.B = 0
    assert call.run() == 0
    assert (call.result()[0] == SENTINEL).all()


def test_profile_counts_the_keys_the_rows_hold(dev):
    """The work the event profiler books for a launch is that of the keys really attended (sum of len[b] + 1 over the rows that take
    part), not of B * cap: the bound the host knows, scaled by a count the launch reports itself."""
    from gnnlm_amd import _lib
    c = make_case(64, 3, "flat", 3)
    call = Call(c, dev)
    _lib.profile_begin(1 << 4)
    assert call.run() == 0
    prof = list(_lib.profile_end().values())
    assert len(prof) == 1 and prof[0]["launches"] == 1
    B, d, cap = c["B"], c["d"], c["cap"]
    keys = sum(int(n) + 1 for n, dn in zip(c["lens"], c["done"]) if not dn and 0 <= n < cap)
    items = B * c["H"] * -(-cap // chunk())
    bound = 8.0 * B * cap * d + 8.0 * items * (c["dk"] + 4) + 16.0 * B * d
    assert 0 < keys < B * cap / 4
    assert abs(prof[0]["bytes"] - bound * keys / (B * cap)) <= 1e-9 * bound
    assert abs(prof[0]["flops"] - 4.0 * d * keys) <= 1e-9 * bound


def test_ops_wrapper(dev):
    """ops.decode_attn over torch tensors gives the bits of the hand-filled descriptor."""
    from gnnlm_amd import ops
    c = make_case(64, 3, "saw", 5)
    call = Call(c, dev)
    assert call.run() == 0
    want = call.result()[0][:, :c["d"]]
    B, d, cap = c["B"], c["d"], c["cap"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    view = lambda a: t(a)[:, :B * c["ld_seq"]].view(LAYERS, B, c["ld_seq"])[:, :, :cap * c["ld_row"]].view(LAYERS, B, cap, c["ld_row"])[..., :d]
    qkv = t(c["qkv"])
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    got = ops.decode_attn(qkv[:B, :d], qkv[:B, d:2 * d], qkv[:B, 2 * d:3 * d], view(c["K"]), view(c["V"]), t(c["lens"]), LAYER, c["H"],
                          done=t(c["done"]), n_bad=n_bad)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)) and int(n_bad.item()) == 2
