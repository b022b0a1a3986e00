"""gnnlm_beam_attn at the descriptor level (include/gnnlm.h): 2 sentences x beam 3, H = 2, d_k 16 and 128, lengths on the chunk
edges, tables that mix the slots of a sentence key by key with the prompt keys in slot b * beam only -- bit for bit against
gnnlm_decode_attn on a cache materialized contiguously by a torch gather of the same rows.  Every cache row no table names is NaN and
every table entry at u >= len is out of range, so a key read from the wrong place or a table entry read too far shows.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
LAYERS, LAYER = 2, 1
SENT, BEAM, H = 2, 3, 2
S = SENT * BEAM
CAP = 264
PROMPT = [100, 40]                                  # the prompt rows of the two sentences (held in slot b * beam), where len allows
LAYOUTS = {
    # name: (len per slot, done per slot, bad table entries {slot: (u, value)})
    # (a launch writes row len[s] of slot s while others read: a table names only slots at least as long, as in beam search, where
    # the hypotheses of a sentence are equally long)
    "edges": ([128, 0, 127, 257, 129, 129], [0] * 6, {}),
    "done_and_bad": ([129, 129, 129, 257, 257, 257], [0, 1, 0, 0, 0, 0], {4: (130, -1), 5: (0, S)}),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make_case(dk, layout):
    lens, done, bad = LAYOUTS[layout]
    d = H * dk
    rs = np.random.RandomState(100 * dk + len(layout))
    ld, ld_row, ldo, ld_src = 3 * d + 8, d + 8, d + 4, CAP + 5
    ld_seq = CAP * ld_row + 12
    ld_layer = S * ld_seq + 4
    qkv = np.full((S + 1, ld), np.nan, np.float32)
    qkv[:S, :3 * d] = rs.randn(S, 3 * d).astype(np.float32) * np.float32(0.5)
    K = np.full((LAYERS, ld_layer), np.nan, np.float32)
    V = np.full((LAYERS, ld_layer), np.nan, np.float32)
    src = np.empty((S, ld_src), np.int32)
    src[:] = rs.choice([-7, S, S + 3, 2 ** 31 - 1, -2 ** 31], size=src.shape)          # entries at u >= len: never read
    row = lambda plane, slot, u: plane[LAYER, slot * ld_seq + u * ld_row:slot * ld_seq + u * ld_row + d]
    for s in range(S):
        b = s // BEAM
        longer = [x for x in range(b * BEAM, (b + 1) * BEAM) if lens[x] >= lens[s]]
        for u in range(lens[s]):
            slot = b * BEAM if u < PROMPT[b] else longer[int(rs.randint(len(longer)))]
            src[s, u] = slot
            if np.isnan(row(K, slot, u)[0]):
                row(K, slot, u)[:] = rs.randn(d).astype(np.float32) * np.float32(0.3 * np.sqrt(128.0 / dk))
                row(V, slot, u)[:] = rs.randn(d).astype(np.float32)
    good = src.copy()
    for s, (u, v) in bad.items():
        src[s, u] = v
    return dict(dk=dk, d=d, lens=np.asarray(lens, np.int32), done=np.asarray(done, np.int32), bad=bad, qkv=qkv, K=K, V=V, src=src, good=good,
                ld=ld, ld_row=ld_row, ld_seq=ld_seq, ld_layer=ld_layer, ldo=ldo, ld_src=ld_src)


class Call:
    def __init__(self, c, dev, contiguous=False):
        """contiguous: the reference -- gnnlm_decode_attn over a cache holding row u of hypothesis s at (s, u), gathered with torch."""
        from gnnlm_amd import _lib
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.c, self.contiguous = c, contiguous
        d = c["d"]
        self.qkv, self.K, self.V = t(c["qkv"]), t(c["K"]), t(c["V"])
        self.lens, self.done, self.src = t(c["lens"]), t(c["done"]), t(c["src"])
        if contiguous:
            view = lambda x: x[:, :S * c["ld_seq"]].view(LAYERS, S, c["ld_seq"])[:, :, :CAP * c["ld_row"]].view(LAYERS, S, CAP, c["ld_row"])
            idx = t(c["good"][:, :CAP].astype(np.int64))                                 # [S, CAP], garbage beyond len
            u_ok = torch.arange(CAP, device=dev)[None, :] < self.lens[:, None].long()
            idx = torch.where(u_ok, idx, torch.arange(S, device=dev)[:, None].expand(S, CAP))
            for plane in (self.K, self.V):
                rows = view(plane)[LAYER]                                                # [S, CAP, ld_row]
                new = rows[idx, torch.arange(CAP, device=dev)[None, :].expand(S, CAP)]   # row u of slot idx[s, u]
                rows.copy_(torch.where(u_ok[:, :, None], new, rows))
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = torch.full((S, c["ldo"]), SENTINEL, device=dev)
        need = _lib.lib().gnnlm_decode_attn_workspace_bytes(S, H, c["dk"], CAP)
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev)
        self.desc = _lib.gnnlm_beam_attn_t()
        a = self.desc.a
        a.q, a.k_new, a.v_new, a.ld = self.qkv.data_ptr(), self.qkv.data_ptr() + 4 * d, self.qkv.data_ptr() + 8 * d, c["ld"]
        a.out, a.ldo = self.out.data_ptr(), c["ldo"]
        a.cache.k, a.cache.v = self.K.data_ptr(), self.V.data_ptr()
        a.cache.ld_row, a.cache.ld_seq, a.cache.ld_layer = c["ld_row"], c["ld_seq"], c["ld_layer"]
        a.cache.L, a.cache.B, a.cache.cap, a.cache.d = LAYERS, S, CAP, d
        a.cache.len, a.cache.done, a.cache.n_bad = self.lens.data_ptr(), self.done.data_ptr(), self.n_bad.data_ptr()
        a.layer, a.H, a.dk, a.max_len = LAYER, H, c["dk"], 0
        a.workspace, a.workspace_bytes = self.ws.data_ptr(), need
        self.desc.src, self.desc.ld_src = self.src.data_ptr(), c["ld_src"]

    def run(self):
        from gnnlm_amd import _lib
        L = _lib.lib()
        rc = L.gnnlm_decode_attn(ctypes.byref(self.desc.a), _lib.stream()) if self.contiguous else L.gnnlm_beam_attn(ctypes.byref(self.desc), _lib.stream())
        torch.cuda.synchronize()
        return rc

    def result(self):
        return self.out.cpu().numpy(), self.K.cpu().numpy(), self.V.cpu().numpy(), int(self.n_bad.item())


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dk", [16, 128])
def test_beam_attn_is_decode_attn_on_the_gathered_cache(dev, dk, layout):
    c = make_case(dk, layout)
    d = c["d"]
    ref = Call(c, dev, contiguous=True)
    assert ref.run() == 0
    want = ref.result()[0]
    call = Call(c, dev)
    assert call.run() == 0
    out, K, V, n_bad = call.result()
    zero = [s for s in range(S) if c["done"][s] or s in c["bad"]]
    live = [s for s in range(S) if s not in zero]
    assert np.isfinite(out[live, :d]).all() and np.abs(out[live, :d]).max() > 0
    assert np.array_equal(bits(out[live, :d]), bits(want[live, :d]))
    # a done row and a row with a table entry outside [0, B) below len: zeros; only the latter is counted
    assert not out[zero, :d].any() and n_bad == len(c["bad"]) and (out[:, d:] == SENTINEL).all()
    # the new row lands in slot s, row len[s] (not for the done row); no other cache byte changes
    K2, V2 = c["K"].copy(), c["V"].copy()
    for s in range(S):
        if not c["done"][s]:
            o = s * c["ld_seq"] + int(c["lens"][s]) * c["ld_row"]
            K2[LAYER, o:o + d], V2[LAYER, o:o + d] = c["qkv"][s, d:2 * d], c["qkv"][s, 2 * d:3 * d]
    assert np.array_equal(bits(K), bits(K2)) and np.array_equal(bits(V), bits(V2))
    assert np.array_equal(call.lens.cpu().numpy(), c["lens"]) and np.array_equal(call.src.cpu().numpy(), c["src"])
    # again: the same bits
    assert call.run() == 0
    assert np.array_equal(bits(call.result()[0]), bits(out))


def test_ops_wrapper_and_refusals(dev):
    from gnnlm_amd import _lib, ops
    c = make_case(16, "edges")
    d = c["d"]
    call = Call(c, dev)
    assert call.run() == 0
    want, K0, V0, _ = call.result()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    view = lambda a: t(a)[:, :S * c["ld_seq"]].view(LAYERS, S, c["ld_seq"])[:, :, :CAP * c["ld_row"]].view(LAYERS, S, CAP, c["ld_row"])[..., :d]
    qkv = t(c["qkv"])
    got = ops.beam_attn(qkv[:S, :d], qkv[:S, d:2 * d], qkv[:S, 2 * d:3 * d], view(c["K"]), view(c["V"]), t(c["lens"]), t(c["src"]), LAYER, H,
                        done=t(c["done"]))
    assert np.array_equal(bits(got.cpu().numpy()), bits(want[:, :d]))
    with pytest.raises(TypeError):
        ops.beam_attn(qkv[:S, :d], qkv[:S, d:2 * d], qkv[:S, 2 * d:3 * d], view(c["K"]), view(c["V"]), t(c["lens"]), t(c["src"]).long(), LAYER, H)

    def refused(edit, match):
        x = Call(c, dev)
        edit(x.desc)
        assert x.run() == -22
        assert match in _lib.lib().gnnlm_last_error().decode()
        out, K, V, bad = x.result()
        assert (out == SENTINEL).all() and bad == 0 and np.array_equal(bits(K), bits(c["K"])) and np.array_equal(bits(V), bits(c["V"]))

    refused(lambda b: setattr(b, "src", None), "src")
    refused(lambda b: setattr(b, "src", b.src + 2), "src")
    refused(lambda b: setattr(b, "ld_src", CAP - 1), "ld_src")
    refused(lambda b: setattr(b.a, "dk", 24), "d_k must be 16, 32, 64 or 128")
    refused(lambda b: setattr(b.a, "max_len", CAP + 1), "max_len")
    refused(lambda b: setattr(b.a, "workspace", None), "workspace")
    assert _lib.lib().gnnlm_beam_attn(None, _lib.stream()) == -22
    x = Call(c, dev)
    x.desc.a.cache.B = 0
    x.desc.src = None
    assert x.run() == 0 and (x.result()[0] == SENTINEL).all()
