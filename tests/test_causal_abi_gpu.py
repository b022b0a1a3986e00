"""The causal ('tgt','intra','tgt') attention at the call level (include/gnnlm.h): gnnlm_causal_attn (the fused 256 x 128 kernel),
gnnlm_causal_attn_varlen with a hand-filled gnnlm_ragged_t, and gnnlm_causal_softmax, each called through ``_lib.call`` -- the ``ops``
wrappers are not used -- against the float64 restatement of tests/causal_ref.py.

The case tables, their inputs, the bars and the mutations live in causal_ref.py; tests/test_causal_ref_cpu.py shows without a GPU that every
case takes the route written next to it, that a kernel with a window off by one, a block boundary off by one, another head's K, a lost
diagonal or a lost key tile would miss the bar of a ``flat`` case by a factor of 100, that ``high`` / ``low`` need the maximum subtracted,
and that no table handed to a kernel points outside the buffers allocated here.

Per case: the result within the case's bar (printed with the achieved error), a second call with the same bits, and every element the
kernel must not write -- the columns behind H * dk of an output row, the guard behind the buffer, the rows of skipped table entries --
still the NaN sentinel, compared as bits.  Apart-ness (blocks, future keys, keys below the window, heads) is bit-exact on ``flat`` inputs:
what is overwritten is finite, so a masked probability of exactly 0 times it stays 0.

The ``accumulate`` flag of the two launchers is not reachable through the C ABI; it stays covered through gnnlm_hgt_forward only."""
import ctypes

import numpy as np
import pytest
import torch

import causal_ref as ref

pytestmark = pytest.mark.gpu

SENT_BITS = 0x7FC0BEEF                                                        # a NaN with a payload of its own
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sentinel(n, dev):
    return torch.from_numpy(np.full(n, SENT_BITS, dtype=np.uint32).view(np.float32)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_REF = {}


def reference(c):
    """(case arrays, float64 result, bar) of a table case, computed once"""
    key = ref.attn_case_id(c)
    if key not in _REF:
        a = ref.make_attn_case(c)
        _REF[key] = (a, ref.causal_ref(a["Q"], a["K"], a["V"], a["lengths"], a["H"], a["max_ctx"]), ref.attn_bar(c, a))
    return _REF[key]


class Run:
    """The arguments of one call of gnnlm_causal_attn (route "fused") or gnnlm_causal_attn_varlen over the arrays of a case of
    causal_ref.make_attn_case, in ``g`` (a test may change any of them before ``call``), with the device tensors they point to.  buf / tiles
    replace the case's; off is a block-offset table handed over as it is (default: the case's, from entry OFF0 on); ``out`` gets out_rows rows
    of ldo elements and GUARD more, all sentinel."""

    def __init__(self, dev, a, route, buf=None, tiles=None, off=None, out_rows=None):
        self.dev, self.route, self.a = dev, route, a
        self.buf = torch.from_numpy(np.ascontiguousarray(a["buf"] if buf is None else buf)).to(dev)
        d, base = a["H"] * a["dk"], self.buf.data_ptr()
        self.out_rows = a["n_tok"] if out_rows is None else out_rows
        g = self.g = dict(Q=base, K=base + 4 * d, V=base + 8 * d, ld=a["ld"], ldo=a["ldo"], H=a["H"], dk=a["dk"], max_ctx=a["max_ctx"], out_shift=0)
        if route == "fused":
            g.update(n_blocks=len(a["lengths"]), T=ref.FUSED_T)
        else:
            tiles = a["tiles"] if tiles is None else tiles
            self.table = torch.from_numpy(np.array(a["table"] if off is None else off, dtype=np.int32)).to(dev)
            self.tiles = torch.from_numpy(np.array(tiles, dtype=np.int32)).to(dev)
            g.update(block_off=self.table.data_ptr() + (4 * ref.OFF0 if off is None else 0), tiles=self.tiles.data_ptr(),
                     n_blocks=len(a["lengths"]), n_tiles=len(tiles), n_tok=a["n_tok"])

    def call(self):
        """-> (out [out_rows, ldo], guard) as numpy"""
        from gnnlm_amd import _lib
        g, n = self.g, self.out_rows * self.a["ldo"]
        out = self.out = sentinel(n + GUARD, self.dev)
        po = out.data_ptr() + g["out_shift"] if g.get("out", 1) is not None else None
        if self.route == "fused":
            _lib.call("gnnlm_causal_attn", g["Q"], g["K"], g["V"], g["ld"], po, g["ldo"], g["n_blocks"], g["T"], g["H"], g["dk"], g["max_ctx"],
                      _lib.stream())
        else:
            desc = _lib.gnnlm_ragged_t()
            desc.block_off, desc.tiles = g["block_off"], g["tiles"]
            desc.n_blocks, desc.n_tiles, desc.n_tok = g["n_blocks"], g["n_tiles"], g["n_tok"]
            _lib.call("gnnlm_causal_attn_varlen", g["Q"], g["K"], g["V"], g["ld"], po, g["ldo"], ctypes.byref(desc), g["H"], g["dk"], g["max_ctx"],
                      _lib.stream())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        return out[:n].reshape(self.out_rows, self.a["ldo"]), out[n:]


def check(tag, out, guard, a, want, bar):
    """the result within the bar; nothing written behind the H * dk columns of a row or behind the buffer"""
    d = a["H"] * a["dk"]
    got = out[:a["n_tok"], :d]
    assert not np.isnan(got).any(), tag                                       # an element not written, or a row no rule reads was read
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{tag}: max |out - ref| = {err:.3e}   bar = {bar:.3e}")
    assert err < bar, tag
    assert (bits(out[:, d:]) == SENT_BITS).all() and (bits(guard) == SENT_BITS).all(), tag
    return err


# ======================================================================================================== the fused kernel
@pytest.mark.parametrize("case", ref.FUSED_CASES, ids=ref.attn_case_id)
def test_causal_attn_fused_call(dev, case):
    a, want, bar = reference(case)
    r = Run(dev, a, "fused")
    out, guard = r.call()
    check(ref.attn_case_id(case), out, guard, a, want, bar)
    out2, guard2 = r.call()
    assert np.array_equal(bits(out), bits(out2)) and (bits(guard2) == SENT_BITS).all()


# ======================================================================================================== the varlen kernel
def test_ragged_tiles_restated(dev):
    """causal_ref.ragged_tiles (what the CPU checks walk) is what gnnlm_ragged_tiles writes"""
    from gnnlm_amd import _lib
    for lengths in ref.VARLEN_LENGTHS + [[257, 40, 1, 64]]:
        off = np.concatenate([[19], 19 + np.cumsum(lengths)]).astype(np.int32)
        want = ref.ragged_tiles(lengths)
        assert _lib.lib().gnnlm_ragged_tiles(off.ctypes.data, len(lengths), None) == len(want)
        got = np.full_like(want, -7)
        assert _lib.lib().gnnlm_ragged_tiles(off.ctypes.data, len(lengths), got.ctypes.data) == len(want)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("case", ref.VARLEN_CASES, ids=ref.attn_case_id)
def test_causal_attn_varlen_call(dev, case):
    a, want, bar = reference(case)
    first = None
    for name, tiles in ref.tile_orders(a["tiles"]):
        r = Run(dev, a, "varlen", tiles=tiles)
        out, guard = r.call()
        if first is None:
            check(ref.attn_case_id(case), out, guard, a, want, bar)
            first = out
            out2, guard2 = r.call()
            assert np.array_equal(bits(out), bits(out2)) and (bits(guard2) == SENT_BITS).all()
        else:                                                                 # a work list: the same bits in any order
            assert np.array_equal(bits(out), bits(first)) and (bits(guard) == SENT_BITS).all(), name


@pytest.mark.parametrize("case", ref.CROSS_ROUTE_CASES, ids=ref.attn_case_id)
def test_both_routes_of_the_shared_shape(dev, case):
    """[256, 256] at d_k = 128 through the fused kernel and through the varlen kernel: each within its bar of the same reference"""
    a, want, bar = reference(case)
    for route in ("fused", "varlen"):
        out, guard = Run(dev, a, route).call()
        check(f"{route} <- {ref.attn_case_id(case)}", out, guard, a, want, bar)


# ------------------------------------------------------------------------------------------ apart-ness, bit-exact
APART = [("fused", dict(route="fused", n_blocks=3, H=2, max_ctx=0, ldo_pad=12, profile="flat")),
         ("varlen", dict(route="varlen", lengths=[64, 65, 97], dk=32, H=2, max_ctx=0, ldo_pad=12, profile="flat")),
         ("varlen", dict(route="varlen", lengths=[257, 40], dk=128, H=2, max_ctx=0, ldo_pad=0, profile="flat"))]
APART_IDS = [ref.attn_case_id(c) for _, c in APART]


def blocks_of(a):
    off = np.concatenate([[0], np.cumsum(a["lengths"])])
    return [(int(off[b]), int(off[b + 1])) for b in range(len(a["lengths"]))]


def overwritten(a, rows, cols, salt):
    """a copy of the case's buffer with 3 * randn in the given rows (bool [n_tok]) and columns (bool [ld])"""
    buf = a["buf"].copy()
    rs = np.random.RandomState(salt)
    sel = np.zeros(buf.shape, dtype=bool)
    sel[:a["n_tok"]] = rows[:, None] & cols[None, :]
    buf[sel] = (3 * rs.randn(int(sel.sum()))).astype(np.float32)
    assert np.isfinite(buf[sel]).all()
    return buf


def columns(a, which="QKV", head=None):
    d, dk = a["H"] * a["dk"], a["dk"]
    cols = np.zeros(a["ld"], dtype=bool)
    for j, name in enumerate("QKV"):
        if name in which:
            cols[j * d + (0 if head is None else head * dk):(j * d + d) if head is None else j * d + (head + 1) * dk] = True
    return cols


def run_with(dev, a, route, max_ctx, buf=None):
    r = Run(dev, a, route, buf=buf)
    r.g["max_ctx"] = max_ctx
    out, guard = r.call()
    assert (bits(guard) == SENT_BITS).all()
    return out[:, :a["H"] * a["dk"]]


@pytest.mark.parametrize("route,case", APART, ids=APART_IDS)
def test_blocks_stay_apart(dev, route, case):
    a = ref.make_attn_case(case)
    for ctx in (0, 33):
        base = run_with(dev, a, route, ctx)
        for b, (r0, r1) in enumerate(blocks_of(a)):
            rows = np.zeros(a["n_tok"], dtype=bool)
            rows[r0:r1] = True
            got = run_with(dev, a, route, ctx, overwritten(a, rows, columns(a), b))
            assert np.array_equal(bits(got[~rows]), bits(base[~rows])), (ctx, b)
            assert not np.array_equal(bits(got[rows]), bits(base[rows]))      # (the overwrite reached the kernel)


@pytest.mark.parametrize("route,case", APART, ids=APART_IDS)
def test_future_keys_stay_unseen(dev, route, case):
    a = ref.make_attn_case(case)
    base = run_with(dev, a, route, 0)
    for w0 in (0, 31, 32, 40, "T-2"):
        rows, safe = np.zeros(a["n_tok"], dtype=bool), np.zeros(a["n_tok"], dtype=bool)
        for r0, r1 in blocks_of(a):
            w = r1 - r0 - 2 if w0 == "T-2" else w0
            if 0 <= w < r1 - r0 - 1:
                rows[r0 + w + 1:r1] = True
                safe[r0:r0 + w + 1] = True
        assert rows.any()
        got = run_with(dev, a, route, 0, overwritten(a, rows, columns(a, "KV"), 7))
        assert np.array_equal(bits(got[safe]), bits(base[safe])), w0
        assert not np.array_equal(bits(got[rows]), bits(base[rows]))


@pytest.mark.parametrize("route,case", APART, ids=APART_IDS)
def test_keys_below_the_window_stay_unseen(dev, route, case):
    """with max_ctx = c, K and V rows below a do not reach out[w] for any w >= a + c - 1 (a = 20 and 40, or as far up as the longest block
    still has such a w: 32 for c = 65 on 97 tokens)"""
    a = ref.make_attn_case(case)
    for c in (1, 32, 33, 65):
        base = run_with(dev, a, route, c)
        for lo in (20, min(40, max(a["lengths"]) - c)):
            rows, safe = np.zeros(a["n_tok"], dtype=bool), np.zeros(a["n_tok"], dtype=bool)
            for r0, r1 in blocks_of(a):
                if r1 - r0 > lo:
                    rows[r0:r0 + lo] = True
                    safe[min(r0 + lo + c - 1, r1):r1] = True
            assert rows.any() and safe.any()
            got = run_with(dev, a, route, c, overwritten(a, rows, columns(a, "KV"), 11))
            assert np.array_equal(bits(got[safe]), bits(base[safe])), (c, lo)
            assert not np.array_equal(bits(got[rows]), bits(base[rows]))


@pytest.mark.parametrize("route,case", APART[:2] + [("varlen", dict(route="varlen", lengths=[64, 65, 97], dk=16, H=8, max_ctx=0, ldo_pad=0, profile="flat"))],
                         ids=APART_IDS[:2] + ["varlen-64+65+97-dk16-H8"])
def test_heads_stay_apart(dev, route, case):
    a = ref.make_attn_case(case)
    dk, every = a["dk"], np.ones(a["n_tok"], dtype=bool)
    base = run_with(dev, a, route, 0)
    for h in range(a["H"]):
        got = run_with(dev, a, route, 0, overwritten(a, every, columns(a, head=h), h))
        mine = np.zeros(a["H"] * dk, dtype=bool)
        mine[h * dk:(h + 1) * dk] = True
        assert np.array_equal(bits(got[:, ~mine]), bits(base[:, ~mine])), h
        assert not np.array_equal(bits(got[:, mine]), bits(base[:, mine]))


# ------------------------------------------------------------------------------------------ the tile-table contract
CONTRACT = dict(route="varlen", lengths=ref.CONTRACT_LENGTHS, dk=16, H=2, max_ctx=0, ldo_pad=12, profile="flat")


def test_varlen_skips_entries_that_name_no_rows(dev):
    """"A table entry that does not describe rows of [0, n_tok) is skipped by the kernel, never followed" (gnnlm.h): one entry more, naming
    no block, a block past the last, no tile, or a tile past its block's end, changes nothing."""
    a, want, bar = reference(CONTRACT)
    out, guard = Run(dev, a, "varlen").call()
    check("varlen contract, plain", out, guard, a, want, bar)
    for extra in ref.CONTRACT_EXTRA:
        tiles = np.insert(a["tiles"], ref.CONTRACT_AT, extra, axis=0)
        assert len(tiles) == len(a["tiles"]) + 1
        got, guard = Run(dev, a, "varlen", tiles=tiles).call()
        assert np.array_equal(bits(got), bits(out)) and (bits(guard) == SENT_BITS).all(), extra


def test_varlen_skips_a_block_that_claims_rows_past_n_tok(dev):
    """The last block of the table claims rows 24 .. 40 of a call that declares n_tok = 32: skipped, its rows of ``out`` keep the sentinel
    (the buffers hold 48 rows, finite poison behind the tokens: a kernel that followed the entry would be seen, not fault)."""
    a, _, _ = reference(CONTRACT)
    d = a["H"] * a["dk"]
    base, _ = Run(dev, a, "varlen").call()
    buf = np.full((ref.OVERCLAIM_ROWS, a["ld"]), np.nan, dtype=np.float32)
    buf[:, :3 * d] = ref.POISON
    buf[:a["n_tok"]] = a["buf"][:a["n_tok"]]
    r = Run(dev, a, "varlen", buf=buf, off=ref.OVERCLAIM_OFF, out_rows=ref.OVERCLAIM_ROWS)
    assert r.g["n_tok"] == ref.OVERCLAIM_N_TOK and r.g["n_blocks"] == len(ref.OVERCLAIM_OFF) - 1
    out, guard = r.call()
    assert np.array_equal(bits(out[:24]), bits(base[:24]))
    assert (bits(out[24:]) == SENT_BITS).all() and (bits(guard) == SENT_BITS).all()


# ------------------------------------------------------------------------------------------ refusals
def refused(r, **fields):
    from gnnlm_amd._lib import GnnlmError
    r.g.update(fields)
    with pytest.raises(GnnlmError):
        r.call()
    torch.cuda.synchronize()
    assert (bits(r.out.cpu().numpy()) == SENT_BITS).all(), fields           # nothing was written


def test_fused_refusals(dev):
    """Every descriptor here is one argument away from a call that runs, and is refused by the launcher before any launch (the buffers are
    large enough for what it claims all the same: SLACK_ROWS rows more than the tokens)."""
    a = ref.make_attn_case(dict(route="fused", n_blocks=1, H=2, max_ctx=0, ldo_pad=12, profile="flat"))
    d = a["H"] * a["dk"]
    new = lambda: Run(dev, a, "fused")
    new().call()
    refused(new(), T=255)
    refused(new(), T=64)
    refused(new(), dk=64)
    refused(new(), ld=a["ld"] + 2)                                            # ld % 4 != 0
    r = new()
    refused(r, Q=r.g["Q"] + 4)                                                # not 16-byte aligned
    r = new()
    refused(r, K=r.g["K"] + 8)
    r = new()
    refused(r, V=r.g["V"] + 4)
    for name in ("Q", "K", "V", "out"):
        refused(new(), **{name: None})
    refused(new(), H=0)
    refused(new(), H=-1)
    refused(new(), n_blocks=-1)
    refused(new(), n_blocks=1 << 30)                                          # n_blocks * H does not fit the grid
    refused(new(), ld=d - 4)                                                  # ld < H * dk
    refused(new(), ldo=d - 4)                                                 # ldo < H * dk


def test_varlen_refusals(dev):
    """Every GNNLM_REQUIRE of causal_attn_varlen, each one argument away from a call that runs."""
    a = ref.make_attn_case(CONTRACT)
    d = a["H"] * a["dk"]
    new = lambda: Run(dev, a, "varlen")
    new().call()
    for name in ("Q", "K", "V", "out"):
        refused(new(), **{name: None})
    refused(new(), dk=24)
    refused(new(), dk=0)
    refused(new(), H=0)
    refused(new(), n_blocks=-1)
    refused(new(), n_tiles=-1)
    refused(new(), n_tok=-1)
    refused(new(), n_tok=1 << 31)
    refused(new(), ld=a["ld"] + 2)                                            # ld % 4 != 0
    refused(new(), ldo=a["ldo"] + 2)                                          # ldo % 4 != 0
    refused(new(), ld=d - 4)
    refused(new(), ldo=d - 4)
    for name in ("Q", "K", "V"):
        r = new()
        refused(r, **{name: r.g[name] + 4})                                   # not 16-byte aligned
    refused(new(), out_shift=4)
    refused(new(), block_off=None)
    refused(new(), tiles=None)
    refused(new(), n_tok=3)                                                   # more blocks than tokens
    refused(new(), n_tiles=3)                                                 # fewer tiles than blocks
    refused(new(), n_tiles=6)                                                 # more than n_tok / 32 + n_blocks


# ======================================================================================================== gnnlm_causal_softmax
def softmax_call(dev, S, T, ld, n_mats, max_ctx):
    """-> (S after the call [n_mats, T, ld], guard); S may be None (a NULL pointer is handed over)"""
    from gnnlm_amd import _lib
    n = 0 if S is None else S.size
    t = sentinel(n + GUARD, dev)
    if S is not None:
        t[:n] = torch.from_numpy(S.reshape(-1)).to(dev)
    before = t.cpu().numpy()
    try:
        _lib.call("gnnlm_causal_softmax", None if S is None else t.data_ptr(), n_mats, T, ld, max_ctx, _lib.stream())
    finally:
        torch.cuda.synchronize()
        softmax_call.after, softmax_call.before = t.cpu().numpy(), before
    out = softmax_call.after
    return out[:n].reshape(S.shape), out[n:]


@pytest.mark.parametrize("case", ref.SOFTMAX_CASES, ids=ref.softmax_case_id)
def test_causal_softmax_call(dev, case):
    T, ld, m, ctx = case["T"], case["ld"], case["n_mats"], case["max_ctx"]
    S = ref.make_softmax_case(case)
    want, bar = ref.softmax_ref(S, T, ctx), ref.softmax_bar(case, S)
    got, guard = softmax_call(dev, S, T, ld, m, ctx)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{ref.softmax_case_id(case)}: max |P - ref| = {err:.3e}   bar = {bar:.3e}")
    assert err < bar
    assert (bits(got[want == 0]) == 0).all()                                  # outside the window and in the padding T .. ld: exactly zero
    assert (want[:, :, T:] == 0).all() and (want > 0).sum() == m * sum(min(w + 1, ctx) if ctx > 0 else w + 1 for w in range(T))
    assert np.abs(got.astype(np.float64).sum(-1) - 1).max() < 1e-6
    assert (bits(guard) == SENT_BITS).all()
    got2, guard2 = softmax_call(dev, S, T, ld, m, ctx)
    assert np.array_equal(bits(got), bits(got2)) and (bits(guard2) == SENT_BITS).all()


def test_softmax_refusals(dev):
    from gnnlm_amd._lib import GnnlmError
    S = ref.make_softmax_case(dict(T=5, ld=8, n_mats=3, max_ctx=0, shift=0.0))
    softmax_call(dev, S, 5, 8, 3, 0)
    for T, ld, m, s in [(9, 8, 1, S), (0, 8, 3, S), (-1, 8, 3, S), (5, 8, -1, S), (5, 8, -3, S), (5, 8, 3, None)]:   # ld < T; T <= 0; n_mats < 0; NULL
        with pytest.raises(GnnlmError):
            softmax_call(dev, s, T, ld, m, 0)
        assert np.array_equal(bits(softmax_call.after), bits(softmax_call.before))       # nothing was written
