"""tests/causal_ref.py is right before it judges a kernel, and the cases of tests/test_causal_abi_gpu.py can tell a wrong kernel from a
right one.  No GPU.

1. causal_ref / softmax_ref equal explicit loops over (w, u) with math.exp to 1e-12; ragged_tiles is the order the header states.
2. The bars: 2e-5 on ``flat``; max(2e-5, 4 * e32) on every other profile, e32 = max |causal_f32 - causal_ref| of the case, printed.
3. Sensitivity: on every ``flat`` case each listed mutation of the reference's arguments moves the float64 result by at least 100 x the
   case's bar somewhere, and on every ``falling`` case with max_ctx > 0, max_ctx +- 1 does.  (``rising`` is dominated by the newest keys
   and carries no window sensitivity: that is what ``falling`` and ``flat`` are for.)
4. A float32 restatement without the maximum subtracted is not finite on ``high`` and ``low``: those cases would catch its loss.
5. Every table entry takes the route written next to it, and the tables hold every value the kernels branch on.
6. No table, tile or block offset handed to a kernel addresses memory outside the buffers the GPU test allocates."""
import math

import numpy as np
import pytest

import causal_ref as ref

FAR = 100


# ------------------------------------------------------------------------------------------ 1. the references
def loop_attn(Q, K, V, lengths, H, max_ctx):
    n_tok, d = Q.shape
    dk = d // H
    out, r0 = np.zeros((n_tok, d)), 0
    for n in lengths:
        for w in range(n):
            for h in range(H):
                us = [u for u in range(n) if u <= w and (max_ctx == 0 or w - u < max_ctx)]
                sc = [sum(float(Q[r0 + w, h * dk + e]) * float(K[r0 + u, h * dk + e]) for e in range(dk)) for u in us]
                m = max(sc)
                ex = [math.exp(s - m) for s in sc]
                for e in range(dk):
                    out[r0 + w, h * dk + e] = sum(x * float(V[r0 + u, h * dk + e]) for x, u in zip(ex, us)) / sum(ex)
        r0 += n
    return out


@pytest.mark.parametrize("case", [dict(route="varlen", lengths=[5, 1, 9], dk=16, H=2, max_ctx=0, ldo_pad=0, profile="flat"),
                                  dict(route="varlen", lengths=[7, 34], dk=16, H=3, max_ctx=4, ldo_pad=12, profile="falling")], ids=ref.attn_case_id)
def test_causal_ref_is_the_explicit_loop(case):
    a = ref.make_attn_case(case)
    args = (a["Q"], a["K"], a["V"], a["lengths"], a["H"], a["max_ctx"])
    assert np.abs(ref.causal_ref(*args) - loop_attn(*args)).max() < 1e-12
    assert np.abs(ref.causal_f32(*args) - loop_attn(*args)).max() < 1e-4      # (the float32 restatement states the same rule)


@pytest.mark.parametrize("T,ld,max_ctx", [(5, 8, 0), (9, 9, 3)])
def test_softmax_ref_is_the_explicit_loop(T, ld, max_ctx):
    S = ref.make_softmax_case(dict(T=T, ld=ld, n_mats=2, max_ctx=max_ctx, shift=-200.0))
    want = np.zeros(S.shape)
    for m in range(2):
        for w in range(T):
            us = [u for u in range(T) if u <= w and (max_ctx == 0 or w - u < max_ctx)]
            mx = max(float(S[m, w, u]) for u in us)
            den = sum(math.exp(float(S[m, w, u]) - mx) for u in us)
            for u in us:
                want[m, w, u] = math.exp(float(S[m, w, u]) - mx) / den
    assert np.abs(ref.softmax_ref(S, T, max_ctx) - want).max() < 1e-12


def test_ragged_tiles_order():
    t = ref.ragged_tiles([257, 40, 1, 64]).tolist()
    assert t == [[0, 8], [0, 7], [0, 6], [0, 5], [0, 4], [0, 3], [0, 2], [0, 1], [1, 1], [3, 1], [0, 0], [1, 0], [2, 0], [3, 0]]


# ------------------------------------------------------------------------------------------ 2. bars
def test_bars():
    print()
    for c in ref.FUSED_CASES + ref.VARLEN_CASES:
        if c["profile"] == "flat":
            assert ref.attn_bar(c) == ref.TOL == 2e-5
            continue
        e32, bar = ref.attn_e32(c), ref.attn_bar(c)
        print(f"{ref.attn_case_id(c):60s} e32 = {e32:.2e}   bar = {bar:.2e}")
        assert 0 < e32 < 1e-3 and bar == max(2e-5, 4 * e32)                   # (1e-3: a restatement that far off states another rule)
    worst = {}
    for c in ref.SOFTMAX_CASES:
        if c["shift"] == 0:
            assert ref.softmax_bar(c) == 1e-6
        else:
            e32 = ref.softmax_e32(c)
            worst[c["shift"]] = max(worst.get(c["shift"], 0.0), e32)
            assert ref.softmax_bar(c) == max(1e-6, 4 * e32)
    for sh, e in worst.items():
        print(f"softmax, scores randn {sh:+.0f}: largest e32 = {e:.2e}   bar = {max(1e-6, 4 * e):.2e}")


# ------------------------------------------------------------------------------------------ 3. sensitivity
def moved(a, kw):
    base = ref.causal_ref(a["Q"], a["K"], a["V"], a["lengths"], a["H"], a["max_ctx"])
    return float(np.abs(ref.causal_ref(**kw) - base).max())


@pytest.mark.parametrize("case", [c for c in ref.FUSED_CASES + ref.VARLEN_CASES if c["profile"] == "flat"], ids=ref.attn_case_id)
def test_flat_cases_feel_every_mutation(case):
    a = ref.make_attn_case(case)
    muts = ref.attn_mutations(a)
    longest, ctx = max(a["lengths"]), a["max_ctx"]
    eff = longest if ctx == 0 else min(ctx, longest)
    # the list is what the rules of attn_mutations give: nothing is dropped because it failed to move the result
    want = (ctx == 0 and longest >= 2) + (ctx >= 2 and ctx - 1 < longest) + (0 < ctx < longest) + \
        (eff >= 2) * (1 + (len(a["lengths"]) > 1) + (a["H"] > 1) + (longest > 32))
    assert len(muts) == want
    for what, kw in muts:
        assert moved(a, kw) >= FAR * ref.attn_bar(case), what


@pytest.mark.parametrize("case", [c for c in ref.FUSED_CASES + ref.VARLEN_CASES if c["profile"] == "falling" and c["max_ctx"] > 0],
                         ids=ref.attn_case_id)
def test_falling_cases_feel_the_window(case):
    a = ref.make_attn_case(case)
    muts = [m for m in ref.attn_mutations(a) if m[0].startswith("max_ctx")]
    assert len(muts) == 2
    for what, kw in muts:
        assert moved(a, kw) >= FAR * ref.attn_bar(case, a), what


# ------------------------------------------------------------------------------------------ 4. the maximum
@pytest.mark.parametrize("case", [c for c in ref.FUSED_CASES + ref.VARLEN_CASES if c["profile"] in ("high", "low")], ids=ref.attn_case_id)
def test_high_and_low_need_the_maximum(case):
    a = ref.make_attn_case(case)
    args = (a["Q"], a["K"], a["V"], a["lengths"], a["H"], a["max_ctx"])
    assert np.isfinite(ref.causal_f32(*args)).all()
    assert not np.isfinite(ref.causal_f32(*args, subtract_max=False)).all()


# ------------------------------------------------------------------------------------------ 5. routes and coverage
def kt_lo(q0, ctx):
    return max(0, q0 - ctx + 1) // 32 if ctx > 0 else 0


def test_tables_take_their_routes_and_cover_every_value():
    ids = [ref.attn_case_id(c) for c in ref.FUSED_CASES + ref.VARLEN_CASES]
    assert len(set(ids)) == len(ids)
    for c in ref.FUSED_CASES:
        assert ref.attn_route(ref.FUSED_T, ref.FUSED_DK) == c["route"] == "fused"
    for c in ref.VARLEN_CASES:
        assert ref.attn_route(c["lengths"], c["dk"]) == c["route"]
        assert (c["H"] * c["dk"] + c["ldo_pad"]) % 4 == 0
    assert ref.attn_route(64, 128) == ref.attn_route(256, 64) == "" and ref.attn_route([8], 24) == ""
    flat = [c for c in ref.FUSED_CASES if c["profile"] == "flat"]
    assert {(c["n_blocks"], c["H"]) for c in flat} == set(ref.FUSED_SHAPES) and {c["max_ctx"] for c in flat} == set(ref.FUSED_CTX)
    assert {c["ldo_pad"] for c in flat} == {0, 12}
    flat = [c for c in ref.VARLEN_CASES if c["profile"] == "flat"]
    assert {(tuple(c["lengths"]), c["max_ctx"]) for c in flat} >= {(tuple(l), x) for l in ref.VARLEN_LENGTHS for x in ref.VARLEN_CTX}
    assert {c["dk"] for c in flat} == {16, 32, 64, 128} and {c["H"] for c in flat} == {1, 2, 8}
    assert {(c["dk"], c["ldo_pad"]) for c in flat} == {(dk, p) for dk in ref.VARLEN_DK for p in (0, 12)}
    for cases in (ref.FUSED_CASES, ref.VARLEN_CASES):
        assert {(c["profile"], c["max_ctx"]) for c in cases} >= {(p, x) for p in ref.PROFILES for x in (0, 33)}
    assert [c["profile"] for c in ref.CROSS_ROUTE_CASES].count("flat") >= 1 and len(ref.CROSS_ROUTE_CASES) >= 2
    # every head width of the varlen kernel meets, on flat inputs: a query tile that starts above key tile 0; one whose first key tile is
    # wholly masked for its later queries (they still visit it); a window over three key tiles of which the first is partly masked
    for dk in ref.VARLEN_DK:
        above = masked = three = False
        for c in flat:
            if c["dk"] != dk or c["max_ctx"] == 0:
                continue
            for n in c["lengths"]:
                for q0 in range(0, n, 32):
                    lo = kt_lo(q0, c["max_ctx"])
                    last_q = min(q0 + 31, n - 1)
                    above |= lo > 0
                    masked |= lo > 0 and last_q - c["max_ctx"] + 1 >= 32 * (lo + 1)
                    three |= lo > 0 and q0 // 32 - lo >= 2 and (q0 - c["max_ctx"] + 1) % 32 != 0
        assert above and masked and three, dk
    assert len({ref.softmax_case_id(c) for c in ref.SOFTMAX_CASES}) == len(ref.SOFTMAX_CASES)
    for T, ld, m in ref.SOFTMAX_SHAPES:
        mine = [c for c in ref.SOFTMAX_CASES if (c["T"], c["ld"], c["n_mats"]) == (T, ld, m)]
        assert {c["max_ctx"] for c in mine} == {0, 1, 5, T - 1, T, T + 5} and {c["shift"] for c in mine} == {0.0, 200.0, -200.0}
    assert any(c["T"] * c["n_mats"] % 4 for c in ref.SOFTMAX_CASES) and any(c["T"] > 64 for c in ref.SOFTMAX_CASES)


# ------------------------------------------------------------------------------------------ 6. in bounds
@pytest.mark.parametrize("case", ref.FUSED_CASES + ref.VARLEN_CASES, ids=ref.attn_case_id)
def test_attn_case_stays_inside_its_buffers(case):
    a = ref.make_attn_case(case)
    d = a["H"] * a["dk"]
    assert a["buf"].shape == (a["n_tok"] + ref.SLACK_ROWS, a["ld"]) and a["ld"] % 4 == 0 and a["ld"] >= 3 * d and a["ldo"] >= d
    assert all((v.ctypes.data - a["buf"].ctypes.data) % 16 == 0 for v in (a["Q"], a["K"], a["V"]))     # (the device buffer itself is aligned)
    assert np.isfinite(a["buf"][:a["n_tok"], :3 * d]).all() and np.isnan(a["buf"][a["n_tok"]:]).all() and np.isnan(a["buf"][:, 3 * d:]).all()
    off = a["table"][ref.OFF0:]
    assert off[0] != 0 and np.array_equal(np.diff(off[:len(a["lengths"]) + 1]), a["lengths"]) and len(a["table"]) == len(a["lengths"]) + 4
    assert len(a["tiles"]) == sum((n + 31) // 32 for n in a["lengths"]) <= a["n_tok"] // 32 + len(a["lengths"])
    for name, tiles in ref.tile_orders(a["tiles"]):
        assert sorted(map(tuple, tiles.tolist())) == sorted(map(tuple, a["tiles"].tolist())), name
        ext = ref.attn_extent(a, tables=(off, tiles))
        assert ext["ok"] and ext["rows"] == a["n_tok"], name
    if case["route"] != "varlen":                           # the fused kernel: n_blocks * 256 rows, no table
        assert all(n == 256 for n in a["lengths"]) and a["dk"] == 128 and a["n_tok"] == 256 * len(a["lengths"]) <= a["buf"].shape[0]


def test_contract_tables_stay_inside_their_buffers():
    a = ref.make_attn_case(dict(route="varlen", lengths=ref.CONTRACT_LENGTHS, dk=16, H=2, max_ctx=0, ldo_pad=12, profile="flat"))
    assert len(a["tiles"]) + 1 <= a["n_tok"] // 32 + len(a["lengths"])         # the launcher admits one entry more
    for extra in ref.CONTRACT_EXTRA:
        tiles = np.insert(a["tiles"], ref.CONTRACT_AT, extra, axis=0)
        ext = ref.attn_extent(a, tables=(a["table"][ref.OFF0:], tiles))
        assert ext["ok"] and ext["rows"] == a["n_tok"]
        # the kernel's guards, in its order, stop the entry before it is used as an index
        blk, qt = extra
        assert blk < 0 or blk >= len(a["lengths"]) or qt < 0 or 32 * qt >= a["lengths"][blk]
    # the over-claiming table: the rows it claims lie inside the buffers, the rows the guards let through inside the declared n_tok
    off = np.array(ref.OVERCLAIM_OFF)
    assert off[-1] - off[0] > ref.OVERCLAIM_N_TOK and off[-1] - off[0] <= ref.OVERCLAIM_ROWS and off[-2] - off[0] <= ref.OVERCLAIM_N_TOK
    ext = ref.attn_extent(a, n_rows=ref.OVERCLAIM_ROWS, tables=(off, a["tiles"]), n_tok=ref.OVERCLAIM_N_TOK)
    assert ext["ok"] and ext["rows"] == off[-2] - off[0] == 24
    assert len(off) - 1 <= ref.OVERCLAIM_N_TOK and len(a["tiles"]) <= ref.OVERCLAIM_N_TOK // 32 + len(off) - 1


def test_softmax_cases_stay_inside_their_buffers():
    for c in ref.SOFTMAX_CASES:
        S = ref.make_softmax_case(c)
        assert S.shape == (c["n_mats"], c["T"], c["ld"]) and c["ld"] >= c["T"] > 0 and np.isfinite(S).all()
