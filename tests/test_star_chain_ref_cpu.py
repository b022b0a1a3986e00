"""tests/star_chain_ref.py is right before it judges a kernel, and the inputs of tests/test_star_chain_abi_gpu.py can tell a kernel
that ignores a descriptor field from one that honours it.  No GPU.

1. star_ref / chain_ref with the plainest descriptor equal the formulas of test_star_attn_pq / test_star_attn_dense and the
   explicit-edge loop of test_chain_attn (oracle.graph.build_ntgt_edges), on those tests' inputs.
2. For every case of the GPU tables and every field the case sets: the reference with that one field neutralised differs from the true
   one by more than 100 x the GPU bar somewhere in Z / out, or in has_nb / the write mask.
3. Per star case: 30 % .. 90 % of the neighbours valid, a token without any, and for every validity rule in force a neighbour that this
   rule alone excludes.  (A case of one token cannot have a token without neighbours next to one with: T = 1 is exempt from that
   one condition, the T = 6 case of the same route and option carries it.)
4. star_chain_ref.star_route is the dispatcher: it is compared with star_route() of csrc/star_route.h itself
   (tests/star_route_main.cpp, built with the host compiler)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import star_chain_ref as ref
from oracle import graph as og
from oracle import pq as opq

FAR = 100 * ref.TOL


def differs(a, b):
    """somewhere further apart than FAR (a NaN on one side only is as far as it gets)"""
    with np.errstate(invalid="ignore"):
        return bool((~(np.abs(a - b) <= FAR) & ~(np.isnan(a) & np.isnan(b))).any())


# ------------------------------------------------------------------------------------------ 1. the plainest option
@pytest.mark.parametrize("T,H,M,dsub,kg", [(5, 2, 4, 4, 4), (9, 8, 128, 8, 128), (3, 8, 128, 4, 33), (4, 3, 16, 8, 70), (2, 12, 32, 8, 16)])
def test_star_ref_is_the_pq_formula(T, H, M, dsub, kg):
    rs = np.random.RandomState(T * 31 + H)                  # the inputs of test_star_attn_pq
    N, D = 3000, M * dsub
    codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
    cen = (rs.randn(M, 256, dsub) * 0.5).astype(np.float32)
    U = (rs.randn(T, H, D) / np.sqrt(D)).astype(np.float32)
    ids = rs.randint(0, N, size=(T, kg)).astype(np.int64)
    ids[0, 1] = -1
    ids[1, :] = -1
    X = opq.pq_lookup(codes[np.where(ids < 0, 0, ids).reshape(-1)], cen).reshape(T, kg, D).astype(np.float64)
    s = np.einsum("tjd,thd->thj", X, U.astype(np.float64))
    s = np.where((ids >= 0)[:, None, :], s, -np.inf)
    with np.errstate(invalid="ignore"):
        a = np.exp(s - s.max(-1, keepdims=True))
        a = np.nan_to_num(a / a.sum(-1, keepdims=True))
    want = np.einsum("thj,tjd->thd", a, X)
    Z, has = ref.star_ref(U, ids, codes=codes, centroids=cen, M=M, dsub=dsub, row0=0, n_local=N, n_store=N)
    assert np.abs(Z - want).max() < 1e-12
    assert np.array_equal(has, (ids >= 0).any(1).astype(np.float32))


@pytest.mark.parametrize("T,H,D,kg,n_g", [(6, 8, 64, 10, 3), (4, 8, 1024, 37, 1), (3, 5, 512, 128, 5), (3, 8, 256, 9, 2), (2, 12, 1024, 16, 1)])
def test_star_ref_is_the_dense_formula(T, H, D, kg, n_g):
    rs = np.random.RandomState(2 + D + kg)                  # the inputs of test_star_attn_dense
    X = rs.randn(T * kg * n_g, D).astype(np.float32)
    U = (rs.randn(T, H, D) / np.sqrt(D) * 3).astype(np.float32)
    ids = rs.randint(0, 100, size=(T, kg)).astype(np.int64)
    ids[2 % T, 3] = -1
    ids[0, rs.rand(kg) < 0.3] = -1
    ids[1] = -1
    Xc = X.reshape(T, kg, n_g, D)[:, :, 0].astype(np.float64)
    s = np.where((ids >= 0)[:, None, :], np.einsum("tjd,thd->thj", Xc, U.astype(np.float64)), -np.inf)
    with np.errstate(invalid="ignore"):
        a = np.exp(s - s.max(-1, keepdims=True))
        a = np.nan_to_num(a / a.sum(-1, keepdims=True))
    Z, has = ref.star_ref(U, ids, X=X.reshape(-1), ldx=D, x_group_stride=n_g)
    assert np.abs(Z - np.einsum("thj,tjd->thd", a, Xc)).max() < 1e-12
    assert np.array_equal(has, (ids >= 0).any(1).astype(np.float32))


def edge_loop(Q, K, V, rows, valid, scale, H, dk):
    """the reference loop of test_chain_attn: explicit edges from the oracle's restatement of build_ntgt_edges"""
    G, n_g = rows.shape
    out = np.zeros((G * n_g, H * dk))
    for g in range(G):
        o2i = {int(rows[g, c]): g * n_g + c for c in range(n_g) if valid[g, c]}
        src, dst = og.build_ntgt_edges(o2i, context=1, bidirect=True)
        for node in set(dst):
            us = [s for s, t in zip(src, dst) if t == node]
            for h in range(H):
                sl = slice(h * dk, (h + 1) * dk)
                sc = np.array([Q[node, sl].astype(np.float64) @ K[u, sl] for u in us]) * scale[h]
                a = np.exp(sc - sc.max())
                a /= a.sum()
                out[node, sl] = sum(ai * V[u, sl].astype(np.float64) for ai, u in zip(a, us))
    return out


@pytest.mark.parametrize("left,right,H,dk", [(2, 2, 8, 128), (0, 0, 2, 16), (1, 1, 8, 4), (3, 1, 4, 32), (0, 2, 2, 8)])
def test_chain_ref_is_the_edge_loop(left, right, H, dk):
    rs = np.random.RandomState(left * 5 + right)            # the inputs of test_chain_attn
    n_store, G, d = 40, 23, H * dk
    n_g = 1 + left + right
    ids = rs.randint(0, n_store, size=G).astype(np.int64)
    ids[:5] = [0, 1, n_store - 1, n_store - 2, -1]
    rows, valid = og.slot_layout(ids.reshape(-1, 1), n_store, left, right)
    rows, valid = rows.reshape(G, n_g), valid.reshape(G, n_g)
    Q, K, V = (rs.randn(G * n_g, d).astype(np.float32) for _ in range(3))
    scale = (1 + 0.3 * rs.randn(H)).astype(np.float32)
    out, mask = ref.chain_ref(Q, K, V, valid.reshape(-1), n_groups=G, left=left, right=right, H=H, dk=dk, scale=scale)
    assert np.abs(out - edge_loop(Q, K, V, rows, valid, scale, H, dk)).max() < 1e-12
    assert mask.all() and not out[~valid.reshape(-1)].any()


@pytest.mark.parametrize("left,right", ref.CHAIN_SHAPES + [(1, 1)])
def test_chain_ref_with_holes_is_the_edge_loop(left, right):
    """the validity patterns of the GPU cases (holes in the middle of a group, whole groups, group 0 and the last group partly invalid):
    slot c of a group stands for the row o + delta[c], so a hole leaves a gap of 2 between its neighbours and breaks the path."""
    c = ref.make_chain_case(dict(left=left, right=right, dk=4, H=2, scale=True))
    G, n_g = c["G"] + ref.SLACK_GROUPS, c["n_g"]
    valid = c["valid"].reshape(G, n_g) != 0
    if n_g > 2:
        assert any(not valid[g, ref.chain_slot(p, left)] and valid[g, ref.chain_slot(p - 1, left)] and valid[g, ref.chain_slot(p + 1, left)]
                   for g in range(G) for p in range(1, n_g - 1))
    delta = np.concatenate([[0], np.arange(-left, 0), np.arange(1, right + 1)])
    rows = 100 * np.arange(1, G + 1)[:, None] + delta[None, :]
    out, mask = ref.chain_ref(c["Q"], c["K"], c["V"], c["valid"], **dict(c["kw"], n_groups=G))
    want = edge_loop(c["Q"], c["K"], c["V"], rows, valid, c["kw"]["scale"], 2, 4)
    assert np.abs(out - want).max() < 1e-12 and mask.all()


def test_chain_ref_kv_index_radius_and_count():
    """the three later fields against the plain reference: row-keyed K / V are the gathered K / V; a radius and a group count only
    shrink the write mask, the rows inside it do not change."""
    c = ref.make_chain_case(dict(left=4, right=3, dk=4, H=2, scale=True, kv=True))
    kw, idx = c["kw"], c["kw"]["kv_index"]
    out, mask = ref.chain_ref(c["Q"], c["K"], c["V"], c["valid"], **kw)
    plain = dict(kw, kv_index=None)
    Kg, Vg = c["K"][np.maximum(idx, 1)], c["V"][np.maximum(idx, 1)]
    out0, _ = ref.chain_ref(c["Q"], Kg, Vg, c["valid"], **plain)
    assert np.array_equal(out, out0) and mask[:c["G"] * c["n_g"]].all() and not mask[c["G"] * c["n_g"]:].any()
    for rad, ngd in [(1, None), (2, None), (3, 4), (0, 0), (0, 100)]:
        o, m = ref.chain_ref(c["Q"], Kg, Vg, c["valid"], **dict(plain, radius_p1=rad, n_groups_dev=ngd))
        slot = np.arange(c["n_slots"])
        dist = np.array([0, 4, 3, 2, 1, 1, 2, 3])[slot % 8]
        want = (slot // 8 < (c["G"] if ngd is None else min(c["G"], ngd))) & ((rad == 0) | (dist <= rad - 1))
        assert np.array_equal(m, want) and np.abs(o[m] - out0[m]).max(initial=0) < 1e-12 and not o[~m].any()


# ------------------------------------------------------------------------------------------ 2 + 3. the inputs of the GPU cases
def test_star_tables_cover_every_route_and_option():
    for shapes, options in ((ref.STAR_PQ_SHAPES, ref.PQ_OPTIONS), (ref.STAR_DENSE_SHAPES, ref.DENSE_OPTIONS)):
        for route, shape in shapes:
            assert ref.star_route(**shape) == route, (route, shape)
            assert all((route, shape, o) in ref.STAR_CASES for o in options)
    assert {r for r, _ in ref.STAR_PQ_SHAPES} == {"tab<8,128>", "tab<8,0>", "tab<4,0>", "generic<1>,staged", "generic<2>,staged",
                                                  "generic<4>,staged", "generic<4>,unstaged"}
    assert {r for r, _ in ref.STAR_DENSE_SHAPES} == {"dense<1>", "dense<2>", "dense<4>", "generic<1>,dense", "generic<4>,dense"}
    assert len({ref.star_case_id(c) for c in ref.STAR_CASES}) == len(ref.STAR_CASES)


# ------------------------------------------------------------------------------------------ 4. the dispatcher itself
ROUTE_NAMES = {"tab<8,128>", "tab<8,0>", "tab<4,0>", "dense<1>", "dense<2>", "dense<4>"} | \
              {f"generic<{n}>,{how}" for n in (1, 2, 4) for how in ("staged", "unstaged", "dense")}
PQ_GRID = [dict(T=4, H=8, M=M, dsub=dsub, kg=kg) for M in [8] + list(range(16, 257, 16)) for dsub in (4, 8, 16) if M * dsub <= 1024
           for kg in (1, 128, 129, 330, 1024)]
DENSE_GRID = [dict(T=4, H=H, D=D, kg=kg) for D in (64, 256, 512, 768, 1024) for H in (1, 8, 9, 12) for kg in (1, 128, 1024, 4000)]
# the literals of ref.star_route, by the names csrc/star_route.h gives them
STAR_CONSTANTS = dict(HB=8, KGM=128, CD=32, TPW=4, TABF=32 * 256, SCS=132, STAR_THREADS=256, STAR_TAB_THREADS=768,
                      STAR_LDS_MAX=160 * 1024, STAR_LDS_TWO_WG=64 * 1024)


@pytest.fixture(scope="module")
def star_route_program(tmp_path_factory):
    """tests/star_route_main.cpp: csrc/star_route.h behind a command line, built with the host compiler alone"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("star_route") / "star_route_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(os.path.dirname(os.path.abspath(__file__)), "star_route_main.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(exe, *args, stdin="", env=None):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GNNLM_STAR_")}
    e.update(env or {})
    r = subprocess.run([exe, *args], input=stdin, capture_output=True, text=True, env=e)
    assert r.returncode == 0, r.stderr
    return r.stdout.split("\n")[:-1]


def real_routes(exe, shapes, env=None):
    """[(route of star_route() spelt as ref.star_route spells it, dynamic LDS bytes, threads)] for the shapes"""
    lines = [" ".join(str(s.get(k, 0)) for k in ("T", "H", "kg", "M", "dsub")) + f" {s['M'] * s['dsub'] if 'M' in s else s['D']}" for s in shapes]
    out = [l.split() for l in ask(exe, "route", stdin="\n".join(lines) + "\n", env=env)]
    assert len(out) == len(shapes)
    res = []
    for s, (name, staged, lds, threads, heads) in zip(shapes, out):
        assert int(heads) == 8 and (name.startswith("generic") or staged == "0")
        if name.startswith("generic"):
            name += ",dense" if "M" not in s else ",staged" if staged == "1" else ",unstaged"
        res.append((name, int(lds), int(threads)))
    return res


def lds_bytes(route, T, H, kg, M=0, dsub=0, D=0):
    """the dynamic LDS of the route's launch, by the formulas of ref.star_route"""
    D = M * dsub if M else D
    if route.startswith("tab"):
        return 2 * 32 * 256 * 4 + 4 * 8 * 132 * 4 + 2 * 4 * 1024 + 4 * 128 + 4 * 128 * M
    if route.startswith("dense"):
        return (8 * D + 4 * 8 * 2) * 4 + kg * 8
    return (8 * kg + 8 * D + ((kg + 3) & ~3)) * 4 + (((kg * M + 15) & ~15) if route.endswith(",staged") else 0)


def test_star_route_is_the_dispatcher(star_route_program):
    """ref.star_route against star_route() of csrc/star_route.h itself: on every shape of the case tables and over a grid that
    reaches every route; the LDS bytes and the workgroup size of the plan; the A/B switch; the header's constants by value."""
    got = dict(l.split() for l in ask(star_route_program, "constants"))
    assert {k: int(v) for k, v in got.items()} == STAR_CONSTANTS
    listed = ref.STAR_PQ_SHAPES + ref.STAR_DENSE_SHAPES
    for (want, shape), (rt, _, _) in zip(listed, real_routes(star_route_program, [s for _, s in listed])):
        assert rt == want, (shape, rt)                                 # (the labels, asked of the code too)
    # one step to either side of the two LDS bounds that choose a kernel, written by hand: the dense kernel's 64 KiB
    # ((8 * 1024 + 64) * 4 + 8 kg: k_g = 4064) and the staging of the generic one (41792 + 23680 = 65472, 41840 + 23728 = 65568)
    edges = [(dict(T=4, H=8, D=1024, kg=4064), "dense<4>"), (dict(T=4, H=8, D=1024, kg=4065), "generic<4>,dense"),
             (dict(T=4, H=8, M=40, dsub=16, kg=592), "generic<4>,staged"), (dict(T=4, H=8, M=40, dsub=16, kg=593), "generic<4>,unstaged")]
    for (s, want), (rt, _, _) in zip(edges, real_routes(star_route_program, [s for s, _ in edges])):
        assert rt == want, (s, rt)
    shapes = [s for _, s in listed] + [s for s, _ in edges] + PQ_GRID + DENSE_GRID
    real = real_routes(star_route_program, shapes)
    for s, (rt, lds, threads) in zip(shapes, real):
        assert rt == ref.star_route(**s), (s, rt)
        assert lds == lds_bytes(rt, **s), (s, rt, lds)
        assert threads == (768 if rt.startswith("tab") else 256), (s, rt)
    assert {rt for rt, _, _ in real[len(listed) + len(edges):]} == ROUTE_NAMES                 # the grid alone reaches every route
    # GNNLM_STAR_GENERIC: neither tab nor dense, and the generic kernel as it would be chosen without them
    off = real_routes(star_route_program, shapes, env={"GNNLM_STAR_GENERIC": "1"})
    for s, (rt, lds, threads), (rt0, _, _) in zip(shapes, off, real):
        assert rt.startswith("generic") and threads == 256 and lds == lds_bytes(rt, **s), (s, rt)
        assert rt == rt0 or not rt0.startswith("generic"), (s, rt, rt0)
    # T = 0: nothing to launch
    assert real_routes(star_route_program, [dict(T=0, H=8, M=128, dsub=8, kg=128), dict(T=0, H=8, D=256, kg=9)]) == [("none", 0, 0)] * 2


@pytest.mark.parametrize("case", ref.STAR_CASES, ids=ref.star_case_id)
def test_star_case_inputs(case):
    c = ref.make_star_case(*case)
    kw, T = c["kw"], c["T"]
    Z, has = ref.star_ref(c["U"], c["ids"], **kw)
    rules = ref.star_rules(c["ids"], **kw)
    ok = np.logical_and.reduce(list(rules.values()))
    # the construction and the rules agree; nothing valid touches poison
    assert np.array_equal(ok, c["reason"] == "") and np.abs(Z).max() < 50
    # validity variety
    assert 0.3 <= ok.mean() <= 0.9, ok.mean()
    assert T == 1 or (has == 0).any()
    assert (has == 1).any()
    for name, r in rules.items():
        others = np.logical_and.reduce([v for k, v in rules.items() if k != name] + [np.ones_like(r)])
        assert (~r & others).any(), f"no neighbour is excluded by {name} alone"
    if "window" in rules:                                   # both sides of the window, and the ids on the edges of every bound
        ids = c["ids"]
        assert (ids[ids >= 0] < ref.ROW0).any() and (ids >= ref.ROW0 + ref.N_LOCAL).any()
        assert {ref.ROW0 - 1, ref.ROW0 + ref.N_LOCAL} <= set(ids.reshape(-1).tolist())
        if kw.get("x_index") is None:
            assert ref.ROW0 in ids[ok] and (min(ref.N_STORE, ref.ROW0 + ref.N_LOCAL) if kw["n_store"] else ref.ROW0 + ref.N_LOCAL) - 1 in ids[ok]
    if kw["n_store"]:
        assert ref.N_STORE in c["ids"]
    if kw.get("x_index") is not None:                       # many neighbours share a group
        g = kw["x_index"][kw["x_index"] >= 0]
        assert len(np.unique(g)) < len(g) / 2
    if kw.get("codes_index") is not None:                   # permuted, many to one, no entry out of range
        t = kw["codes_index"]
        own = t[np.arange(T * c["kg"])[ok.reshape(-1)] * kw["codes_direct"]]
        assert t.min() >= 0 and t.max() < len(kw["codes"]) and len(np.unique(own)) < len(own)
        assert (own != np.arange(T * c["kg"])[ok.reshape(-1)] * kw["codes_direct"]).any()
    # sensitivity: one field neutralised at a time
    neutral = ref.star_neutralised(c)
    O = dict((ref.PQ_OPTIONS if "codes" in kw else ref.DENSE_OPTIONS)[c["opt"]])
    assert len(neutral) == sum([O.get("cd", 0) > 1, O.get("cidx", False), 2 * (O.get("nbv", 0) > 0) - (O.get("nbv", 0) == 1),
                                O.get("xidx", False), O.get("xgs", 1) > 1, "X" in kw, O.get("window", False), O.get("n_store", False)])
    for what, kw2 in neutral:
        Z2, has2 = ref.star_ref(c["U"], c["ids"], **kw2)
        assert differs(Z, Z2) or not np.array_equal(has, has2), what


@pytest.mark.parametrize("case", ref.CHAIN_CASES, ids=ref.chain_case_id)
def test_chain_case_inputs(case):
    c = ref.make_chain_case(case)
    kw, G, n_g = c["kw"], c["G"], c["n_g"]
    out, mask = ref.chain_ref(c["Q"], c["K"], c["V"], c["valid"], **kw)
    assert np.isfinite(out).all()                           # no NaN row is read by the rule
    cnt = min(G, kw.get("n_groups_dev", G))
    assert not mask[cnt * n_g:].any() and not out[~mask].any()
    v = c["valid"].reshape(-1, n_g)[:G] != 0
    assert not v[2].any() and v[3].all() and (c["valid"].reshape(-1, n_g)[G:] != 0).all()
    if n_g > 1:
        assert 0 < v[0].sum() < n_g and 0 < v[G - 1].sum() < n_g
    if "kv_index" in kw:
        idx = kw["kv_index"]
        assert len(c["K"]) != len(c["Q"]) and ((idx == -1) == (c["valid"] == 0)).all() and idx.max() < len(c["K"])
        live = idx[(idx > 0) & (idx < len(c["K"]) - 1)]
        assert len(np.unique(live)) < len(live) and not (idx == 0).any()
    neutral = ref.chain_neutralised(c)
    assert len(neutral) >= (2 if kw["radius_p1"] else 0) + ("kv_index" in kw) + ("n_groups_dev" in kw)
    for what, kw2, K2, V2 in neutral:
        out2, mask2 = ref.chain_ref(c["Q"], K2, V2, c["valid"], **kw2)
        assert not np.array_equal(mask, mask2) or differs(out, out2), what
