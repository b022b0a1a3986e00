"""tests/adaptive_ref.py is right before it judges gnnlm_adaptive_target_logp, and the table of tests/test_adaptive_abi_gpu.py reaches
what it claims.  No GPU.

1. The reference equals oracle.adaptive_softmax.target_log_prob (precision 0, float64 on both sides) and the closed form -log N of an
   all-zero row; a target outside the vocabulary is -inf.
2. The constants the table depends on are the sources': the part count 2 * cdiv(N, 128), the 1024-part switch of lse_reduce, the
   n >= 1024 tile-order switch of the head, BS_WAVES and the chunk of band_split_kernel, the bars of test_gemm_abi_gpu.py; the
   dispatch constants behind gemm_ref.route() are pinned by test_gemm_ref_cpu.py, called from here.
3. Every case reaches the routes it names; the table reaches every route and both reduce kernels it claims, the head on
   tile_order 6 with more than four m-tiles, and every pattern of the compaction list does what its name says.
4. A float32 emulation of the call -- numpy float32 GEMMs over a shuffled k order, per-part (max, sum) pairs, the reduce, the
   float32 epilogue -- stays inside bound(case) for every case.
5. Every deliberately wrong reference leaves the bound on at least one row of a named case.
6. The parent commit's row kernels, emulated: row_lse_pick's running (max, sum) gives NaN for a -inf in front of a finite logit and
   for two +inf, the new loop gives what torch.logsumexp gives; band_split's casts alias 2^32 + 3 to a real column and send -1 / V to
   picks the GEMM epilogue never writes."""
import os
import re

import numpy as np
import pytest
import torch

import adaptive_ref as ar
import gemm_ref
from oracle import adaptive_softmax as oasm
from test_gemm_ref_cpu import route_program  # noqa: F401  (fixture: the dispatcher behind a command line)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnn-lm_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def body_of(text, start, end):
    return text[text.index(start):text.index(end, text.index(start))]


# ------------------------------------------------------------------------------------------ 1. what the project already trusts
@pytest.mark.parametrize("name", ["num-p0", "shape-dims-differ", "cmp-n65-b8-uniform", "shape-one-word-band"])
def test_reference_is_the_oracle(name):
    case = ar.case_by_name(name)
    nb = len(case["cutoff"])
    w = {"cutoff": case["cutoff"], "emb": [torch.from_numpy(case["head_w"][:case["cutoff"][0]]).double()]
         + [torch.from_numpy(case["emb"][b]).double() for b in range(1, nb)],
         "proj": [None] + [torch.from_numpy(case["proj_t"][b]).double().t() for b in range(1, nb)],
         "class_proj": torch.from_numpy(case["head_w"][case["cutoff"][0]:]).double()}
    want = oasm.target_log_prob(torch.from_numpy(case["x"]).double(), torch.from_numpy(case["target"]), w).numpy()
    got = ar.adaptive_ref(case)
    assert got["valid"].all()
    # the projection goes through float32 on its way into the band GEMM: 2^-24 sum |xi||e| on a logit
    assert (np.abs(got["logp"] - want) <= 1e-5 + 1e-6 * np.abs(want)).all(), float(np.abs(got["logp"] - want).max())
    assert (got["bound"] > 0).all() and (got["bound"] < 1.0).all()


def test_reference_closed_forms_and_numerics_of_the_table():
    """Row 2 of the numerics cases is all zero: -log(head logits) - log(band size).  Rows 5 and 6 carry a logit of +90.  The target
    is the arg-max on a good part of the rows r % 4 == 1 and 20 nats or more below it on most rows r % 4 == 3."""
    for p in (0, 1, 2, 3):
        case = ar.case_by_name(f"num-p{p}")
        out = ar.case_ref(case)
        cut, nb = case["cutoff"], len(case["cutoff"])
        b = int(out["band"][2])
        assert b == 2 and not case["x"][2].any()
        want = -np.log(cut[0] + nb - 1) - np.log(cut[b] - cut[b - 1])
        assert abs(out["logp"][2] - want) < 1e-12
        assert out["band"][5] > 0 and out["band"][6] == 0
        lp = out["logp"]
        assert (lp[1::4] > -1e-2).mean() > 0.25 and (lp[3::4] < -20).mean() > 0.75, (np.sort(lp[1::4]), np.sort(lp[3::4]))
        assert len({row.tobytes() for row in case["x"]}) == case["n"], "every row has an x of its own"
    one = ar.case_by_name("shape-one-word-band")
    out = ar.case_ref(one)
    m = out["band"] == 1
    head_pick, _ = ar.compact(one)
    ph, lh, _, _ = ar.lse_pick(one["x"][m], one["head_w"], head_pick[m], 0)
    assert m.any() and np.array_equal(out["logp"][m], ph - lh), "the tail term of a one-word band is exactly 0"


def test_outside_the_vocabulary_is_minus_infinity():
    for name in ("oor-p0", "oor-n1100", "oor-n70-b1"):
        case = ar.case_by_name(name)
        V = case["cutoff"][-1]
        out = ar.case_ref(case)
        t = case["target"]
        bad = (t < 0) | (t >= V)
        assert set(np.nonzero(bad)[0]) == set(case["oor_rows"]) and bad.sum() >= 7
        for v in ar.OOR_TARGETS:
            assert ar._oor_value(v, V) in t.tolist(), v
        assert np.array_equal(bad, ~out["valid"]) and np.isneginf(out["logp"][bad]).all() and np.isfinite(out["logp"][~bad]).all()
        assert np.isneginf(out["image"][bad]).all()
    empty = ar.adaptive_ref(dict(ar.case_by_name("cmp-n1-b3-uniform"), n=0, x=np.zeros((0, 16), dtype=np.float32),
                                 target=np.zeros(0, dtype=np.int64)))
    assert empty["image"].size == 0


# ------------------------------------------------------------------------------------------ 2. the sources
def test_constants_are_the_sources(route_program):
    import test_gemm_ref_cpu
    test_gemm_ref_cpu.test_route_constants_are_the_sources(route_program)
    api, rowops, main = src("adaptive_logp.hip"), src("rowops.hip"), src("gemm_f32.hip")
    impl = body_of(api, "int adaptive_impl(", "\n}\n")
    assert "lse_reduce(b.head_part, 2 * (int)cdiv(head_n, 128), n, nullptr, b.head_lse, s)" in impl
    assert "lse_reduce(b.tail_part, 2 * (int)cdiv(size, 128), n, cnt, b.tail_lse, s)" in impl
    assert "const int head_n = w.cutoff[0] + nt;" in impl and "const int size = w.cutoff[i] - w.cutoff[i - 1];" in impl
    assert ar.n_parts(129) == 4 and ar.n_parts(128) == 2 and ar.n_parts(1) == 2
    m = re.search(r"if \(n >= (\d+)\) g\.tile_order = (\d+) \+ (\d+);", impl)
    assert int(m.group(1)) == ar.HEAD_ORDER_MIN_N and int(m.group(2)) + int(m.group(3)) == ar.HEAD_TILE_ORDER
    # the gathered projection and the band GEMM as gemm_descs() restates them
    assert "g.a_rows = rows; g.W = w.proj_t[i]; g.ldw = w.d; g.C = b.xi; g.ldc = w.dim[i];" in impl
    assert "g.M = (int)n; g.N = w.dim[i]; g.K = w.d; g.m_dev = cnt;" in impl
    assert "t.M = (int)n; t.N = size; t.K = w.dim[i]; t.m_dev = cnt;" in impl and "t.A = b.xi; t.lda = w.dim[i];" in impl
    red = body_of(main, "int lse_reduce(", "\n}\n")
    m = re.search(r"if \(n_parts >= (\d+)\)\s*hipLaunchKernelGGL\(lse_reduce_kernel<4>", red)
    assert int(m.group(1)) == ar.REDUCE4_MIN_PARTS and "lse_reduce_kernel<1>" in red
    m = re.search(r"constexpr int BS_WAVES = (\d+);", rowops)
    assert int(m.group(1)) == ar.BS_WAVES
    split = body_of(rowops, "void band_split_kernel(", "\n}\n")
    assert "base += 64 * BS_WAVES" in split and ar.CHUNK == 64 * ar.BS_WAVES == 1024
    gpu = open(os.path.join(ROOT, "tests", "test_gemm_abi_gpu.py")).read()
    assert eval(re.search(r"^BAR = (\{.*\})$", gpu, re.M).group(1)) == ar.BAR
    assert float(re.search(r"^LSE_BAR = (\S+)$", gpu, re.M).group(1)) == ar.LSE_BAR


# ------------------------------------------------------------------------------------------ 3. the table
def _shape_case(spec):
    """a case without its data: enough for routes()"""
    s = dict(precision=0)
    s.update(spec)
    return dict(name=s["name"], n=s["n"], d=s["d"], cutoff=list(s["cut"]), dim=[0] + list(s["dim"]), precision=s["precision"])


def test_every_case_reaches_the_routes_it_names():
    for spec in ar.SPECS:
        rt = ar.routes(_shape_case(spec))
        for k, v in spec.get("expect", {}).items():
            assert rt[k] == v, (spec["name"], k, rt[k], v)
        assert all(d % 4 == 0 and d > 0 for d in spec["dim"]) and spec["d"] % 4 == 0


def test_the_table_reaches_what_it_claims():
    head, band, proj, red_head, red_band, prec_of = set(), set(), set(), set(), set(), {}
    for spec in ar.SPECS:
        c = _shape_case(spec)
        rt = ar.routes(c)
        head.add(rt["head"])
        band.update(rt["band"])
        proj.update(rt["proj"])
        red_band.update(rt["reduce"][1:])
        for k, rts in (("head", [rt["head"]]), ("band", rt["band"])):
            for r in rts:
                prec_of.setdefault((k, r), set()).add(c["precision"])
    assert head == {"reg128", "astat128", "dma128", "dma256", "sched128", "split128", "split256"}
    assert band == {"reg128", "astat128", "dma128", "sched128", "split128"}
    assert proj == {"skinny32", "reg64", "reg128"}
    assert red_band == {1, 4}
    for k in ("head", "band"):
        assert prec_of[(k, "reg128")] == {0, 1, 2, 3} and prec_of[(k, "split128")] == {1, 2, 3}
    assert prec_of[("head", "split256")] == {1, 2, 3}
    # every epilogue route route() can name is reached or listed with its reason
    lse_routes = {"reg128", "astat128", "dma128", "dma256", "sched128", "split128", "split256"}
    assert lse_routes - band == {r for (k, r) in ar.LEFT_OUT if k == "band"}
    # the head on tile_order 6: more than 4 m-tiles of every tile size, more than one band of tiles
    big = _shape_case(ar.SPEC_BY_NAME["head-sched128"])
    assert ar.head_tile_order(big) == 6 and gemm_ref.cdiv(big["n"], 256) > 4
    assert ar.head_tile_order(_shape_case(ar.SPEC_BY_NAME["cmp-n1023-b3-uniform"])) == 0
    assert ar.head_tile_order(_shape_case(ar.SPEC_BY_NAME["cmp-n1024-b3-uniform"])) == 6
    # the four-wave reduce from 65,409 words on, one wave at 65,408
    assert ar.n_parts(65409) == 1024 and ar.n_parts(65408) == 1022
    ns = {s["n"] for s in ar.SPECS if s["name"].startswith("cmp-")}
    assert set(ar.NS) <= ns and {len(s["cut"]) for s in ar.SPECS if s["name"].startswith("cmp-")} == {1, 2, 3, 8}


def test_compaction_patterns_do_what_they_say():
    def counts(name):
        case = ar.case_by_name(name)
        _, lists = ar.compact(case)
        return case, [len(r) for r, _ in lists], lists

    for nb in (3, 8):
        for b in range(nb):
            _, cnt, _ = counts(f"cmp-n2085-b{nb}-all{b}")
            assert cnt == [2085 if i == b else 0 for i in range(1, nb)]
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-row0")
        assert cnt[0] == 1 and lists[0][0][0] == 0 and sum(cnt) == 1
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-rowlast")
        assert cnt[-1] == 1 and lists[-1][0][0] == 2084 and sum(cnt) == 1
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-mod")
        assert all(c >= 2085 // nb for c in cnt)
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-late")
        assert cnt[-1] > 64 and lists[-1][0].min() >= ar.CHUNK and all(len(r) and r.min() < ar.CHUNK for r, _ in lists[:-1])
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-wave")
        assert np.array_equal(lists[0][0], np.arange(ar.CHUNK + 64, ar.CHUNK + 128))
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-chunk")
        assert np.array_equal(lists[0][0], np.arange(ar.CHUNK, 2 * ar.CHUNK))
        case, cnt, lists = counts(f"cmp-n2085-b{nb}-edges")
        cut = case["cutoff"]
        want = {0, cut[-1] - 1} | {c - 1 for c in cut} | set(cut[:-1])
        assert set(case["target"].tolist()) == want
        for c0 in (0, ar.CHUNK, 2 * ar.CHUNK):                     # ... in every chunk
            assert set(case["target"][c0:c0 + ar.CHUNK].tolist()) == want
    case = ar.case_by_name("shape-band-65409")
    assert 0 < len(ar.compact(case)[1][1][0]) < 64


# ------------------------------------------------------------------------------------------ 4. the float32 emulation
def _mm32(A, W, precision, rs):
    perm = rs.permutation(A.shape[1])
    pa, pw = gemm_ref.planes(A, precision), gemm_ref.planes(W, precision)
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j in gemm_ref.PRODUCTS[precision]:
            t = np.ascontiguousarray(pa[i][:, perm]) @ np.ascontiguousarray(pw[j][:, perm]).T
            out = t if out is None else out + t
    assert out.dtype == np.float32
    return out


def _lse_pick32(A, W, pick, precision, rs):
    m, N = A.shape[0], W.shape[0]
    npart = ar.n_parts(N)
    picked, lse = np.full(m, np.nan, dtype=np.float32), np.empty(m, dtype=np.float32)
    for r0 in range(0, m, 256):
        r1 = min(m, r0 + 256)
        x = _mm32(A[r0:r1], W, precision, rs)
        ok = (pick[r0:r1] >= 0) & (pick[r0:r1] < N)
        picked[r0:r1][ok] = x[np.nonzero(ok)[0], pick[r0:r1][ok]]
        xp = np.full((r1 - r0, npart * 64), -np.inf, dtype=np.float32)
        xp[:, :N] = x
        xp = xp.reshape(r1 - r0, npart, 64)
        pm = xp.max(-1)
        with np.errstate(invalid="ignore"):
            ps = np.where(np.isneginf(xp), np.float32(0), np.exp(xp - pm[..., None])).sum(-1, dtype=np.float32)
            mm = pm.max(-1)
            ss = np.where(np.isneginf(pm), np.float32(0), ps * np.exp(pm - mm[:, None])).sum(-1, dtype=np.float32)
        lse[r0:r1] = mm + np.log(ss)
    return picked, lse


def emulate32(case, seed=0):
    rs = np.random.RandomState(seed)
    n, prec, cut = case["n"], case["precision"], case["cutoff"]
    head_pick, lists = ar.compact(case)
    out = np.full(n, -np.inf, dtype=np.float32)
    rows = np.nonzero(head_pick >= 0)[0]
    ph, lh = _lse_pick32(case["x"][rows], case["head_w"], head_pick[rows], prec, rs)
    out[rows] = ph - lh
    for b in range(1, len(cut)):
        br, bp = lists[b - 1]
        if len(br):
            xi = _mm32(case["x"][br], case["proj_t"][b], prec, rs)
            pt, lt = _lse_pick32(xi, case["emb"][b], bp, prec, rs)
            out[br] = out[br] + (pt - lt)
    return out


@pytest.mark.parametrize("name", ar.CASES)
def test_float32_emulation_is_inside_the_bound(name):
    case = ar.case_by_name(name)
    ref = ar.case_ref(case)
    got = emulate32(case)
    bad = ar.outside(got, ref["logp"], ref["bound"], ref["valid"])
    v = ref["valid"] & np.isfinite(ref["logp"])
    worst = float((np.abs(got[v] - ref["logp"][v]) / ref["bound"][v]).max()) if v.any() else 0.0
    print(f"{name}: emulation error / bound {worst:.3f}, bound {ref['bound'][v].min():.2e} .. {ref['bound'][v].max():.2e}")
    assert not len(bad), (name, bad[:5], got[bad[:5]], ref["logp"][bad[:5]], ref["bound"][bad[:5]])
    assert ref["image"].dtype == np.float32 and ref["image"].shape == (case["n"],)


# ------------------------------------------------------------------------------------------ 5. mutations
MUTATION_CASES = {
    "shift_picks": "cmp-n65-b3-uniform",
    "no_carry": "cmp-n2085-b3-late",
    "gt_cutoff": "cmp-n2085-b3-edges",
    "no_class": "num-p0",
    "tail_assigned": "num-p0",
    "one_part_fewer": "cmp-n65-b1-uniform",         # 90 head logits: the second part holds 26 of them
    "no_max": "num-p0",                             # rows 5 and 6: a logit of +90
    "no_reround_p3": "num-p3",
    "clamp_oor": "oor-p0",
}


@pytest.mark.parametrize("mutation", ar.MUTATIONS)
def test_a_wrong_reference_leaves_the_bound(mutation):
    case = ar.case_by_name(MUTATION_CASES[mutation])
    ref = ar.case_ref(case)
    wrong = ar.adaptive_ref(case, mutate=mutation)
    bad = ar.outside(wrong["logp"], ref["logp"], ref["bound"], ref["valid"])
    print(f"{mutation} on {case['name']}: {len(bad)} of {case['n']} rows leave the bound")
    assert len(bad) >= 1
    if mutation == "no_max":
        assert {5, 6} <= set(bad.tolist())
    if mutation == "clamp_oor":
        assert set(bad.tolist()) == set(case["oor_rows"])
    if mutation == "no_carry":
        assert (bad >= ar.CHUNK).any() or (bad < ar.CHUNK).any()
    if mutation == "no_reround_p3":                 # ... and at the other precisions there is no second rounding to leave out
        assert len(bad) >= case["n"] // 8


def test_mutation_list_is_the_issue_list():
    assert set(MUTATION_CASES) == set(ar.MUTATIONS) and len(ar.MUTATIONS) == 9


# ------------------------------------------------------------------------------------------ 6. the parent commit's row kernels
def _row_lse_thread(vals, old):
    """the running (max, sum) of one thread of row_lse_pick_kernel, float32: the parent commit's loop and this one's"""
    f = np.float32
    m, s, pinf = f(-np.inf), f(0), False
    with np.errstate(invalid="ignore", over="ignore"):
        for v in np.asarray(vals, dtype=np.float32):
            if old:
                if v > m:
                    s = f(s * np.exp(f(m - v)) + f(1))
                    m = v
                else:
                    s = f(s + np.exp(f(v - m)))
            elif v == f(np.inf):
                pinf = True
            elif v > m:
                s = f(s * np.exp(f(m - v)) + f(1))
                m = v
            elif v != f(-np.inf):
                s = f(s + np.exp(f(v - m)))
        if old:
            return f(m + np.log(s))
        return s if s != s else f(np.inf) if pinf else f(-np.inf) if s == 0 else f(m + np.log(s))


@pytest.mark.parametrize("vals", [[-np.inf, 1.0], [-np.inf, -np.inf, 2.0, 0.5], [np.inf, np.inf], [np.inf, 1.0, np.inf], [-np.inf, -np.inf],
                                  [1.0, -np.inf, 3.0], [np.nan, 1.0], [-np.inf, np.nan]])
def test_row_lse_loop_red_on_the_parent_commit(vals):
    want = torch.logsumexp(torch.tensor(vals, dtype=torch.float64), 0).item()
    new = float(_row_lse_thread(vals, old=False))
    assert (np.isnan(want) and np.isnan(new)) or new == want or abs(new - want) < 1e-6, (vals, new, want)
    if vals[0] == -np.inf and np.isfinite(vals).any() or vals.count(np.inf) >= 2:
        assert np.isnan(float(_row_lse_thread(vals, old=True))), "the parent commit's loop"


def test_band_split_red_on_the_parent_commit():
    """The parent commit's band_split_kernel, restated: band by t >= cutoff alone, (int32_t) casts.  2^32 + 3 becomes column 3 of the
    head and INT64_MIN column 0 (a finite log-probability where -inf is due); -1 stays a negative pick and V, V + 1, 2^31, INT64_MAX land in the last
    band with a pick at or beyond its size (or a negative one): the epilogue leaves lse_picked alone -- whatever the workspace held."""
    case = ar.case_by_name("oor-p0")
    cut = np.asarray(case["cutoff"], dtype=np.int64)
    t = case["target"]
    band = np.searchsorted(cut[:-1], t, side="right")
    i32 = lambda v: ((v + 2 ** 31) % 2 ** 32 - 2 ** 31)
    head_pick = np.where(band == 0, i32(t), cut[0] + band - 1)
    size_last = cut[-1] - cut[-2]
    for r in case["oor_rows"]:
        v = int(t[r])
        if v == 2 ** 32 + 3:
            assert band[r] == len(cut) - 1 and not 0 <= i32(v - int(cut[-2])) < size_last
        elif v == ar.INT64_MIN:
            assert band[r] == 0 and head_pick[r] == 0, "the low 32 bits are 0: the parent commit scores row r against word 0"
        elif v < 0:
            assert band[r] == 0 and head_pick[r] < 0, "lse_picked[r] stays what the workspace held"
        else:
            assert band[r] == len(cut) - 1 and not 0 <= i32(v - int(cut[-2])) < size_last
    # with one band the casts alias: 2^32 + 3 is column 3
    one = ar.case_by_name("oor-n70-b1")
    r = [r for r in one["oor_rows"] if int(one["target"][r]) == 2 ** 32 + 3][0]
    assert i32(int(one["target"][r])) == 3 < one["cutoff"][0], "the parent commit scores row r against word 3"
    head_pick_new, _ = ar.compact(one)
    assert head_pick_new[r] == -1 and np.isneginf(ar.case_ref(one)["logp"][r])
