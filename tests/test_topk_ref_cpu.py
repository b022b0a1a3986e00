"""tests/topk_ref.py is right before it judges a kernel, and the tables of tests/test_topk_abi_gpu.py can tell a kernel that ignores a
descriptor field from one that honours it.  No GPU.

1. Without ties and invalid entries, fold() from an empty state equals the project's oracle (oracle.knn.brute_force_search) through the
   col_scale / col_bias / alpha recipe of knn_model.py: both metrics, with and without cosine; ids exactly, values within the float32
   rounding of the two formulas.
2. With ties, fold() equals np.argsort(kind="stable") over the columns sorted by id.
3. Folding any split of CHUNK_CASES chunk by chunk equals folding the row at once.
4. For every case and every field it sets, the reference with that one field neutralised or shifted differs in the expected bits.
5. route() agrees with the dispatch constants of csrc/topk.hip, parsed from the source; every route it can name is covered, with every
   boundary, id mode, direction, state and chunk width the tables promise.
6. The rows are what their names say: the id-digit rows tie across the cut with ids that differ in one 11-bit digit only."""
import collections
import functools
import re

import numpy as np
import pytest

import topk_ref as ref
from oracle import knn as oknn


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def select_case(i):
    return ref.make_case(ref.SELECT_CASES[i])


@functools.lru_cache(maxsize=None)
def merge_case(i):
    return ref.make_merge_case(ref.MERGE_CASES[i])


# ------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_fold_is_the_oracle(metric, cosine):
    rs = np.random.RandomState(5)
    n, N, d, k = 4, 200, 8, 17
    q, keys = rs.randn(n, d).astype(np.float32), rs.randn(N, d).astype(np.float32)
    want_v, want_i = oknn.brute_force_search(q, keys, k, metric=metric, cosine=cosine)
    full_v, _ = oknn.brute_force_search(q, keys, N, metric=metric, cosine=cosine)
    n2 = (keys ** 2).sum(-1)
    scale = (1.0 / np.sqrt(n2)).astype(np.float32) if cosine else None          # knn_model.py: col_scale = |key|^-1 (cosine),
    bias = None                                                                 # col_bias = |key|^2 (l2; of the normalised key with cosine)
    if metric == "l2":
        bias = (n2 * scale ** 2).astype(np.float32) if cosine else n2
    call = dict(scores=(q @ keys.T).astype(np.float32), ncols=N, k=k, largest=int(metric == "ip"), init=1,
                alpha=1.0 if metric == "ip" else -2.0, col_scale=scale, col_bias=bias, col0=0, col_ids=None, ids=None, row_ncols=None)
    got_v, got_i = ref.fold(call)
    if metric == "l2":
        got_v = got_v + (q ** 2).sum(-1, keepdims=True)
    # float32 rounding of the two formulas: each is a sum of d products of magnitude at most (|q| + |key|)^2 (cosine: |key| = 1)
    kn = 1.0 if cosine else np.sqrt(n2).max()
    bar = (d + 8) * 2.0 ** -24 * (np.sqrt((q ** 2).sum(-1, keepdims=True)) + kn) ** 2
    assert (np.abs(np.diff(full_v[:, :k + 1].astype(np.float64), axis=1)) > 2 * bar).all()   # a condition of the test: no two of the best k + 1 within the rounding
    assert np.array_equal(got_i, want_i)
    assert (np.abs(got_v.astype(np.float64) - want_v) <= bar).all()


# ------------------------------------------------------------------------------------------ 2. ties: the stable sort
@pytest.mark.parametrize("largest", [1, 0])
def test_fold_is_the_stable_sort(largest):
    rs = np.random.RandomState(11 + largest)
    n, N, k = 6, 500, 64
    scores = rs.randint(-4, 5, (n, N)).astype(np.float32)
    scores[0, :40] = [0.0, -0.0] * 20                                           # the two zeros tie
    ids = np.stack([rs.permutation(N) for _ in range(n)]).astype(np.int64) << 24
    call = dict(scores=scores, ncols=N, k=k, largest=largest, init=1, alpha=1.0, col_scale=None, col_bias=None, col0=0, col_ids=None,
                ids=ids, row_ncols=None)
    got_v, got_i = ref.fold(call)
    for r in range(n):
        by_id = np.argsort(ids[r], kind="stable")
        v, i = scores[r][by_id], ids[r][by_id]
        order = np.argsort(-v if largest else v, kind="stable")[:k]
        assert np.array_equal(got_i[r], i[order]) and np.array_equal(got_v[r], v[order])
        assert len(np.unique(v[order])) < 4                                     # heavy ties inside the result and at the cut


def test_fold_pads_and_skips():
    call = dict(scores=np.array([[np.nan, -np.inf, np.inf, 1.0, 2.0, 3.0]], dtype=np.float32), ncols=6, k=4, largest=1, init=1, alpha=0.0,
                col_scale=None, col_bias=None, col0=-4, col_ids=None, ids=None, row_ncols=np.array([5], dtype=np.int32))
    v, i = ref.fold(call)                                                       # ids -4 .. 1: only columns 4 (id 0) counts; 5 is beyond the row
    assert i.tolist() == [[0, -1, -1, -1]] and v.tolist() == [[2.0, -np.inf, -np.inf, -np.inf]]
    v, i = ref.fold(dict(call, largest=0, col0=0, row_ncols=None))
    assert i.tolist() == [[1, 3, 4, 5]] and v.tolist() == [[-np.inf, 1.0, 2.0, 3.0]]
    v, i = ref.fold(dict(call, col0=10, init=0, k=2), (np.array([[5.0, 2.0]], dtype=np.float32), np.array([[99, 3]])))
    assert i.tolist() == [[12, 99]] and v.tolist() == [[np.inf, 5.0]]
    v, i = ref.fold(dict(call, col0=10, init=0, k=2, largest=0), (np.array([[2.0, np.inf]], dtype=np.float32), np.array([[20, -1]])))
    assert i.tolist() == [[11, 13]] and v.tolist() == [[-np.inf, 1.0]]          # an unfilled slot of the state is no entry


# ------------------------------------------------------------------------------------------ 3. chunking
@pytest.mark.parametrize("spec", ref.CHUNK_CASES, ids=ref.chunk_case_id)
def test_fold_is_independent_of_the_chunking(spec):
    call = ref.make_case(spec)
    whole = ref.fold(call)
    assert set(spec["cuts"]) == {"one", "1+rest", "ragged", "wide+rest"}
    for name, cuts in spec["cuts"].items():
        assert sorted(c for a, b in cuts for c in range(a, b)) == list(range(spec["ncols"])), name
        assert same(ref.fold_chunks(call, cuts), whole), name
        assert same(ref.fold_chunks(call, cuts[::-1]), whole), name             # in any order
    assert (whole[1][[call["patterns"].index("random_ties")]] >= 0).all()
    assert ref.route(call) == f"select<{ref._first(ref.SELECT_KP, spec['k'])},20>"
    first = ref.split(call, *spec["cuts"]["wide+rest"][0], init=1)
    wide = dict(first, ncols=spec["wide"], row_ncols=np.full(len(call["patterns"]), first["ncols"], dtype=np.int32))
    assert ref.route(wide) == f"merge<{ref.merge_kp(spec['k'])}>+prepass"


# ------------------------------------------------------------------------------------------ 4. every field is noticed
def check_fields(call, state):
    base = ref.fold(call, state)
    fields = ref.fields_of(call)
    for f in ref.FIELDS:                                                        # what the case sets is what it claims
        if f in ("largest", "k"):
            continue
        is_set = {"alpha": call["alpha"] not in (0.0, 1.0), "col0": call["ids"] is None and call["col_ids"] is None}.get(f, call.get(f) is not None)
        if f == "col_ids" and call["ids"] is not None:
            is_set = False                                                      # (poisoned: must be ignored)
        assert (f in fields) == (is_set and call["ncols"] > 0), f
    for f in fields:
        other = ref.neutralise(call, f)
        st = state
        if f == "k" and state is not None:
            k2 = other["k"]
            st = tuple(np.concatenate([s, e], axis=1)[:, :k2] for s, e in zip(state, ref.empty_state(len(state[0]), 1, call["largest"])))
        if f == "largest" and state is not None:
            st = (np.where(state[1] >= 0, state[0], -state[0]), state[1])       # the padding of the other direction
        assert not same(ref.fold(other, st), base), f
    if call["ids"] is not None:                                                 # the poisoned sources are ignored
        assert same(ref.fold(dict(call, col_ids=None, col0=0), state), base)
    elif call["col_ids"] is not None:
        assert same(ref.fold(dict(call, col0=0), state), base)


@pytest.mark.parametrize("i", range(len(ref.SELECT_CASES)), ids=[ref.select_case_id(s) for s in ref.SELECT_CASES])
def test_select_cases_notice_their_fields(i):
    check_fields(select_case(i), None)


@pytest.mark.parametrize("i", range(len(ref.MERGE_CASES)), ids=[ref.merge_case_id(s) for s in ref.MERGE_CASES])
def test_merge_cases_notice_their_fields(i):
    call, state = merge_case(i)
    if call["ncols"] > 0:
        check_fields(call, state)
    else:                                                                       # an empty chunk leaves the state's content as it is
        assert same(ref.fold(call, state), state if state is not None else ref.empty_state(len(call["patterns"]), call["k"], call["largest"]))


# ------------------------------------------------------------------------------------------ 5. routes
def test_route_constants_are_the_source():
    src = open(ref.TOPK_SOURCE).read()
    assert int(re.search(r"#define GNNLM_TOPK_PRESEL (\d+)", src).group(1)) == ref.PRESEL
    assert re.search(r"presel = p\.init && ncols >= GNNLM_TOPK_PRESEL \* KP;", src)
    assert int(re.search(r"if \(d\.init && !merge_only && d\.ncols <= (\d+)\)", src).group(1)) == ref.SELECT_MAX_NCOLS
    m = re.search(r"if \(d\.ncols <= (\d+)\) hipLaunchKernelGGL\(\(topk_select_kernel<KP, (\d+)>\).*?\n\s*else hipLaunchKernelGGL\(\(topk_select_kernel<KP, (\d+)>\)", src)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (ref.SELECT_REG_NCOLS, 16, 20)
    assert ref.SELECT_REG_NCOLS == 16 * ref.NT and int(re.search(r"c < min\(ncols, (\d+)\)", src).group(1)) == ref.SAMPLE
    sel = re.findall(r"(?:if \(d\.k <= (\d+)\) |else )GNNLM_TOPK_SELECT\((\d+)\)", src)
    assert [int(b) for a, b in sel] == list(ref.SELECT_KP) and [int(a) for a, b in sel[:-1]] == list(ref.SELECT_KP[:-1])
    mer = re.findall(r"(?:if \(d\.k <= (\d+)\) |else )GNNLM_TOPK_LAUNCH\((\d+)\)", src)
    assert [int(b) for a, b in mer] == list(ref.MERGE_KP) and [int(a) for a, b in mer[:-1]] == [256, 1024]
    assert re.search(r"d\.k > 0 && d\.k <= (\d+)", src).group(1) == str(ref.K_MAX)
    assert re.search(r"constexpr int SB = KP / 2 >= NT \? KP / 2 : NT;", src) and re.search(r"constexpr int NT = (\d+);", src).group(1) == str(ref.NT)
    assert [int(x) for x in re.search(r"for \(int sh = (\d+); sh >= 0; sh -= (\d+)\)", src).groups()] == [55, 11]
    # route() at the thresholds
    def r(nc, k, init, rn=None):
        return ref.route(dict(scores=np.zeros((2, 0), dtype=np.float32), ncols=nc, k=k, init=init, row_ncols=rn))
    assert r(16384, 64, 1) == "select<64,20>" and r(16385, 64, 1) == "merge<512>+prepass" and r(4096, 65, 1) == "select<256,16>"
    assert r(4097, 2048, 1) == "select<2048,20>" and r(1023, 256, 1) == "select<256,16>" and r(1023, 256, 0) == "merge<512>"
    assert r(40000, 257, 0) == "merge<1024>" and r(40000, 1025, 1) == "merge<2048>+prepass"
    assert r(40000, 1025, 1, np.array([4095, -1], dtype=np.int32)) == "merge<2048>" and r(40000, 1025, 1, np.array([4096, 0], dtype=np.int32)) == "merge<2048>+prepass"


def route_counts():
    cnt = collections.Counter(ref.route(select_case(i)) for i in range(len(ref.SELECT_CASES)))
    cnt.update(ref.route(merge_case(i)[0]) for i in range(len(ref.MERGE_CASES)))
    return cnt


def test_every_route_is_covered():
    cnt = route_counts()
    print({r: cnt[r] for r in ref.ALL_ROUTES})
    assert set(cnt) == set(ref.ALL_ROUTES) and all(cnt[r] > 0 for r in ref.ALL_ROUTES)
    ids = [ref.select_case_id(s) for s in ref.SELECT_CASES] + [ref.merge_case_id(s) for s in ref.MERGE_CASES]
    assert len(set(ids)) == len(ids)


def test_select_table_covers_the_issue():
    S = ref.SELECT_CASES
    assert {s["k"] for s in S} == {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048}
    for k in {s["k"] for s in S}:
        assert {k - 1, k, k + 1} <= {s["ncols"] for s in S if s["k"] == k}
    for KP in ref.SELECT_KP:
        sub = [s for s in S if ref._first(ref.SELECT_KP, s["k"]) == KP]
        assert {0, 1, 4095, 4096, 4097, 5119, 5120, 5121, 16384} <= {s["ncols"] for s in sub}, KP
        for ept in (16, 20):
            e = [s for s in sub if (s["ncols"] > ref.SELECT_REG_NCOLS) == (ept == 20) and s["ncols"] > 1]
            assert {s["largest"] for s in e} == {0, 1}, (KP, ept)
    for ept in (16, 20):
        e = [s for s in S if (s["ncols"] > ref.SELECT_REG_NCOLS) == (ept == 20) and s["ncols"] > 1]
        assert {s["idmode"] for s in e} == set(ref.IDMODES) and {s["xf"] for s in e} == set(ref.XF_NAMES)
        assert any(s["ragged"] for s in e) and any(s["col0"] == -5 and s["idmode"] == "col0" for s in e)
        assert any(s["idmode"] == "ids" and s["xf"] != "general" and s["ncols"] > s["k"] for s in e)      # the id-digit rows, with a cut
    assert all(8 <= len(select_case(i)["patterns"]) <= 12 for i in range(len(S)))


def test_merge_table_covers_the_issue():
    Mc = ref.MERGE_CASES
    for KP, ks in ref.MERGE_KS.items():
        SB = ref.sub_block(KP)
        sub = [s for s in Mc if s["init"] == 0 and ref.merge_kp(s["k"]) == KP and s["ragged"] != "cap"]
        assert {(s["chunk"], s["state"]) for s in sub} == {(w, st) for w in (0, 1, 255, 256, 257, SB, SB + 1, 3 * SB + 5) for st in ref.STATES}
        assert {s["k"] for s in sub} == set(ks) and {s["largest"] for s in sub} == {0, 1} and {s["idmode"] for s in sub} == set(ref.IDMODES)
        assert any(s["state"] == "half" and s["largest"] == 0 for s in sub)     # unfilled -1 slots under largest = 0
        assert [s for s in Mc if s["ragged"] == "cap" and ref.merge_kp(s["k"]) == KP and s["idmode"] == "ids" and s["largest"] == 1]
    assert sorted((s["k"], s["largest"]) for s in Mc if s["init"] == 1) == [(8, 0), (8, 1), (1024, 0), (1024, 1), (2048, 0), (2048, 1)]
    assert all(s["chunk"] == 16385 for s in Mc if s["init"] == 1)


def test_tied_states_have_ties_on_both_sides_of_the_ids():
    """'tied' states: values of the chunk equal values of the state, with ids below and above the state's; 'half' states with
    largest = 0 hold unfilled -1 slots."""
    seen_below = seen_above = seen_unfilled = 0
    for i, spec in enumerate(ref.MERGE_CASES):
        if spec["init"] or spec["chunk"] < 255:
            continue
        call, state = merge_case(i)
        if spec["state"] == "half" and spec["largest"] == 0:
            seen_unfilled += int((state[1] < 0).any() and np.isposinf(state[0][state[1] < 0]).all())
        if spec["state"] != "tied":
            continue
        v, ids, ok = ref.values(call), ref.column_ids(call), ref.valid(call)
        below = above = False
        for r in range(len(v)):
            real = state[1][r] >= 0
            for val in np.unique(state[0][r][real])[:8]:
                cid, sid = ids[r][ok[r] & (v[r] == val)], state[1][r][real & (state[0][r] == val)]
                below |= bool(len(cid)) and cid.min() < sid.max()
                above |= bool(len(cid)) and cid.max() > sid.min()
        assert below, ref.merge_case_id(spec)                                   # chunk ids smaller than those of equal values in the state
        seen_below += below
        seen_above += above
    assert seen_below >= 12 and seen_above >= 6 and seen_unfilled >= 3


# ------------------------------------------------------------------------------------------ 6. the rows
def test_digit_rows_tie_across_the_cut_in_one_digit():
    seen = collections.Counter()
    for i, spec in enumerate(ref.SELECT_CASES):
        call = select_case(i)
        if "digit0" not in call["patterns"] or spec["ncols"] <= spec["k"] or spec["ncols"] < 2:
            continue
        v, ids, ok = ref.values(call), ref.column_ids(call), ref.valid(call)
        out_v, out_i = ref.fold(call)
        for s in ref.DIGIT_SHIFTS:
            r = call["patterns"].index(f"digit{s}")
            assert ok[r].all()
            cut = out_v[r, -1]                                                  # the k-th best value
            run = ids[r][v[r] == cut]
            taken = int((out_v[r] == cut).sum())
            assert 0 < taken < len(run), (i, s)                                 # the cut falls inside the run
            width = 0xFF if s == 55 else 0x7FF
            assert len(set((run & ~np.int64(width << s)).tolist())) == 1 and len(set(((run >> s) & width).tolist())) == len(run), (i, s)
            seen[(s, spec["ncols"] > ref.SELECT_REG_NCOLS)] += 1
    assert all(seen[(s, wide)] >= 2 for s in ref.DIGIT_SHIFTS for wide in (False, True)), seen


def test_rows_are_what_their_names_say():
    call = ref.make_case(dict(k=100, ncols=6000, largest=0, idmode="col0", xf="dyadic", seed=3, ragged=False, init=1))
    v, ok, P = ref.values(call), ref.valid(call), call["patterns"]
    g = -v                                                                      # goodness for largest = 0
    assert (np.diff(g[P.index("ascending")]) > 0).all() and (np.diff(g[P.index("descending")]) < 0).all()
    assert len(np.unique(v[P.index("constant")])) == 1 and len(np.unique(v[P.index("few_distinct")])) == 5
    assert not ok[P.index("sample_invalid"), :ref.SAMPLE].any() and ok[P.index("sample_invalid"), ref.SAMPLE:].all()
    sc = v[P.index("sample_constant")]
    assert len(np.unique(sc[:ref.SAMPLE])) == 1 and (sc[ref.SAMPLE:] < sc[0]).any() and (sc[ref.SAMPLE:] > sc[0]).any()
    rt = v[P.index("random_ties")]
    assert 1000 < len(np.unique(rt)) < 6000
    sp = ref.values(ref.make_case(dict(k=100, ncols=60, largest=1, idmode="col0", xf="none", seed=3, ragged=False, init=1)))[-1]
    assert np.isnan(sp).any() and np.isposinf(sp).any() and np.isneginf(sp).any() and (np.signbit(sp) & (sp == 0)).any()
    assert ((sp != 0) & (np.abs(sp) < 1.17549435e-38)).sum() >= 8               # denormals, of both signs
    gen = ref.make_case(dict(k=100, ncols=6000, largest=1, idmode="col_ids", xf="general", seed=4, ragged=True, init=1))
    assert (gen["col_scale"] < 0).any() and (gen["col_scale"] > 0).any() and gen["alpha"] == 0.7
    # a fused multiply-add would give other bits on this data: the rounding order is visible to the cases of the "general" transform
    p = (gen["scores"].astype(np.float64) * np.float32(0.7)).astype(np.float32).astype(np.float64)
    fused = (p * gen["col_scale"].astype(np.float64) + gen["col_bias"].astype(np.float64)).astype(np.float32)
    live = ref.valid(gen)
    assert (fused[live] != ref.values(gen)[live]).mean() > 0.05
    beyond = np.arange(6000)[None, :] >= gen["row_ncols"][:, None]
    assert np.isposinf(ref.values(gen)[beyond]).all() and beyond.sum() > 6000   # the winning infinity beyond row_ncols
