"""tests/gather_ref.py is right before it judges a kernel, and the inputs of tests/test_gather_abi_gpu.py can tell a kernel that ignores a
descriptor field from one that honours it.  No GPU.

1. gather_ref equals the project's oracle (oracle.graph.slot_layout + oracle.pq.pq_lookup) on what the oracle can express: a store,
   with the window applied to the oracle's rows; no direct codes, no shards.
2. Every case takes the route written next to it (gather_route restates the dispatch of gather_decode()); the two grid-cap cases exceed
   the caps.  No index of a valid slot leaves its buffer.
3. For every case and every field it sets, the reference with that one field neutralised or shifted by one differs in an output the case
   asks for.
4. pq_encode: the derived bound of encode_ref holds for a float32 emulation of the kernel's chain; at least 95 % of the entries of every
   random case are decided exactly; in the tie cases only the duplicates can win, and wrong tie rules give other codes.
5. The ctypes mirrors carry every field the tables use."""
import numpy as np
import pytest

import gather_ref as ref
from oracle import graph as og
from oracle import pq as opq

OUT_INDEX = {"x": 0, "c": 1, "l": 2, "v": 3}
GATHER_FIELDS = ["codes", "vals", "vals_itemsize", "n_store", "row0", "n_local", "M", "dsub", "centroids", "ids", "n_groups", "left", "right",
                 "out_x", "ld_x", "out_codes", "out_labels", "out_valid", "direct", "in_valid", "in_index", "shards", "n_groups_dev"]
SHARDS_FIELDS = ["n", "rows_per_rank", "base", "row0", "rows"]
PEER_FIELDS = ["shard", "shard_row0", "shard_rows", "world", "row_bytes", "rows_per_rank", "n_store", "rows", "n", "out", "out_valid"]


def same(a, b, outs):
    """the outputs a case asks for, and the write mask, are equal as bits"""
    return np.array_equal(a[4], b[4]) and all(np.array_equal(a[OUT_INDEX[o]].view(np.uint8), b[OUT_INDEX[o]].view(np.uint8)) for o in outs)


# ------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("case", [c for c in ref.GATHER_CASES if "win" in c[1] and c[1].get("G", 0) < 10 ** 5], ids=ref.gather_case_id)
def test_gather_ref_is_the_oracle(case):
    c = ref.make_gather_case(*case)
    kw = dict(c["kw"], outs="xclv")
    x, codes, labels, valid, written = ref.gather_ref(kw)
    G = kw["n_groups"]
    rows, ok = og.slot_layout(kw["ids"][:G].reshape(-1, 1), kw["n_store"], kw["left"], kw["right"])
    rows, ok = rows.reshape(-1), ok.reshape(-1)
    ok = ok & (rows >= kw["row0"]) & (rows < kw["row0"] + kw["n_local"])
    assert np.array_equal(valid != 0, ok)
    if ok.any():
        want = opq.pq_lookup(kw["codes"][np.where(ok, rows - kw["row0"], 0)], kw["centroids"])
        assert np.array_equal(x[ok].view(np.uint32), np.ascontiguousarray(want[ok]).view(np.uint32))
        assert np.array_equal(codes[ok], kw["codes"][(rows - kw["row0"])[ok]])
        if kw.get("vals") is not None:
            assert np.array_equal(labels[ok], kw["vals"][(rows - kw["row0"])[ok]].astype(np.int64))
            assert kw["vals"].dtype != np.int16 or (labels[ok] < 0).any()
    assert not x[~ok].any() and not codes[~ok].any() and (labels[~ok] == -1).all()
    assert np.array_equal(written, np.arange(len(ok)) < min(G, kw.get("n_groups_dev", G)) * c["n_g"])


# ------------------------------------------------------------------------------------------ 2. routes, caps, bounds
def test_gather_tables_cover_both_routes():
    ids = [ref.gather_case_id(c) for c in ref.GATHER_CASES]
    assert len(set(ids)) == len(ids)
    for route in ("rows", "wave"):
        sub = [s for r, s in ref.GATHER_CASES if r == route]
        assert {s["vals"] for s in sub} == {"i16", "i32", None}
        assert {s.get("win") for s in sub} >= {"win", "win_ns", "none", "empty"}
        assert {s.get("ngd") for s in sub} >= {"0", "1", "G-1", "G", "G+5"}
    wave = [s for r, s in ref.GATHER_CASES if r == "wave"]
    assert {(s["M"], s["dsub"]) for _, s in ref.GATHER_CASES} >= {(8, 4), (16, 8), (128, 8), (24, 4)}
    assert {(s.get("left", 0), s.get("right", 0)) for s in wave} >= {(0, 0), (2, 2), (3, 1), (0, 2)}
    assert {"".join(sorted(s["outs"])) for _, s in ref.GATHER_CASES} == \
        {"".join(sorted(o for k, o in enumerate("xclv") if n >> k & 1)) for n in range(1, 16)}
    assert {s["shards"][0] for s in wave if "shards" in s} == {1, 3, 16}
    assert {s["direct"] for s in wave if "direct" in s} == {"valid", "index"} and any(s.get("ids_null") for s in wave)


def test_gather_grid_cap_cases():
    (rw, w), (rr, r) = [c for c in ref.GATHER_CASES if c[1].get("G", 0) > 10 ** 4]
    assert (rw, rr) == ("wave", "rows")
    slots = w["G"] * (1 + w["left"] + w["right"])
    assert 4 * ref.WAVE_CAP < slots < 5 * ref.WAVE_CAP                      # every wave walks four slots, some a fifth
    total = r["G"] * (r["M"] // 16)
    assert 4 * ref.ROWS_CAP < total < 5 * ref.ROWS_CAP                      # a full trip of four pieces per thread, then a partial one
    assert r.get("left", 0) == r.get("right", 0) == 0


@pytest.mark.parametrize("case", ref.GATHER_CASES, ids=ref.gather_case_id)
def test_gather_case_inputs(case):
    c = ref.make_gather_case(*case)
    kw, spec = c["kw"], c["spec"]
    assert ref.gather_route(kw) == c["route"]
    out = ref.gather_ref(kw)
    valid, written = out[3] != 0, out[4]
    G, n_g = kw["n_groups"], c["n_g"]
    # no valid slot leaves its buffer
    if kw.get("direct"):
        idx = kw.get("in_index")
        assert len(kw["in_valid"]) >= c["S"] and (idx is None or (idx[:c["S"]][valid] < len(kw["codes"])).all())
        assert idx is None or ((idx == -1) == (kw["in_valid"] == 0)).all() and len(np.unique(idx[idx >= 0])) < (idx >= 0).sum()
        assert idx is not None or len(kw["codes"]) >= c["S"]
        assert kw.get("vals") is None or len(kw["vals"]) == len(kw["codes"])
    elif kw.get("shards") is not None:
        sh = kw["shards"]
        assert all(b is None and n == 0 or len(b) == n for b, n in zip(sh["base"], sh["rows"]))
        assert sh["n"] * sh["rows_per_rank"] < kw["n_store"] and kw["n_store"] % sh["rows_per_rank"]
        centre = set(kw["ids"][:G].tolist())
        assert set(ref.halo_ids(sh["n"], sh["rows_per_rank"], kw["n_store"])) <= centre
    elif spec["win"] != "empty":
        assert kw["n_local"] <= len(kw["codes"]) and (kw.get("vals") is None or kw["n_local"] <= len(kw["vals"]))
        centre = set(kw["ids"][:G].tolist())
        assert {-1, 0, 1, kw["n_store"] - 1, kw["n_store"], ref.FAR_ID} <= centre
        assert {kw["row0"] - 1, kw["row0"], kw["row0"] + kw["n_local"] - 1, kw["row0"] + kw["n_local"]} <= centre
    else:
        assert "codes" not in kw and not valid.any()
    if spec.get("win") != "empty" and kw.get("n_groups_dev", G) > 1:
        assert valid[written].any() and not valid[written].all()
    if "ids" in kw and not kw.get("direct"):
        assert len(kw["ids"]) == G + ref.SLACK_GROUPS
    # one field neutralised at a time
    for what, kw2, opts in ref.gather_neutralised(c):
        assert ref.gather_route(kw2) == c["route"], what
        assert not same(out, ref.gather_ref(kw2, **opts), kw["outs"]), what
    fields = len(ref.gather_neutralised(c))
    assert fields >= (("ngd" in spec) + ("shards" in spec) + ("direct" in spec) + (spec.get("direct") == "index") if spec.get("win") != "empty" else 0)


# ------------------------------------------------------------------------------------------ 4. pq_encode
@pytest.mark.parametrize("case", ref.ENCODE_CASES, ids=ref.encode_case_id)
def test_encode_bound_holds_for_the_float32_chain(case):
    c = ref.make_encode_case(case)
    x = c["x"][:, :c["M"] * c["dsub"]]
    dist, B = ref.encode_ref(x, c["cen"], c["norm2"])
    emu = ref.encode_emulate(x, c["cen"], c["norm2"])
    worst = float((np.abs(emu.astype(np.float64) - dist) / B).max())
    assert worst < 1.0, worst
    # the float32 argmin (lowest index on ties) passes the test the kernel's codes get, and the case is not hollow
    excess, share, wrong = ref.encode_judge(emu.argmin(-1).astype(np.uint8), dist, B)
    assert excess <= 1.0 and wrong == 0, (excess, share, wrong)
    assert share >= 0.95 or case["n"] * case["M"] < 100, share                                      # (one near-tie in 18 entries is 5.6 %)


@pytest.mark.parametrize("M,dsub", ref.ENCODE_SHAPES)
def test_encode_cases_are_decided(M, dsub):
    share = ref.encode_shape_share(M, dsub)
    print(f"pq_encode M={M} dsub={dsub}: {100 * share:.2f} % of the entries decided exactly")
    assert share >= 0.95


@pytest.mark.parametrize("case", ref.TIE_CASES, ids=ref.encode_case_id)
def test_encode_tie_cases_tie(case):
    c = ref.make_encode_case(case)
    dup = list(case["dup"])
    x = c["x"][:, :c["M"] * c["dsub"]]
    assert all(np.array_equal(c["cen"][:, d].view(np.uint32), c["cen"][:, dup[0]].view(np.uint32)) for d in dup)
    assert (c["norm2"][:, dup].view(np.uint32) == c["norm2"][:, dup[:1]].view(np.uint32)).all()
    dist, B = ref.encode_ref(x, c["cen"], c["norm2"])
    emu = ref.encode_emulate(x, c["cen"], c["norm2"])
    assert (emu[:, :, dup].view(np.uint32) == emu[:, :, dup[:1]].view(np.uint32)).all()          # equal as bits whatever the rounding
    others = np.delete(dist, dup, axis=-1).min(-1)
    assert (others - dist[:, :, dup[0]] > 4 * B.max(-1)).all()                                     # nothing else can win
    assert (c["want"] == min(dup)).all()


def test_encode_tie_sets_separate_the_rules():
    """the kernel's rule gives the lowest index on every set; every wrong rule gives another code on some set, every set catches some
    wrong rule, and the sets named for one half of the rule catch the wrong rules of that half"""
    wrong = {"highest index": lambda d: max(d),
             "first lane, whatever the index": lambda d: min(d, key=lambda c: (c % 64, c)),
             "in-lane: last": lambda d: ref.tie_winner(d, in_lane="last"),
             "cross-lane: keep mine": lambda d: ref.tie_winner(d, cross="keep"),
             "cross-lane: take the other": lambda d: ref.tie_winner(d, cross="take")}
    assert all(ref.tie_winner(d) == min(d) for d in ref.TIE_SETS)
    miss = {name: [d for d in ref.TIE_SETS if rule(d) != min(d)] for name, rule in wrong.items()}
    assert all(miss.values()), miss
    assert all(any(d in m for m in miss.values()) for d in ref.TIE_SETS)
    assert (7, 71, 135, 199) in miss["in-lane: last"] and (200, 7, 71) in miss["in-lane: last"]
    assert (7, 8) in miss["cross-lane: keep mine"] and (7, 39) in miss["cross-lane: take the other"]
    assert (63, 64) in miss["first lane, whatever the index"] and (0, 255) in miss["highest index"]
    for name, rule in wrong.items():                        # as code matrices
        got = [np.full_like(ref.make_encode_case(t)["want"], rule(t["dup"])) for t in ref.TIE_CASES]
        assert any((g != ref.make_encode_case(t)["want"]).any() for g, t in zip(got, ref.TIE_CASES)), name


# ------------------------------------------------------------------------------------------ gather_rows_peer
@pytest.mark.parametrize("case", ref.PEER_CASES, ids=ref.peer_case_id)
def test_peer_case_inputs(case):
    c = ref.make_peer_case(*case)
    kw = c["kw"]
    assert ref.peer_route(kw["row_bytes"]) == c["route"]
    out, valid = ref.peer_ref(kw)
    rows, sh = kw["rows"], kw["shards"]
    assert {-1, 0, kw["n_store"] - 1, kw["n_store"]} <= set(rows.tolist()) and kw["n_store"] % kw["rows_per_rank"]
    assert kw["n"] % 256 and (kw["n"] * max(1, kw["row_bytes"] // 16)) % 256
    assert 0 < valid.sum() < kw["n"] and not out[valid == 0].any()
    inside = (rows >= 0) & (rows < kw["n_store"])
    assert c["spec"]["variant"] == "full" or (inside & (valid == 0)).any()              # a row of the store its owner does not hold
    assert c["spec"]["variant"] != "empty" or (sh["base"][min(1, sh["n"] - 1)] is None and 0 in sh["rows"])
    if sh["n"] > 1:                                                                     # halo rows are served by their owner only
        assert set(ref.halo_ids(sh["n"], kw["rows_per_rank"], kw["n_store"])) <= set(rows.tolist())
        out2, valid2 = ref.peer_ref(kw, owner_rule="any")
        assert c["spec"]["variant"] == "full" or not np.array_equal(valid, valid2)
    # against the table itself: a held row is the table's row
    table = np.zeros((kw["n_store"], kw["row_bytes"]), dtype=np.uint8)
    for b, r0 in zip(sh["base"], sh["row0"]):
        if b is not None:
            table[r0:r0 + len(b)] = b
    assert np.array_equal(out[valid != 0], table[rows[valid != 0]])


def test_peer_table_covers_the_issue():
    assert {s["row_bytes"] for _, s in ref.PEER_CASES} == {1, 2, 4, 12, 16, 48, 128}
    assert {s["world"] for _, s in ref.PEER_CASES} == {1, 3, 16}
    for rb in ref.PEER_ROW_BYTES:
        assert {s["out_valid"] for _, s in ref.PEER_CASES if s["row_bytes"] == rb} == {True, False}


# ------------------------------------------------------------------------------------------ 5. mirrors
def test_mirrors_carry_the_fields():
    from gnnlm_amd import _lib
    assert set(GATHER_FIELDS) <= {f for f, _ in _lib.gnnlm_gather_t._fields_}
    assert set(SHARDS_FIELDS) <= {f for f, _ in _lib.gnnlm_shards_t._fields_}
    assert set(PEER_FIELDS) <= {f for f, _ in _lib.gnnlm_peer_gather_t._fields_}
