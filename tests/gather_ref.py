"""numpy restatement of gnnlm_pq_gather_decode, gnnlm_pq_encode and gnnlm_gather_rows_peer driven by the DESCRIPTOR fields
(include/gnnlm.h: gnnlm_gather_t, gnnlm_shards_t, gnnlm_peer_gather_t), and the case tables of tests/test_gather_abi_gpu.py.  Plain
numpy; nothing here imports gnnlm_amd, and the rules are the header's comments, not the kernels.

A buffer is the array that starts at the pointer the kernel is handed (``codes`` of a store window is the table from row ``row0`` on).
The references never read what the rule excludes.  Gathered data is compared as bits: a gather copies, it does not compute.  Centre ids
are -1 or >= 0, as the neighbour search produces them (the header's "ids[g] != -1"); other negative centres are outside the tables.

The one tolerance of this module is the bound B of encode_ref, derived there."""
import functools
import zlib

import numpy as np

N_STORE = 1000                      # rows of the whole store in the gather cases
ROW0, N_LOCAL = 300, 500            # the window of the cases that have one: rows [300, 800)
N_STORE_IN = 700                    # flavour "win_ns": the store ends inside the window, so the n_store bound decides
SLACK_GROUPS = 5                    # ids / in_valid / in_index hold this many groups more than n_groups (valid, in-bounds data)
FAR_ID = 10 ** 12

# grid caps of gather_decode() (csrc/gather_decode.hip): at most 256 * 16 workgroups of 256 threads
CAP_BLOCKS = 256 * 16
WAVE_CAP = CAP_BLOCKS * 4           # waves of gather_decode_kernel (one slot per wave per trip)
ROWS_CAP = CAP_BLOCKS * 256         # threads of gather_rows_kernel (four 16-byte pieces per thread per trip)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def slot_delta(left, right):
    """row offset of slot c of a group: centre, then o-left .. o-1, then o+1 .. o+right"""
    return np.concatenate([[0], np.arange(-left, 0), np.arange(1, right + 1)]).astype(np.int64)


# ======================================================================================================== shards
def make_shards(table, world, per, variant="full", halo=2):
    """A range-sharded table as gnnlm_shards_t / gnnlm_peer_gather_t describe it: shard g is a COPY of the rows rank g holds -- its
    range [g * per, (g + 1) * per) (the last one up to the end of the table) plus ``halo`` rows on either side.  variant "hole": shard
    1 (shard 0 of a single one) lost all but its first 10 rows; "empty": it holds no row and has no base."""
    n = len(table)
    base, row0, rows = [], [], []
    for g in range(world):
        lo = max(0, g * per - halo)
        hi = n if g == world - 1 else min(n, (g + 1) * per + halo)
        if g == min(1, world - 1) and variant == "hole":
            hi = lo + 10
        if g == min(1, world - 1) and variant == "empty":
            base.append(None), row0.append(0), rows.append(0)
            continue
        base.append(table[lo:hi].copy()), row0.append(lo), rows.append(hi - lo)
    return dict(n=world, rows_per_rank=per, base=base, row0=row0, rows=rows)


def shard_lookup(sh, row, ok, owner_rule="owner"):
    """-> (shard index, local row, held) per request; rule "owner": only shard min(n - 1, row / rows_per_rank) is asked; "any" (a
    perturbation, NOT the rule): the first shard that holds the row."""
    n = sh["n"]
    r = np.where(ok, row, 0)
    r0, rw = np.asarray(sh["row0"], dtype=np.int64), np.asarray(sh["rows"], dtype=np.int64)
    if owner_rule == "owner":
        g = np.minimum(n - 1, r // sh["rows_per_rank"])
    else:
        holds = (r[:, None] >= r0[None, :]) & (r[:, None] < (r0 + rw)[None, :])
        g = np.where(holds.any(1), holds.argmax(1), 0)
    loc = r - r0[g]
    return g, loc, ok & (loc >= 0) & (loc < rw[g])


def shard_rows(sh, g, loc, held, width):
    out = np.zeros((len(g), width), dtype=np.uint8)
    for k in range(sh["n"]):
        sel = held & (g == k)
        if sel.any():
            out[sel] = sh["base"][k][loc[sel]]
    return out


def halo_ids(world, per, n):
    """ids on both sides of every shard boundary, two rows deep and one beyond (the halo is two rows)"""
    return [b + d for g in range(1, world) for b in [g * per] for d in (-3, -2, -1, 0, 1, 2) if 0 <= b + d < n]


# ======================================================================================================== gather_decode
def gather_ref(kw, owner_rule="owner", int16_unsigned=False):
    """-> (x float32 [S, D] or None when "x" is not in kw["outs"], codes uint8 [S, M], labels int32 [S], valid uint8 [S],
    written bool [S]);  S = n_groups * (1 + left + right).  Rows outside ``written`` must keep what they held."""
    M, dsub = kw["M"], kw["dsub"]
    left, right, G = kw.get("left", 0), kw.get("right", 0), kw["n_groups"]
    n_g = 1 + left + right
    S = G * n_g
    ngd = kw.get("n_groups_dev")
    cnt = G if ngd is None else max(0, min(G, int(ngd)))
    written = np.arange(S) < cnt * n_g
    vals = kw.get("vals")
    if kw.get("direct"):
        ok = np.asarray(kw["in_valid"])[:S] != 0
        lrow = np.arange(S, dtype=np.int64) if kw.get("in_index") is None else np.asarray(kw["in_index"])[:S].astype(np.int64)
        codes = np.where(ok[:, None], kw["codes"][np.where(ok, lrow, 0)], 0).astype(np.uint8)
    else:
        ids = np.asarray(kw["ids"], dtype=np.int64)[:G]
        row = (ids[:, None] + slot_delta(left, right)[None, :]).reshape(-1)
        ok = np.repeat(ids != -1, n_g) & (row >= 0) & (row < kw["n_store"])
        if kw.get("shards") is not None:
            g, loc, ok = shard_lookup(kw["shards"], row, ok, owner_rule)
            codes = shard_rows(kw["shards"], g, loc, ok, M)
            vals = None                                                                # a shard table carries no labels
        else:
            lrow = row - kw.get("row0", 0)
            ok = ok & (lrow >= 0) & (lrow < kw.get("n_local", 0))
            codes = np.where(ok[:, None], kw["codes"][np.where(ok, lrow, 0)], 0).astype(np.uint8) if ok.any() else np.zeros((S, M), np.uint8)
    labels = np.full(S, -1, dtype=np.int32)
    if vals is not None and ok.any():
        v = np.asarray(vals)[np.where(ok, lrow, 0)]
        if int16_unsigned and v.dtype == np.int16:
            v = v.view(np.uint16)
        labels = np.where(ok, v.astype(np.int32), -1).astype(np.int32)
    x = None
    if "x" in kw["outs"]:
        x = kw["centroids"][np.arange(M)[None, :], codes.astype(np.int64)].reshape(S, M * dsub)
        x = np.where(ok[:, None], x, np.float32(0)).astype(np.float32)
    return x, codes, labels, ok.astype(np.uint8), written


def gather_route(kw):
    """The kernel gather_decode() launches: "rows" (gather_rows_kernel, 16-byte pieces) or "wave" (gather_decode_kernel)."""
    rows = kw.get("shards") is None and not kw.get("direct") and "x" not in kw["outs"] and "c" in kw["outs"] and \
        kw.get("left", 0) == 0 and kw.get("right", 0) == 0 and kw["M"] % 16 == 0 and \
        kw.get("codes_mod16", 0) == 0 and kw.get("out_codes_mod16", 0) == 0
    return "rows" if rows else "wave"


def _cases():
    cases = []

    def add(route, **spec):
        cases.append((route, spec))

    VALS = ["i16", "i32", None]
    # -- every non-empty subset of the outputs at M = 16 (left = right = 0: the codes-without-x subsets take the 16-byte-row kernel)
    for n, outs in enumerate(["c", "cl", "cv", "clv"]):
        add("rows", M=16, dsub=8, outs=outs, vals=VALS[n % 3], win="win")
    for n, outs in enumerate(["x", "l", "v", "xc", "xl", "xv", "lv", "xcl", "xcv", "xlv", "xclv"]):
        add("wave", M=16, dsub=8, outs=outs, vals=VALS[n % 3], win="win", ld_pad=8 * (n % 2))
    # -- the other shapes; M = 24 and M = 8 stay on the wave kernel even for a codes-only request
    for n, outs in enumerate(["c", "clv"]):
        add("rows", M=128, dsub=8, outs=outs, vals=VALS[n], win="win_ns")
        add("wave", M=8, dsub=4, outs=outs, vals=VALS[n], win="win_ns")
        add("wave", M=24, dsub=4, outs=outs, vals=VALS[n + 1], win="win")
    for n, (M, dsub) in enumerate([(8, 4), (128, 8), (24, 4)]):
        add("wave", M=M, dsub=dsub, outs="xclv", vals=VALS[n % 2], win="win", ld_pad=8)
        add("wave", M=M, dsub=dsub, outs="x", vals=None, win="none")
    # -- the label table on both routes: int16 (negative values), int32, none
    for v in VALS:
        add("rows", M=16, dsub=4, outs="cl", vals=v, win="win_ns")
        add("wave", M=24, dsub=4, outs="cl", vals=v, win="win_ns")
        add("wave", M=16, dsub=4, outs="xl", vals=v, win="none", ld_pad=8)
    add("rows", M=16, dsub=8, outs="clv", vals="i32", win="none")
    # -- neighbour context: any left / right leaves the 16-byte-row kernel
    for left, right in [(2, 2), (3, 1), (0, 2)]:
        for M, dsub in [(8, 4), (16, 8)]:
            add("wave", M=M, dsub=dsub, outs="xclv", vals="i16", win="win", left=left, right=right, ld_pad=8)
            add("wave", M=M, dsub=dsub, outs="c", vals=None, win="none", left=left, right=right)
    # -- an empty local shard: codes = NULL, every slot invalid
    add("rows", M=16, dsub=8, outs="cv", vals=None, win="empty")
    add("wave", M=16, dsub=8, outs="xclv", vals=None, win="empty", left=1, right=1)
    # -- operands that miss the 16-byte alignment of the row kernel
    add("wave", M=16, dsub=8, outs="clv", vals="i32", win="win", misalign="out")
    add("wave", M=16, dsub=8, outs="clv", vals="i16", win="win", misalign="codes")
    # -- direct = 1: an already-fetched code buffer
    for M, dsub, left, right in [(8, 4, 0, 0), (16, 8, 2, 2), (128, 8, 0, 0)]:
        add("wave", M=M, dsub=dsub, outs="xclv", vals=None, direct="valid", left=left, right=right, ld_pad=8)
        add("wave", M=M, dsub=dsub, outs="xclv", vals="i16", direct="index", left=left, right=right)
        add("wave", M=M, dsub=dsub, outs="c", vals=None, direct="index", left=left, right=right, ids_null=True)
    add("wave", M=16, dsub=8, outs="clv", vals="i32", direct="valid", ids_null=True)
    # -- mapped shards
    for world in (1, 3, 16):
        for variant in ("full", "hole", "empty")[:2 if world == 1 else 3]:
            add("wave", M=16, dsub=8, outs="xcv", vals=None, shards=(world, variant), ld_pad=8)
            add("wave", M=16, dsub=8, outs="c", vals=None, shards=(world, variant))
        add("wave", M=8, dsub=4, outs="xclv", vals=None, shards=(world, "hole"), left=2, right=2)
        add("wave", M=128, dsub=8, outs="lv", vals=None, shards=(world, "full"), left=3, right=1)
    # -- a device-side group count
    for ngd in ("0", "1", "G-1", "G", "G+5"):
        add("rows", M=16, dsub=8, outs="clv", vals="i32", win="win", ngd=ngd)
        add("wave", M=8, dsub=4, outs="xclv", vals="i16", win="win", ngd=ngd, left=2, right=2, ld_pad=8)
    add("wave", M=16, dsub=8, outs="xclv", vals=None, direct="index", ngd="G-1", left=0, right=2)
    add("wave", M=16, dsub=8, outs="xcv", vals=None, shards=(3, "full"), ngd="G-1")
    # -- the grid caps: every wave walks four slots and some a fifth; the unrolled loop of the row kernel runs a second, partial trip
    add("wave", M=8, dsub=4, outs="xclv", vals="i16", win="win", left=1, right=1, G=4 * WAVE_CAP // 3 + 55, ngd="G")
    add("rows", M=16, dsub=4, outs="clv", vals="i32", win="win", G=4 * ROWS_CAP + 1000)
    return cases


GATHER_CASES = _cases()
NGD = {"0": lambda G: 0, "1": lambda G: 1, "G-1": lambda G: G - 1, "G": lambda G: G, "G+5": lambda G: G + 5}


def gather_case_id(case):
    route, s = case
    mode = "direct-" + s["direct"] if "direct" in s else "shards%d-%s" % s["shards"] if "shards" in s else s["win"]
    return f"{route}-M{s['M']}x{s['dsub']}-l{s.get('left', 0)}r{s.get('right', 0)}-{s['outs']}-{s['vals']}-{mode}" + \
        (f"-ld+{s['ld_pad']}" if s.get("ld_pad") else "") + (f"-ngd{s['ngd']}" if "ngd" in s else "") + \
        (f"-G{s['G']}" if "G" in s else "") + ("-noids" if s.get("ids_null") else "") + (f"-mis-{s['misalign']}" if "misalign" in s else "")


def edge_ids(n_store, row0, n_local, left, right):
    e = [-1, 0, 1, n_store - 1, n_store, FAR_ID]
    e += list(range(0, left + 1)) + list(range(n_store - 1 - right, n_store + left + 1))
    e += list(range(row0 - right - 1, row0 + left + 2)) + list(range(row0 + n_local - right - 2, row0 + n_local + left + 2))
    return [i for i in e if i >= -1]


def make_gather_case(route, spec):
    """-> dict(route, spec, kw = the descriptor's fields as gather_ref reads them, code_buf / code_off and vals_buf / vals_off = the
    whole buffers and the row at which the descriptor's pointers start, S, n_g, D, ld_x)"""
    M, dsub = spec["M"], spec["dsub"]
    left, right = spec.get("left", 0), spec.get("right", 0)
    n_g = 1 + left + right
    G = spec.get("G", 301)
    rs = _rs(route, sorted(spec.items(), key=str))
    D = M * dsub
    vdt = {"i16": np.int16, "i32": np.int32, None: None}[spec["vals"]]
    kw = dict(M=M, dsub=dsub, left=left, right=right, n_groups=G, outs=spec["outs"], ld_x=D + spec.get("ld_pad", 0),
              centroids=rs.randn(M, 256, dsub).astype(np.float32))
    c = dict(route=route, spec=spec, kw=kw, S=G * n_g, n_g=n_g, D=D, code_off=0, vals_off=0, code_buf=None, vals_buf=None)
    GS = G + SLACK_GROUPS

    def label_table(n):
        lo, hi = (-32768, 32768) if vdt == np.int16 else (-2 ** 31, 2 ** 31)
        return rs.randint(lo, hi, size=n, dtype=np.int64).astype(vdt)

    if "direct" in spec:
        S = GS * n_g
        in_valid = (rs.rand(S) < 0.7).astype(np.uint8) * rs.choice([1, 2, 255], size=S).astype(np.uint8)
        in_valid[:n_g] = 0                                                             # a whole group without a row
        kw.update(direct=1, in_valid=in_valid)
        if spec["direct"] == "index":
            R = S // 3                                                                 # fewer rows than slots: a permutation with repeats
            index = rs.randint(0, R, size=S).astype(np.int32)
            index[in_valid == 0] = -1                                                  # as nb_code_rows produces it
            kw["in_index"] = index
        else:
            R = S
        c["code_buf"] = kw["codes"] = rs.randint(0, 256, size=(R, M)).astype(np.uint8)
        if vdt is not None:
            c["vals_buf"] = kw["vals"] = label_table(R)
        if not spec.get("ids_null"):
            kw["ids"] = np.full(GS, -1, dtype=np.int64)                                # ignored: a kernel that looked would find no row
        return c

    if "shards" in spec:
        world, variant = spec["shards"]
        n_store = N_STORE + 1
        per = {1: 600, 3: 300, 16: 60}[world]                                          # world * per < n_store: the last shard takes the rest
        table = rs.randint(0, 256, size=(n_store, M)).astype(np.uint8)
        kw.update(n_store=n_store, shards=make_shards(table, world, per, variant))
        edges = edge_ids(n_store, 0, n_store, left, right) + halo_ids(world, per, n_store)
        row0, n_local = 0, n_store
    else:
        win = spec["win"]
        n_store = N_STORE_IN if win == "win_ns" else N_STORE
        row0, n_local = (0, N_STORE) if win == "none" else (ROW0, 0) if win == "empty" else (ROW0, N_LOCAL)
        kw.update(n_store=n_store, row0=row0, n_local=n_local)
        if win != "empty":
            # the whole table, and row0 rows more behind it: a kernel that ignored row0 or n_local would stay inside the buffer
            buf = rs.randint(0, 256, size=(N_STORE + row0 + 8, M)).astype(np.uint8)
            c.update(code_buf=buf, code_off=row0)
            kw["codes"] = buf[row0:]
            if vdt is not None:
                vb = label_table(len(buf))
                c.update(vals_buf=vb, vals_off=row0)
                kw["vals"] = vb[row0:]
        edges = edge_ids(n_store, row0, n_local, left, right)
    ids = rs.randint(0, n_store + 30, size=GS).astype(np.int64)
    ids[rs.rand(GS) < 0.1] = -1
    ids[G:] = rs.randint(row0 + left, max(row0 + left + 1, min(n_store, row0 + n_local) - right), size=SLACK_GROUPS)
    pos = rs.choice(G, size=len(edges), replace=False) if G > len(edges) else np.arange(len(edges)) % G
    ids[pos] = edges
    kw["ids"] = ids
    if "ngd" in spec:
        kw["n_groups_dev"] = NGD[spec["ngd"]](G)
    if spec.get("misalign") == "out":
        kw["out_codes_mod16"] = 4
    if spec.get("misalign") == "codes":
        kw["codes_mod16"] = 8
    return c


def gather_neutralised(c):
    """[(what, kw with that one field neutralised or shifted by one, keyword arguments of gather_ref)] for every field the case sets"""
    kw, spec, res = c["kw"], c["spec"], []
    G, n_g = kw["n_groups"], c["n_g"]
    if spec.get("win") == "empty":                          # every slot is invalid whatever the other fields say
        return res
    if (kw["left"] or kw["right"]) and not kw.get("direct"):    # (with direct codes the two only count the slots)
        l2, r2 = (kw["left"] - 1, kw["right"] + 1) if kw["left"] else (kw["left"] + 1, kw["right"] - 1)
        res.append(("left / right shifted", dict(kw, left=l2, right=r2), {}))
    if kw.get("vals") is not None and "l" in kw["outs"]:
        res.append(("vals ignored", dict(kw, vals=None), {}))
        if kw["vals"].dtype == np.int16:
            res.append(("int16 read as unsigned", kw, dict(int16_unsigned=True)))
    if "n_groups_dev" in kw:
        ngd = kw["n_groups_dev"]
        # (above n_groups the count is clamped and +- 1 moves nothing: there the guards behind the outputs watch the clamp)
        res += [(f"n_groups_dev -> {m}", dict(kw, n_groups_dev=m), {}) for m in ((ngd - 1, ngd + 1) if ngd <= G else (G - 1,)) if 0 <= m <= G]
    if kw.get("direct"):
        res.append(("in_valid ignored", dict(kw, in_valid=np.ones_like(kw["in_valid"]), in_index=None if kw.get("in_index") is None else
                                             np.maximum(kw["in_index"], 0)), {}))
        if kw.get("in_index") is not None:
            res.append(("in_index rolled", dict(kw, in_index=np.roll(kw["in_index"], 1)), {}))
            res.append(("in_index -> identity", dict(kw, in_index=np.arange(len(kw["in_index"]), dtype=np.int32) % len(kw["codes"])), {}))
    elif kw.get("shards") is not None:
        sh = kw["shards"]
        if sh["n"] > 1 and spec["shards"][1] != "full":        # (a full shard holds whatever its neighbours' halos hold)
            res.append(("owner rule -> any shard that holds the row", kw, dict(owner_rule="any")))
        if sh["n"] > 1:
            # (by one row the two-row halo would absorb it: that is what a halo is for)
            res.append(("rows_per_rank ignored: every row asked of shard 0", dict(kw, shards=dict(sh, rows_per_rank=kw["n_store"] + 1)), {}))
        res.append(("shard row0 + 1", dict(kw, shards=dict(sh, row0=[r + (n > 0) for r, n in zip(sh["row0"], sh["rows"])])), {}))
        if sh["row0"][-1] + sh["rows"][-1] == kw["n_store"]:   # (the last shard holds the last row of the store)
            res.append(("n_store - 1", dict(kw, n_store=kw["n_store"] - 1), {}))
    elif spec["win"] != "empty":
        if spec["win"] in ("win", "win_ns"):
            res += [(f"row0 {d:+d}", dict(kw, row0=kw["row0"] + d), {}) for d in (-1, 1)]
        if spec["win"] in ("win", "none"):
            res.append(("n_local - 1", dict(kw, n_local=kw["n_local"] - 1), {}))
        if spec["win"] in ("win_ns", "none"):
            res.append(("n_store - 1", dict(kw, n_store=kw["n_store"] - 1), {}))
    return res


# ======================================================================================================== pq_encode
U24 = 2.0 ** -24


def encode_ref(x, cen, norm2):
    """-> (dist, B) float64 [n, M, 256]: dist = norm2[m, c] - 2 x[r, m] . cen[m, c] without rounding (float64 products of float32
    values are exact, their sums good to 2^-53), and the bound on what a float32 evaluation

        dot = fmaf(x_e, c_e, dot)  (e = 0 .. dsub - 1),    dis = norm2 - 2 * dot

    may differ from it:  B = (dsub + 2) * 2^-24 * (|norm2| + 2 * sum_e |x_e| |c_e|).

    Derivation (u = 2^-24, A = sum_e |x_e| |c_e|; DERIVED, not measured): every fmaf rounds once, by at most u times the magnitude of its
    result, and every partial sum is at most A in magnitude, so the chain is off by at most dsub * u * A.  Doubling is exact.  The
    subtraction rounds once, by at most u * (|norm2| + 2 A).  Together u * (|norm2| + 2 A + 2 dsub A) <= (dsub + 1) * u * (|norm2| + 2 A);
    one more unit covers the second-order terms and a subtraction fused into a multiply-add.  x: [n, M * dsub]."""
    n = x.shape[0]
    M, _, dsub = cen.shape
    xs = x.reshape(n, M, dsub).astype(np.float64)
    c64 = cen.astype(np.float64)
    dist = norm2.astype(np.float64)[None] - 2.0 * np.einsum("nme,mce->nmc", xs, c64)
    B = (dsub + 2) * U24 * (np.abs(norm2.astype(np.float64))[None] + 2.0 * np.einsum("nme,mce->nmc", np.abs(xs), np.abs(c64)))
    return dist, B


def encode_emulate(x, cen, norm2):
    """float32 distances by the kernel's chain (each fmaf: the exact float64 product plus the float32 partial sum, rounded to float32)"""
    n = x.shape[0]
    M, _, dsub = cen.shape
    xs = x.reshape(n, M, dsub)
    dot = np.zeros((n, M, 256), dtype=np.float32)
    for e in range(dsub):
        dot = (xs[:, :, None, e].astype(np.float64) * cen[None, :, :, e].astype(np.float64) + dot.astype(np.float64)).astype(np.float32)
    return norm2[None] - np.float32(2) * dot


def encode_judge(codes, dist, B):
    """-> (worst excess of the chosen distance over the minimum in units of B[chosen] + B[argmin] (at most 2 B), share of entries decided
    exactly, number of decided entries whose code is not the float64 argmin).  A float32 distance lies within B of the float64 one, so the
    kernel's choice c satisfies dist[c] - B[c] <= min + B[argmin]; an entry is decided when no other centroid does: the runner-up is
    then more than the two bounds (2 B) above the minimum, and the kernel's code can only be the float64 argmin."""
    best = dist.argmin(-1)[:, :, None]
    top = np.take_along_axis(dist + B, best, -1)
    c = codes.astype(np.int64)[:, :, None]
    excess = float(((np.take_along_axis(dist, c, -1) - dist.min(-1, keepdims=True)) / (np.take_along_axis(B, c, -1) + np.take_along_axis(B, best, -1))).max())
    low = dist - B
    np.put_along_axis(low, best, np.inf, -1)
    decided = low.min(-1) > top[:, :, 0]
    return excess, float(decided.mean()), int((decided & (codes != best[:, :, 0])).sum())


ENCODE_SHAPES = [(1, 4), (6, 1), (6, 8), (128, 8), (5, 12)]
ENCODE_N = [1, 3, 4, 5, 257]
ENCODE_CASES = [dict(M=M, dsub=d, n=n, pad=pad) for M, d in ENCODE_SHAPES for n in ENCODE_N for pad in (0, 4)]
# index sets of bit-identical centroids: same lane at all four t; adjacent lanes; across the xor-32 step; lane 63 / lane 0 of the next
# t; the two ends; a set whose lowest member is neither the first listed nor alone in its lane
TIE_SETS = [(7, 71, 135, 199), (7, 8), (7, 39), (63, 64), (0, 255), (200, 7, 71)]
TIE_CASES = [dict(M=M, dsub=d, n=n, pad=pad, dup=dup) for dup in TIE_SETS for M, d, n, pad in [(6, 8, 5, 0), (5, 12, 3, 4), (6, 1, 4, 0)]]


def encode_case_id(c):
    return f"M{c['M']}x{c['dsub']}-n{c['n']}-ld+{c['pad']}" + ("-dup" + "_".join(map(str, c["dup"])) if "dup" in c else "")


def make_encode_case(c):
    """-> dict(x [n, ldx] float32 (pad columns NaN: they are not part of the rows), cen, norm2, M, dsub, n, ldx, want = the exact code
    matrix of a tie case or None)"""
    M, dsub, n = c["M"], c["dsub"], c["n"]
    rs = _rs(sorted(c.items()))
    D = M * dsub
    cen = rs.randn(M, 256, dsub).astype(np.float32)
    x = np.full((n, D + c["pad"]), np.nan, dtype=np.float32)
    want = None
    if "dup" in c:
        dup = list(c["dup"])
        v = cen[:, dup[:1]].astype(np.float64)               # bit-identical rows, 1.5 x as far out as any other, so that nothing else comes near
        far = 1.5 * np.sqrt((cen.astype(np.float64) ** 2).sum(-1)).max(-1)
        cen[:, dup] = (v / np.sqrt((v ** 2).sum(-1, keepdims=True)) * far[:, None, None]).astype(np.float32)
        x[:, :D] = (cen[:, dup[0]].reshape(1, D) * (1 + 0.01 * rs.randn(n, D))).astype(np.float32)
        want = np.full((n, M), min(dup), dtype=np.uint8)
    else:
        x[:, :D] = rs.randn(n, D)
    norm2 = (cen.astype(np.float64) ** 2).sum(-1).astype(np.float32)
    if "dup" in c:
        norm2[:, dup] = norm2[:, dup[:1]]                     # computed once and copied
    return dict(x=x, cen=cen, norm2=norm2, M=M, dsub=dsub, n=n, ldx=D + c["pad"], want=want)


@functools.lru_cache(maxsize=None)
def encode_shape_share(M, dsub):
    """share of the entries of a shape's random cases (every n, both row strides) that are decided exactly: a property of the inputs
    alone.  A case of a few entries cannot be held to 95 % on its own (one near-tie in 18 is 5.6 %); the shape is."""
    decided = total = 0
    for c in ENCODE_CASES:
        if (c["M"], c["dsub"]) == (M, dsub):
            k = make_encode_case(c)
            dist, B = encode_ref(k["x"][:, :M * dsub], k["cen"], k["norm2"])
            share = encode_judge(dist.argmin(-1), dist, B)[1]
            decided, total = decided + share * c["n"] * M, total + c["n"] * M
    return decided / total


def tie_winner(dup, in_lane="first", cross="index"):
    """code the kernel's two-stage argmin gives when exactly the centroids ``dup`` share the smallest distance: every lane scans
    c = lane + 64 t and keeps the first (or, wrongly, the last) minimum, then a xor butterfly (32 .. 1) merges the lanes, on a tie
    by the lower index (or, wrongly: keeping its own, or taking the other's); lane 0 stores."""
    dist = np.ones(256)
    dist[list(dup)] = 0.0
    best, bi = np.full(64, np.inf), np.zeros(64, dtype=np.int64)
    for t in range(4):
        cidx = np.arange(64) + 64 * t
        take = dist[cidx] < best if in_lane == "first" else dist[cidx] <= best
        best, bi = np.where(take, dist[cidx], best), np.where(take, cidx, bi)
    for o in (32, 16, 8, 4, 2, 1):
        ob, oi = best[np.arange(64) ^ o], bi[np.arange(64) ^ o]
        tie = {"index": oi < bi, "keep": np.zeros(64, dtype=bool), "take": np.ones(64, dtype=bool)}[cross]
        take = (ob < best) | ((ob == best) & tie)
        best, bi = np.where(take, ob, best), np.where(take, oi, bi)
    return int(bi[0])


# ======================================================================================================== gather_rows_peer
def peer_ref(kw, owner_rule="owner"):
    """-> (out uint8 [n, row_bytes], valid uint8 [n]): row r comes from its OWNER min(world - 1, r / rows_per_rank) if that shard holds
    it; rows outside [0, n_store) and rows the owner does not hold are zero rows with valid 0."""
    rows = np.asarray(kw["rows"], dtype=np.int64)[:kw["n"]]
    ok = (rows >= 0) & (rows < kw["n_store"])
    g, loc, ok = shard_lookup(kw["shards"], rows, ok, owner_rule)
    return shard_rows(kw["shards"], g, loc, ok, kw["row_bytes"]), ok.astype(np.uint8)


PEER_ROW_BYTES = [1, 2, 4, 12, 16, 48, 128]
PEER_CASES = [("bytes" if rb < 16 else f"lanes<{rb // 16}>", dict(row_bytes=rb, world=w, variant=v, out_valid=(n + m) % 2 == 0))
              for n, rb in enumerate(PEER_ROW_BYTES) for m, (w, v) in enumerate([(1, "full"), (1, "hole"), (3, "full"), (3, "hole"), (3, "empty"),
                                                                                  (16, "full"), (16, "empty")])]


def peer_case_id(case):
    route, s = case
    return f"{route}-rb{s['row_bytes']}-w{s['world']}-{s['variant']}" + ("-valid" if s["out_valid"] else "")


def peer_route(row_bytes):
    return "bytes" if row_bytes < 16 else f"lanes<{row_bytes // 16}>"


def make_peer_case(route, spec):
    rb, world = spec["row_bytes"], spec["world"]
    rs = _rs(route, sorted(spec.items()))
    n_store, n = N_STORE + 1, 301
    per = {1: 600, 3: 300, 16: 60}[world]
    table = rs.randint(0, 256, size=(n_store, rb)).astype(np.uint8)
    rows = rs.randint(0, n_store, size=n).astype(np.int64)
    edges = [-1, 0, n_store - 1, n_store, FAR_ID, -7] + halo_ids(world, per, n_store)
    rows[rs.choice(n, size=len(edges), replace=False)] = edges
    kw = dict(shards=make_shards(table, world, per, spec["variant"]), world=world, row_bytes=rb, rows_per_rank=per, n_store=n_store,
              rows=rows, n=n, out_valid=spec["out_valid"])
    return dict(route=route, spec=spec, kw=kw)
