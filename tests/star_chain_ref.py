"""float64 restatement of gnnlm_star_attn / gnnlm_chain_attn driven by the DESCRIPTOR fields (include/gnnlm.h: gnnlm_star_attn_t,
gnnlm_chain_attn_t), and the case tables of tests/test_star_chain_abi_gpu.py.  Plain numpy; nothing here imports gnnlm_amd, and
the rules are the header's comments, not the kernels.

star_ref / chain_ref take the descriptor's fields as arrays.  A buffer is the array that starts at the pointer the kernel is handed
(``codes`` of a store window is the table from row ``row0`` on), ``X`` is flat and addressed through ``ldx`` as the kernel does.
The references never read what the rule excludes: excluded rows may hold NaN.

Inputs of the GPU cases (make_star_case / make_chain_case).  Every neighbour gets ONE reason to be invalid (or none), so each
validity rule has neighbours that only it excludes.  Whatever a rule excludes, and every row or table entry no valid neighbour
owns, points at an in-bounds poison row (PQ: code 255 of every sub-quantizer, a centroid scaled by 1e4; dense: a row of 1e4), and
the buffers are long enough for the identity table and the unit stride, so a kernel that ignored a field would read inside its
buffers and miss the bar by orders of magnitude.  tests/test_star_chain_ref_cpu.py asserts that this holds for every case."""
import zlib

import numpy as np

TOL = 2e-5                  # the bar of test_star_attn_pq / test_star_attn_dense / test_chain_attn
POISON = 1e4
POISON_CODE = 255
N_IDS = 3000                # neighbour ids are drawn from [0, N_IDS)
ROW0, N_LOCAL = 512, 2000   # the store window of the cases that have one: rows [512, 2512)
N_STORE = 2200              # the store bound of the cases that have one (inside the window)
SLACK_GROUPS = 5            # chain buffers hold this many groups more than n_groups (valid, finite data, sentinel output)


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _softmax_last(s):
    with np.errstate(invalid="ignore"):
        a = np.exp(s - s.max(-1, keepdims=True))
        return np.nan_to_num(a / a.sum(-1, keepdims=True))


# ======================================================================================================== star attention
def star_rules(ids, *, codes=None, row0=0, n_local=0, codes_direct=0, n_store=0, nb_valid=None, nb_valid_stride=0, x_index=None, **_):
    """{rule: bool [T, kg]} -- neighbour (i, j) takes part iff every rule holds.  A rule is vacuously true where an earlier one
    already leaves it without a subject (no row for a negative id, no validity byte for group -1), so the neighbours a rule
    ALONE excludes can be counted."""
    T, kg = ids.shape
    e = np.arange(T * kg, dtype=np.int64).reshape(T, kg)
    g = e if x_index is None else np.asarray(x_index, dtype=np.int64)[:T * kg].reshape(T, kg)
    rules = {"ids>=0": ids >= 0}
    if n_store > 0:
        rules["ids<n_store"] = ids < n_store
    if codes is not None and codes_direct == 0:
        rules["window"] = (ids < 0) | ((ids >= row0) & (ids < row0 + n_local))
    if x_index is not None:
        rules["x_index>=0"] = g >= 0
    if nb_valid is not None:
        rules["nb_valid"] = (g < 0) | (np.asarray(nb_valid)[np.where(g >= 0, g, 0) * nb_valid_stride] != 0)
    return rules


def star_ref(U, ids, *, codes=None, row0=0, n_local=0, M=0, dsub=0, codes_direct=0, centroids=None, X=None, ldx=0, x_group_stride=0,
             codes_index=None, n_store=0, nb_valid=None, nb_valid_stride=0, x_index=None):
    """-> (Z [T, H, D] float64, has_nb [T] float32).  codes: uint8 [rows, M] from the descriptor's pointer on; X: flat float array."""
    assert (codes is None) != (X is None)
    T, H, D = U.shape
    kg = ids.shape[1]
    rules = star_rules(ids, codes=codes, row0=row0, n_local=n_local, codes_direct=codes_direct, n_store=n_store, nb_valid=nb_valid,
                       nb_valid_stride=nb_valid_stride, x_index=x_index)
    ok = np.logical_and.reduce(list(rules.values()))
    e = np.arange(T * kg, dtype=np.int64).reshape(T, kg)
    g = e if x_index is None else np.asarray(x_index, dtype=np.int64)[:T * kg].reshape(T, kg)
    if codes is not None:
        assert M * dsub == D
        if codes_direct == 0:
            row = ids - row0
        else:
            row = e * codes_direct
            if codes_index is not None:
                row = np.asarray(codes_index, dtype=np.int64)[row]
        c = codes[np.where(ok, row, 0)].astype(np.int64)                                   # [T, kg, M]
        x = centroids.astype(np.float64)[np.arange(M)[None, None, :], c].reshape(T, kg, D)
    else:
        row = np.where(ok, g * x_group_stride, 0)
        x = np.asarray(X)[(row * ldx)[:, :, None] + np.arange(D)[None, None, :]].astype(np.float64)
    x = np.where(ok[:, :, None], x, 0.0)
    s = np.where(ok[:, None, :], np.einsum("tjd,thd->thj", x, U.astype(np.float64)), -np.inf)
    Z = np.einsum("thj,tjd->thd", _softmax_last(s), x)
    return Z, ok.any(1).astype(np.float32)


# option sets: window / n_store bound in force, nb_valid stride (0: none), x_index, codes_direct (0: the store), codes_index,
# x_group_stride (dense)
PQ_OPTIONS = {
    "a-window":            dict(window=True, n_store=True),
    "b-no-n_store":        dict(window=True),
    "c-nb_valid-s1":       dict(window=True, nbv=1),
    "c-nb_valid-s3":       dict(window=True, nbv=3),
    "d-x_index-nb_valid":  dict(window=True, nbv=3, xidx=True),
    "e-direct-1":          dict(cd=1, n_store=True),
    "e-direct-3":          dict(cd=3, n_store=True),
    "f-direct-1-index":    dict(cd=1, cidx=True, n_store=True),
    "f-direct-3-index":    dict(cd=3, cidx=True, n_store=True),
    "g-dedup-1":           dict(cd=1, cidx=True, n_store=True, nbv=1, xidx=True),
    "g-dedup-3":           dict(cd=3, cidx=True, n_store=True, nbv=3, xidx=True),
}
DENSE_OPTIONS = {
    "h-stride-1":          dict(xgs=1),
    "h-stride-3":          dict(xgs=3),
    "i-x_index":           dict(xgs=3, xidx=True),
    "j-x_index-nbv-s1":    dict(xgs=2, xidx=True, nbv=1),
    "j-x_index-nbv-s3":    dict(xgs=2, xidx=True, nbv=3),
    "k-n_store":           dict(xgs=1, n_store=True),
}

# (route, shape): the route is what star_route() -- the dispatch of star_attn restated -- gives for the shape, asserted on the CPU
STAR_PQ_SHAPES = [
    ("tab<8,128>",          dict(T=5, H=8, M=128, dsub=8, kg=128)),     # T no multiple of the 4 tokens of a workgroup
    ("tab<8,128>",          dict(T=5, H=8, M=128, dsub=8, kg=33)),
    ("tab<8,0>",            dict(T=1, H=12, M=16, dsub=8, kg=70)),      # two head passes
    ("tab<8,0>",            dict(T=6, H=12, M=16, dsub=8, kg=70)),
    ("tab<4,0>",            dict(T=5, H=3, M=16, dsub=4, kg=4)),
    ("tab<4,0>",            dict(T=5, H=3, M=16, dsub=4, kg=128)),
    ("generic<1>,staged",   dict(T=3, H=8, M=16, dsub=8, kg=130)),      # k_g > 128
    ("generic<1>,staged",   dict(T=4, H=8, M=8, dsub=16, kg=21)),       # M % 16 != 0: byte-wise staging
    ("generic<2>,staged",   dict(T=3, H=5, M=32, dsub=16, kg=19)),
    ("generic<4>,staged",   dict(T=3, H=8, M=64, dsub=16, kg=40)),
    ("generic<4>,staged",   dict(T=3, H=8, M=144, dsub=4, kg=40)),      # a tab shape but for its LDS: 91136 + 512 M > 160 KiB
    ("generic<4>,unstaged", dict(T=2, H=8, M=64, dsub=16, kg=330)),     # base + code LDS = 44656 + 21120 > 65536
]
STAR_DENSE_SHAPES = [
    ("dense<1>",            dict(T=5, H=8, D=256, kg=9)),
    ("dense<2>",            dict(T=4, H=5, D=512, kg=37)),
    ("dense<4>",            dict(T=3, H=8, D=1024, kg=128)),
    ("dense<1>",            dict(T=3, H=5, D=256, kg=128)),
    ("generic<1>,dense",    dict(T=6, H=8, D=64, kg=10)),
    ("generic<4>,dense",    dict(T=2, H=12, D=1024, kg=16)),            # H > 8
    ("generic<4>,dense",    dict(T=3, H=8, D=768, kg=21)),              # D not one of 256 / 512 / 1024
]
STAR_CASES = [(r, s, o) for r, s in STAR_PQ_SHAPES for o in PQ_OPTIONS] + [(r, s, o) for r, s in STAR_DENSE_SHAPES for o in DENSE_OPTIONS]


def star_case_id(case):
    route, s, opt = case
    return f"{route}-T{s['T']}-H{s['H']}-" + (f"M{s['M']}x{s['dsub']}" if "M" in s else f"D{s['D']}") + f"-kg{s['kg']}-{opt}"


def star_route(T, H, kg, M=0, dsub=0, D=0, **_):
    """The kernel star_attn (star_attn.hip) takes for a shape: star_route() of csrc/star_route.h restated (the tab and dense
    conditions, the LDS formulas and the QPL choice), for 16-byte aligned buffers and ldx % 4 == 0 -- star_attn refuses others --
    with the A/B switch unset.  tests/test_star_chain_ref_cpu.py compares it with star_route() itself."""
    pq = M > 0
    D = M * dsub if pq else D
    if pq and kg <= 128 and dsub in (4, 8) and M % 16 == 0 and D % 32 == 0 and \
            2 * 32 * 256 * 4 + 4 * 8 * 132 * 4 + 2 * 4 * 1024 + 4 * 128 + 4 * 128 * M <= 160 * 1024:
        return "tab<8,128>" if (dsub, M) == (8, 128) else f"tab<{dsub},0>"
    if not pq and H <= 8 and D in (256, 512, 1024) and (8 * D + 4 * 8 * 2) * 4 + kg * 8 <= 64 * 1024:
        return f"dense<{D // 256}>"
    qpl = 1 if D // 4 <= 64 else 2 if D // 4 <= 128 else 4
    if not pq:
        return f"generic<{qpl}>,dense"
    base = (8 * kg + 8 * D + ((kg + 3) & ~3)) * 4
    return f"generic<{qpl}>," + ("staged" if base + ((kg * M + 15) & ~15) <= 64 * 1024 else "unstaged")


def make_star_case(route, shape, opt):
    """-> dict(kw = the keyword arguments of star_ref (the descriptor's fields), U, ids, code_buf / code_off (the whole code buffer and
    the row at which the descriptor's pointer starts), reason [T, kg] (why a neighbour is invalid, "" if it is not), T, H, D, kg)."""
    T, H, kg = shape["T"], shape["H"], shape["kg"]
    pq = "M" in shape
    M, dsub = (shape["M"], shape["dsub"]) if pq else (0, 0)
    D = M * dsub if pq else shape["D"]
    O = dict(window=False, n_store=False, nbv=0, xidx=False, cd=0, cidx=False, xgs=1)
    O.update((PQ_OPTIONS if pq else DENSE_OPTIONS)[opt])
    rs = _rs(route, sorted(shape.items()), opt)
    n = T * kg
    U = (rs.randn(T, H, D) / np.sqrt(D)).astype(np.float32)

    # ---- one reason per neighbour.  Token 1 (when there is one) has no valid neighbour; the first neighbours of the tokens behind it
    # carry every reason once (with the id on the edge of its rule: n_store, row0 - 1, row0 + n_local), the first and the last valid neighbour
    # have the lowest and the highest valid id, the rest is invalid with probability 0.25
    reasons = ["neg"] + (["n_store"] if O["n_store"] else []) + (["below", "above"] if O["window"] else []) + \
              (["x_index"] if O["xidx"] else []) + (["nb_valid"] if O["nbv"] else [])
    reason = np.where(rs.rand(n) < 0.25, rs.choice(reasons, size=n), "").astype(object).reshape(T, kg)
    none_tok = 1 if T > 1 else None
    if none_tok is not None:
        reason[none_tok] = [reasons[j % len(reasons)] for j in range(kg)]
    free = [(i, j) for j in range(kg) for i in range(T) if i != none_tok]              # (column-major: spread over the tokens)
    reason[free[0]] = ""
    forced = dict(zip(reasons, free[1:]))
    for r, pos in forced.items():
        reason[pos] = r
    reason = reason.astype(str)

    # ---- ids
    lo = ROW0 if O["window"] else 0
    hi = min(ROW0 + N_LOCAL if O["window"] else N_IDS, N_STORE if O["n_store"] else N_IDS)
    ids = rs.randint(lo, hi, size=(T, kg)).astype(np.int64)
    if O["xidx"]:                                           # neighbours come in groups of one centre row each
        G = max(4, n // 3)
        bad = np.zeros(G, dtype=bool)
        bad[rs.choice(G, size=max(1, G // 4), replace=False)] = O["nbv"] > 0
        gid = rs.choice(np.arange(lo, hi), size=G, replace=False).astype(np.int64)
        group = np.where(reason == "nb_valid", rs.choice(np.nonzero(bad)[0] if bad.any() else [0], size=(T, kg)),
                         rs.choice(np.nonzero(~bad)[0], size=(T, kg))).astype(np.int64)
        ids = gid[group]
        x_index = np.where(reason == "x_index", -1, group).astype(np.int32).reshape(-1)
    ids[reason == "neg"] = -1
    top = ROW0 + N_LOCAL if O["window"] else N_IDS
    ids[reason == "n_store"] = rs.randint(N_STORE, top, size=(T, kg))[reason == "n_store"]
    ids[reason == "below"] = rs.randint(0, ROW0, size=(T, kg))[reason == "below"]
    ids[reason == "above"] = rs.randint(ROW0 + N_LOCAL, N_IDS, size=(T, kg))[reason == "above"]
    for r, edge in (("n_store", N_STORE), ("below", ROW0 - 1), ("above", ROW0 + N_LOCAL)):
        if r in forced:
            ids[forced[r]] = edge
    valid = reason == ""
    if not O["xidx"]:
        ids[free[0]] = lo
        ids[tuple(np.argwhere(valid)[-1])] = hi - 1
    e = np.arange(n).reshape(T, kg)
    g = np.where(x_index.reshape(T, kg) >= 0, x_index.reshape(T, kg), 0) if O["xidx"] else e

    kw = dict(n_store=N_STORE if O["n_store"] else 0)
    out = dict(route=route, opt=opt, T=T, H=H, D=D, kg=kg, U=U, ids=ids, reason=reason, kw=kw, code_off=0)
    if O["xidx"]:
        kw["x_index"] = x_index
    if O["nbv"]:
        st = O["nbv"]
        nbv = rs.randint(0, 2, size=n * st + 1).astype(np.uint8)                       # off-stride bytes, unused groups: anything
        nbv[np.arange(n) * st] = rs.choice([1, 2, 255], size=n)
        if O["xidx"]:
            nbv[np.nonzero(bad)[0] * st] = 0
        else:
            nbv[e[reason == "nb_valid"] * st] = 0
        # where a unit stride would look for group k's byte (k no multiple of the stride) stands the opposite of that byte
        good = ~bad if O["xidx"] else reason.reshape(-1) != "nb_valid"
        k = np.arange(len(good))[np.arange(len(good)) % st != 0]
        nbv[k] = np.where(good[k], 0, 1)
        kw.update(nb_valid=nbv, nb_valid_stride=st)

    if pq:
        cen = (0.5 * rs.randn(M, 256, dsub)).astype(np.float32)
        cen[:, POISON_CODE] *= POISON
        kw.update(M=M, dsub=dsub, centroids=cen, codes_direct=O["cd"])
        if O["cd"] == 0:
            # the whole table of ids [0, N_IDS) and ROW0 poison rows behind it (so that row0 read as 0 stays inside); the rows a valid id
            # can name are real, every other one is poison.  The descriptor's pointer starts at row row0.
            buf = np.full((N_IDS + ROW0 + 1, M), POISON_CODE, dtype=np.uint8)
            buf[lo:hi] = rs.randint(0, POISON_CODE, size=(hi - lo, M))
            out.update(code_buf=buf, code_off=lo)
            kw.update(codes=buf[lo:], row0=lo, n_local=N_LOCAL if O["window"] else N_IDS)
        else:
            cd = O["cd"]
            if not O["cidx"]:                                                          # slot (i, j) at row (i * kg + j) * cd
                buf = np.full((n * cd + 1, M), POISON_CODE, dtype=np.uint8)
                buf[e[valid] * cd] = rs.randint(0, POISON_CODE, size=(int(valid.sum()), M))
            else:
                # R real rows scattered over a buffer long enough for the identity table, poison everywhere else; the table sends a valid
                # neighbour (with x_index: its group) to a real row, many to one, and every other entry to a poison row
                R = max(2, (G if O["xidx"] else n) // 2)
                rows = n * cd + 2
                buf = np.full((rows, M), POISON_CODE, dtype=np.uint8)
                real = rs.choice(rows, size=R, replace=False)
                buf[real] = rs.randint(0, POISON_CODE, size=(R, M))
                poison_rows = np.setdiff1d(np.arange(rows), real)
                table = rs.choice(poison_rows, size=n * cd + 1).astype(np.int32)
                own = rs.choice(real, size=G)[g] if O["xidx"] else rs.choice(real, size=(T, kg))
                table[e[valid] * cd] = own[valid]
                kw["codes_index"] = table
            out.update(code_buf=buf)
            kw["codes"] = buf
    else:
        xgs, ldx = O["xgs"], D + 4
        X = np.full((n * xgs + 1, ldx), POISON, dtype=np.float32)
        own = np.unique(g[valid])
        X[own * xgs, :D] = rs.randn(len(own), D)
        kw.update(X=X.reshape(-1), ldx=ldx, x_group_stride=xgs)
    return out


def star_neutralised(case):
    """[(what, keyword arguments of star_ref with that one field neutralised)] for every field the case sets."""
    kw, n, res = case["kw"], case["T"] * case["kg"], []
    if kw.get("codes_direct", 0) > 1:
        res.append(("codes_direct -> 1", dict(kw, codes_direct=1)))
    if kw.get("codes_index") is not None:
        res.append(("codes_index -> identity", dict(kw, codes_index=np.arange(len(kw["codes_index"]), dtype=np.int32))))
    if kw.get("nb_valid") is not None:
        res.append(("nb_valid ignored", dict(kw, nb_valid=None)))
        if kw["nb_valid_stride"] > 1:
            res.append(("nb_valid_stride -> 1", dict(kw, nb_valid_stride=1)))
    if kw.get("x_index") is not None:
        res.append(("x_index -> identity", dict(kw, x_index=np.arange(n, dtype=np.int32))))
    if kw.get("x_group_stride", 0) > 1:
        res.append(("x_group_stride -> 1", dict(kw, x_group_stride=1)))
    if kw.get("X") is not None:
        res.append(("ldx -> D", dict(kw, ldx=case["D"])))
    if kw.get("row0", 0) > 0:
        res.append(("row0 -> 0", dict(kw, row0=0)))
    if kw["n_store"] > 0:
        res.append(("n_store bound removed", dict(kw, n_store=0)))
    return res


# ======================================================================================================== chain attention
def chain_slot(pos, left):
    """slot inside its group of the node at path position pos (order o-l .. o-1, o, o+1 .. o+r; slot 0 is the centre)."""
    return pos + 1 if pos < left else (0 if pos == left else pos)


def chain_ref(Q, K, V, valid, *, n_groups, left, right, H, dk, scale=None, radius_p1=0, n_groups_dev=None, kv_index=None):
    """-> (out [n_slots, H * dk] float64, write mask [n_slots] bool); n_slots = the rows of Q (>= n_groups * n_g).  Q, K, V: 2-D arrays of
    which the first H * dk columns are read.  A row outside the mask must stay as it was; an invalid destination slot is a zero row."""
    n_g = 1 + left + right
    d = H * dk
    n_slots = Q.shape[0]
    cnt = n_groups if n_groups_dev is None else max(0, min(n_groups, int(n_groups_dev)))
    base = np.arange(cnt, dtype=np.int64) * n_g
    valid = np.asarray(valid) != 0
    sc = np.ones(H) if scale is None else np.asarray(scale, dtype=np.float64)
    out, mask = np.zeros((n_slots, d)), np.zeros(n_slots, dtype=bool)

    def kv_rows(K_or_V, s, ok):
        row = s if kv_index is None else np.asarray(kv_index, dtype=np.int64)[s]
        x = K_or_V[np.where(ok, row, 0), :d].astype(np.float64)
        return np.where(ok[:, None], x, 0.0).reshape(cnt, H, dk)

    for pos in range(n_g):
        if radius_p1 > 0 and abs(pos - left) > radius_p1 - 1:
            continue
        s = base + chain_slot(pos, left)
        mask[s] = True
        q = np.where(valid[s][:, None], Q[s, :d].astype(np.float64), 0.0).reshape(cnt, H, dk)
        scores, vals = [], []
        for u in (pos - 1, pos, pos + 1):
            if 0 <= u < n_g:
                su = base + chain_slot(u, left)
                ok = valid[s] & valid[su]                   # an edge needs both ends: a hole breaks the path
                scores.append(np.where(ok[:, None], np.einsum("ghe,ghe->gh", q, kv_rows(K, su, ok)) * sc[None, :], -np.inf))
                vals.append(kv_rows(V, su, ok))
        a = _softmax_last(np.stack(scores, -1))             # [cnt, H, edges]
        out[s] = np.einsum("ghu,ughe->ghe", a, np.stack(vals)).reshape(cnt, d)
    return out, mask


CHAIN_SHAPES = [(0, 0), (2, 2), (4, 3), (0, 7), (3, 1)]
CHAIN_WIDTHS = [(4, 1), (4, 8), (64, 1), (64, 8), (100, 1), (100, 8), (256, 1), (256, 8)]       # (dk, H)


def _chain_cases():
    cases = []
    for n, (l, r) in enumerate(CHAIN_SHAPES):               # every shape x every head width; scale given / NULL alternates
        for m, (dk, H) in enumerate(CHAIN_WIDTHS):
            cases.append(dict(left=l, right=r, dk=dk, H=H, scale=(n + m) % 2 == 0))
    for l, r in [(4, 3), (0, 7)]:                            # n_g = 8: every radius, slot-indexed and row-keyed K / V
        for rad in (0, 1, 2, 3):
            for kv in (False, True):
                cases.append(dict(left=l, right=r, dk=100, H=8, scale=kv, radius_p1=rad, kv=kv))
    for l, r in [(2, 2), (3, 1)]:
        for rad in (1, 2):
            cases.append(dict(left=l, right=r, dk=64, H=8, scale=True, radius_p1=rad))
    for l, r in [(0, 0), (2, 2), (3, 1)]:
        cases.append(dict(left=l, right=r, dk=64, H=1, scale=False, kv=True))
    for ngd in ("0", "1", "G-1", "G", "G+5"):
        cases.append(dict(left=2, right=2, dk=64, H=8, scale=True, ngd=ngd))
    cases.append(dict(left=4, right=3, dk=100, H=8, scale=True, radius_p1=2, kv=True, ngd="G-1"))
    # n_groups * H = 40000 > 32768 = 4 tasks x the 8192 workgroups a device-side count caps the grid at: the waves walk
    cases.append(dict(left=1, right=1, dk=4, H=8, scale=True, ngd="G", G=5000))
    cases.append(dict(left=1, right=1, dk=4, H=8, scale=False, ngd="G+5", G=5000, kv=True))
    return cases


CHAIN_CASES = _chain_cases()


def chain_case_id(c):
    return f"l{c['left']}r{c['right']}-dk{c['dk']}-H{c['H']}-G{c.get('G', 7)}" + ("-scale" if c["scale"] else "") + \
        (f"-rad{c['radius_p1']}" if "radius_p1" in c else "") + ("-kv" if c.get("kv") else "") + (f"-ngd{c['ngd']}" if "ngd" in c else "")


def make_chain_case(c):
    """-> dict(Q, K, V [rows, ld] float32, valid uint8 [n_slots], kw = the other arguments of chain_ref, ld, ldo, n_slots); n_slots covers
    n_groups + SLACK_GROUPS groups.  Validity: group 0 and the last group partly invalid, group 2 wholly, holes in the middle of the
    others (30 % of the slots).  With radius_p1 = r + 1 the rows of Q outside the destinations and the rows of K / V more than r + 1
    from the centre are NaN; with kv_index K / V have rows of their own (fewer than slots, shared), -1 for an invalid slot, NaN in row
    0 (named by nobody) and in the last row (named by the slots the radius leaves out)."""
    l, r, dk, H = c["left"], c["right"], c["dk"], c["H"]
    G, n_g, d = c.get("G", 7), 1 + l + r, H * dk
    rad, kv = c.get("radius_p1", 0), c.get("kv", False)
    rs = _rs(sorted(c.items()))
    n_slots = (G + SLACK_GROUPS) * n_g
    ld, ldo = d + 4, d + 8
    valid = (rs.rand(G + SLACK_GROUPS, n_g) >= 0.3)
    valid[G:] = True
    valid[2] = False
    pos_slot = [chain_slot(p, l) for p in range(n_g)]
    if n_g > 1:
        valid[0, pos_slot[0]], valid[0, pos_slot[-1]], valid[0, pos_slot[n_g // 2]] = False, True, True
        valid[G - 1, pos_slot[-1]], valid[G - 1, pos_slot[0]] = False, True
        valid[1] = True
        valid[1, pos_slot[n_g // 2]] = n_g < 3                                         # a hole in the middle of a group
        valid[3] = True                                                                # a whole group
    else:
        valid[[0, 1, 3], 0] = [True, False, True]
    valid = valid.reshape(-1)
    dist = np.tile(np.array([abs(p - l) for p in range(n_g)])[np.argsort(pos_slot)], G + SLACK_GROUPS)   # per slot
    Q = rs.randn(n_slots, ld).astype(np.float32)
    n_kv = max(3, n_slots // 2) + 2 if kv else n_slots
    K, V = rs.randn(n_kv, ld).astype(np.float32), rs.randn(n_kv, ld).astype(np.float32)
    kw = dict(n_groups=G, left=l, right=r, H=H, dk=dk, radius_p1=rad)
    if c["scale"]:
        kw["scale"] = (1 + 0.3 * rs.randn(H)).astype(np.float32)
    if rad > 0:
        Q[dist > rad - 1] = np.nan
    if kv:
        index = rs.randint(1, n_kv - 1, size=n_slots).astype(np.int32)
        index[valid == 0] = -1
        K[0] = V[0] = K[-1] = V[-1] = np.nan
        if rad > 0:
            index[(dist > rad) & (valid != 0)] = n_kv - 1
        kw["kv_index"] = index
    elif rad > 0:
        K[dist > rad] = np.nan
        V[dist > rad] = np.nan
    if "ngd" in c:
        kw["n_groups_dev"] = {"0": 0, "1": 1, "G-1": G - 1, "G": G, "G+5": G + 5}[c["ngd"]]
    return dict(Q=Q, K=K, V=V, valid=valid.astype(np.uint8), kw=kw, ld=ld, ldo=ldo, n_slots=n_slots, G=G, n_g=n_g)


def chain_neutralised(case):
    """[(what, keyword arguments of chain_ref, K, V)] with one field neutralised; K / V are repeated up to the slot count where the
    slots index them directly.  The count is min(n_groups, *n_groups_dev): a device count above n_groups moves nothing by +- 1, there
    the neutralised field is the clamp (the slack groups make it visible in bounds)."""
    kw, res = case["kw"], []
    K, V = case["K"], case["V"]
    rad = kw["radius_p1"]
    if rad > 0:
        res += [(f"radius_p1 -> {r2}", dict(kw, radius_p1=r2), K, V) for r2 in (rad - 1, rad + 1)]
    if "kv_index" in kw:
        rep = -(-case["n_slots"] // len(K))
        res.append(("kv_index ignored", dict(kw, kv_index=None), np.tile(K, (rep, 1)), np.tile(V, (rep, 1))))
    if "n_groups_dev" in kw:
        ngd, G = kw["n_groups_dev"], kw["n_groups"]
        if ngd > G:
            res.append(("n_groups ignored", dict(kw, n_groups=ngd), K, V))
        else:
            res += [(f"n_groups_dev -> {m}", dict(kw, n_groups_dev=m), K, V) for m in (ngd - 1, ngd + 1) if 0 <= m <= G]
    return res
