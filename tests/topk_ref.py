"""gnnlm_topk_merge (include/gnnlm.h: gnnlm_topk_t) restated in numpy, and the case tables of tests/test_topk_abi_gpu.py.

The contract is exact, so the reference is a sort and every comparison against it is bit for bit:

    value(r, c) = fl(fl(fl(scores[r, c] * alpha) * col_scale[c]) + col_bias[c])       float32, rounded after each step; alpha 0 -> 1
    id(r, c)    = ids[r, c], else col_ids[c], else col0 + c
    valid(r, c) = c < min(ncols, row_ncols[r])  and  id >= 0  and  value is neither NaN nor the worst infinity of the direction
    fold        = the state's real entries (id >= 0) and the chunk's valid entries, sorted by (better value, ascending id), the
                  first k, padded with id -1 and -inf (largest) / +inf

A "call" is a dict with the descriptor's fields as numpy arrays (``scores`` [n, ncols] without padding; the GPU test lays it out with
a row stride of its own).  ``make_case(spec)`` builds one deterministically from a spec of the tables below; ``split`` cuts a column
range out of it; ``route`` names the kernel the dispatcher of csrc/topk.hip launches for it.

Rows.  Every case holds one row per pattern (ROW_PATTERNS; with per-row ids the six id-digit rows take the place of two of them).
The patterns are laid out in VALUE space and carried back through the case's transform, so a tie that is meant is a tie after
the transform: exactly for the transforms "none" and "dyadic" (alpha in {0, 1, -2}, scales +-2^j, biases multiples of 1/4, values
multiples of 1/64: every step of the inversion and of value() is exact), approximately for "general" (alpha 0.7, arbitrary scales and
biases of period 32: what pins the rounding after each step -- a fused multiply-add gives other bits -- and still ties within a
column class).  The reference never looks at the layout: it computes value() from the scores like the kernel."""
import os

import numpy as np

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPK_SOURCE = os.path.join(ROOT, "gnn-lm_amd", "csrc", "topk.hip")

# the dispatch of topk_merge() (csrc/topk.hip); test_topk_ref_cpu.py parses the source and compares
SELECT_MAX_NCOLS = 16384            # init = 1 and ncols <= this: the select kernel
SELECT_REG_NCOLS = 4096             # ncols <= this: EPT = 16 (the whole row in registers), else EPT = 20 (5120 columns in registers)
SELECT_KP = (64, 256, 1024, 2048)
MERGE_KP = (512, 1024, 2048)
MERGE_K = (256, 1024, 2048)         # k <= MERGE_K[i]: merge<MERGE_KP[i]> (KP = 512 for small k: two sub-blocks of 256 columns per sort)
PRESEL = 2                          # GNNLM_TOPK_PRESEL: counting pre-pass of the merge kernel from PRESEL * KP columns on (init = 1)
SAMPLE = 4096                       # columns the pre-pass samples for its value range
NT = 256
K_MAX = 2048
DIGIT_SHIFTS = (0, 11, 22, 33, 44, 55)          # the id tie-break of the select kernel: six digits of 11 bits

ROW_PATTERNS = ("random_ties", "few_distinct", "constant", "ascending", "descending", "sample_invalid", "sample_constant", "specials")
IDS_ROW_PATTERNS = ("random_ties", "few_distinct", "ascending", "descending", "sample_invalid", "specials") + \
    tuple(f"digit{s}" for s in DIGIT_SHIFTS)
FIELDS = ("alpha", "col_scale", "col_bias", "col0", "col_ids", "ids", "row_ncols", "largest", "k")
POISON_COL0 = -(10 ** 15)           # col0 where col_ids / ids must win: every column would be skipped


def sub_block(KP):
    """columns the merge kernel appends between two looks at the candidate count"""
    return max(KP // 2, NT)


def _first(ladder, k):
    return next(KP for KP in ladder if k <= KP)


def merge_kp(k):
    return next(KP for kk, KP in zip(MERGE_K, MERGE_KP) if k <= kk)


def eff_ncols(call):
    """[n] columns that count per row: min(ncols, row_ncols[r]), never below 0"""
    n, nc = call["scores"].shape[0], call["ncols"]
    rn = call.get("row_ncols")
    return np.full(n, nc, dtype=np.int64) if rn is None else np.clip(np.minimum(rn.astype(np.int64), nc), 0, None)


def route(call):
    """What topk_merge() launches: 'select<KP,EPT>', 'merge<KP>' or 'merge<KP>+prepass' (the pre-pass is decided per row: named when
    any row takes it)."""
    k, nc = call["k"], call["ncols"]
    if call["init"] and nc <= SELECT_MAX_NCOLS:
        return f"select<{_first(SELECT_KP, k)},{16 if nc <= SELECT_REG_NCOLS else 20}>"
    KP = merge_kp(k)
    pre = bool(call["init"]) and bool((eff_ncols(call) >= PRESEL * KP).any())
    return f"merge<{KP}>" + ("+prepass" if pre else "")


ALL_ROUTES = tuple(f"select<{KP},{E}>" for KP in SELECT_KP for E in (16, 20)) + \
    tuple(f"merge<{KP}>{p}" for KP in MERGE_KP for p in ("", "+prepass"))


# ------------------------------------------------------------------------------------------------------ the header, restated
def value(scores, alpha=1.0, col_scale=None, col_bias=None):
    """float32, rounded after each of the three operations (numpy's float32 arithmetic does exactly that)"""
    with np.errstate(all="ignore"):
        v = np.asarray(scores, dtype=F32) * F32(1.0 if alpha == 0 else alpha)
        if col_scale is not None:
            v = v * np.asarray(col_scale, dtype=F32)
        if col_bias is not None:
            v = v + np.asarray(col_bias, dtype=F32)
    assert v.dtype == F32
    return v


def column_ids(call):
    """[n, ncols]: ids over col_ids over col0 + c"""
    n, nc = call["scores"].shape
    if call.get("ids") is not None:
        return np.asarray(call["ids"], dtype=np.int64)[:, :nc]
    if call.get("col_ids") is not None:
        return np.broadcast_to(np.asarray(call["col_ids"], dtype=np.int64)[:nc], (n, nc))
    return np.broadcast_to(np.int64(call.get("col0", 0)) + np.arange(nc, dtype=np.int64), (n, nc))


def values(call):
    return value(call["scores"], call.get("alpha", 1.0), call.get("col_scale"), call.get("col_bias"))


def valid(call):
    v = values(call)
    worst = -np.inf if call["largest"] else np.inf
    cols = np.arange(call["ncols"])[None, :] < eff_ncols(call)[:, None]
    return cols & (column_ids(call) >= 0) & ~np.isnan(v) & (v != worst)


def empty_state(n, k, largest):
    return np.full((n, k), -np.inf if largest else np.inf, dtype=F32), np.full((n, k), -1, dtype=np.int64)


def fold(call, state=None):
    """(best_val [n, k] f32, best_id [n, k] i64) after the call.  ``state``: (val, id) before it (ignored with init = 1)."""
    n, k, largest = call["scores"].shape[0], call["k"], call["largest"]
    out_v, out_i = empty_state(n, k, largest)
    if call["init"] or state is None:
        state = empty_state(n, k, largest)
    v, ids, ok = values(call), column_ids(call), valid(call)
    for r in range(n):
        real = state[1][r] >= 0
        vs = np.concatenate([state[0][r][real], v[r][ok[r]]]) + F32(0)         # (-0 -> +0: the sign of a zero is unspecified)
        is_ = np.concatenate([state[1][r][real], ids[r][ok[r]]])
        order = np.lexsort((is_, -vs if largest else vs))[:k]
        out_v[r, :len(order)], out_i[r, :len(order)] = vs[order], is_[order]
    return out_v, out_i


def split(call, c0, c1, init):
    """the columns [c0, c1) of a call as a call of their own (what a caller that walks a row in chunks passes)"""
    sub = dict(call, scores=call["scores"][:, c0:c1], ncols=c1 - c0, init=init)
    for f in ("col_ids", "col_scale", "col_bias"):
        if call.get(f) is not None:
            sub[f] = call[f][c0:c1]
    if call.get("ids") is not None:
        sub["ids"] = call["ids"][:, c0:c1]
    sub["col0"] = call.get("col0", 0) + (0 if call.get("col_ids") is not None or call.get("ids") is not None else c0)
    if call.get("row_ncols") is not None:
        sub["row_ncols"] = (call["row_ncols"].astype(np.int64) - c0).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32)   # may be < 0 or > ncols
    return sub


def fold_chunks(call, cuts):
    """fold the row chunk by chunk: cuts = [(c0, c1), ...] in any order that covers the columns once"""
    state = None
    for j, (c0, c1) in enumerate(cuts):
        state = fold(split(call, c0, c1, init=int(j == 0)), state)
    return state


# ------------------------------------------------------------------------------------------------------ rows
def _payload_ids(rs, m):
    """m unique ids shaped like the search's payloads: id << 24 | label, id < 2^31 (tied keys differ in bits 24..55)"""
    if m == 0:
        return np.zeros(0, dtype=np.int64)
    stride = (1 << 31) // m
    hi = rs.permutation(m).astype(np.int64) * stride + rs.randint(0, stride, m)
    return (hi << 24) | rs.randint(0, 1 << 24, m).astype(np.int64)


def _goodness(rs, pattern, nc, k):
    """[nc] float64 'goodness' (larger = better, multiples of 1/64 with |g| < 2^11) and a mask of columns to invalidate"""
    bad = np.zeros(nc, dtype=bool)
    tail = rs.randint(-2048, 2048, nc) / 64.0
    if pattern == "random_ties":
        g = tail
    elif pattern == "few_distinct":
        g = rs.randint(0, 5, nc) * 0.75
    elif pattern == "constant":
        g = np.full(nc, 1.5)
    elif pattern == "ascending":                                       # every column beats the running threshold
        g = np.arange(nc) / 16.0
    elif pattern == "descending":
        g = (nc - np.arange(nc)) / 16.0
    elif pattern == "sample_invalid":                                  # the pre-pass's sample holds nothing
        g = tail
        bad[:SAMPLE] = True
    elif pattern == "sample_constant":
        g = np.where(np.arange(nc) < SAMPLE, 0.0, tail)
    else:
        raise ValueError(pattern)
    return g, bad


SPECIALS = np.array([-np.inf, np.inf, np.nan, -0.0, 0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 3.0e38, -3.0e38,
                     1.0, -1.0], dtype=F32)


def digit_row(rs, nc, k, shift):
    """goodness [nc] and ids [nc]: a run of tied values across the cut whose ids are ``base | perm << shift`` (they differ in ONE
    11-bit digit; at shift 55 only 8 bits exist below 2^63), ``a`` strictly better columns, the rest strictly worse; shuffled."""
    tmax = 256 if shift == 55 else 2048
    T = min(tmax, nc, max(2, k))
    a = min(max(0, k - T // 2), nc - T)
    g = np.concatenate([1.0 + (1 + rs.permutation(a)) / 64.0, np.full(T, 1.0), -(1 + rs.permutation(nc - a - T)) / 64.0])
    digit = np.int64((tmax - 1) << shift)
    base = np.int64(rs.randint(0, 1 << 31)) << 32 | np.int64(rs.randint(0, 1 << 32))
    base = (base & np.int64((1 << 62) - 1)) & ~digit
    run = base | (rs.permutation(tmax)[:T].astype(np.int64) << shift)
    others = _payload_ids(rs, nc - T)
    ids = np.concatenate([others[:a], run, others[a:]])
    assert len(ids) == nc and len(np.unique(ids)) == nc and (ids >= 0).all()
    order = rs.permutation(nc)
    return g[order], ids[order]


XF_NAMES = ("none", "dyadic", "general", "alpha0")


def _transform(rs, xf, nc):
    """(alpha, col_scale, col_bias) of a transform kind"""
    if xf == "none":
        return 1.0, None, None
    if xf == "alpha0":                                                 # alpha 0 is read as 1; a scale alone
        return 0.0, rs.choice(np.array([-2.0, -1.0, 0.5, 2.0, 4.0], dtype=F32), nc).astype(F32), None
    if xf == "dyadic":
        return -2.0, rs.choice(np.array([-4.0, -1.0, -0.5, 0.25, 0.5, 2.0], dtype=F32), nc).astype(F32), \
            (rs.randint(1, 33, nc) * rs.choice([-1, 1], nc) / 4.0).astype(F32)
    if xf == "general":
        S = (rs.uniform(0.5, 2.0, 32) * rs.choice([-1.0, 1.0], 32)).astype(F32)
        B = rs.uniform(-3.0, 3.0, 32).astype(F32)
        return 0.7, S[np.arange(nc) % 32], B[np.arange(nc) % 32]
    raise ValueError(xf)


def make_case(spec):
    """spec: dict(k, ncols, largest, idmode in {'col0', 'col_ids', 'ids'}, xf in XF_NAMES, seed, ragged (bool), col0, init) -> call"""
    k, nc, largest, idmode, xf = spec["k"], spec["ncols"], int(spec["largest"]), spec["idmode"], spec["xf"]
    rs = np.random.RandomState(spec["seed"])
    patterns = IDS_ROW_PATTERNS if idmode == "ids" and xf != "general" else ROW_PATTERNS
    n = len(patterns)
    alpha, scale, bias = _transform(rs, xf, nc)
    a_eff = F32(1.0 if alpha == 0 else alpha)
    W = np.zeros((n, nc), dtype=F32)                                    # value space
    ids = np.zeros((n, nc), dtype=np.int64)
    bad = np.zeros((n, nc), dtype=bool)
    sgn = 1.0 if largest else -1.0
    for r, pat in enumerate(patterns):
        ids[r] = _payload_ids(rs, nc)
        if pat == "specials":
            W[r] = np.resize(SPECIALS, nc) if nc else W[r]
        elif pat.startswith("digit"):
            g, ids[r] = digit_row(rs, nc, k, int(pat[5:])) if nc >= 2 else (np.zeros(nc), ids[r])
            W[r] = (sgn * g).astype(F32)
        else:
            g, bad[r] = _goodness(rs, pat, nc, k)
            W[r] = (sgn * g).astype(F32)
    with np.errstate(all="ignore"):                                     # scores = the transform undone, step by step in float32
        s = W.copy()
        if bias is not None:
            s = s - bias
        if scale is not None:
            s = s / scale
        s = (s / a_eff).astype(F32)
    worst = F32(-np.inf if largest else np.inf)
    col_sign = np.sign(a_eff * (scale if scale is not None else np.ones(nc, dtype=F32))).astype(F32)
    half = (np.arange(nc) % 2 == 0)[None, :]
    s = np.where(bad & half, F32(np.nan), np.where(bad, worst * col_sign, s)).astype(F32)      # invalid: NaN / the worst infinity
    call = dict(scores=np.ascontiguousarray(s), ncols=nc, k=k, largest=largest, init=int(spec.get("init", 1)), alpha=alpha,
                col_scale=scale, col_bias=bias, col0=0, col_ids=None, ids=None, row_ncols=None, patterns=patterns, spec=spec)
    if idmode == "col0":
        call["col0"] = spec.get("col0", 7_000_000_000)
    else:
        call["col0"] = POISON_COL0                                      # must be ignored
        col_ids = _payload_ids(rs, nc)
        if idmode == "col_ids":
            col_ids[rs.rand(nc) < 0.05] = -1                            # skipped columns
            if nc >= 8:
                col_ids[nc // 2] = -7
            call["col_ids"] = col_ids
        else:
            skip = rs.rand(n, nc) < 0.03
            skip[[i for i, p in enumerate(patterns) if p.startswith("digit")]] = False
            ids[skip] = -1
            if nc >= 8:
                ids[0, nc // 3] = -(1 << 40)
            call["ids"] = ids
            call["col_ids"] = np.where(np.arange(nc) % 2 == 0, np.int64(-1), col_ids)    # must be ignored: other ids, half of them skipped
    if spec.get("ragged"):
        # rows that end early, one above ncols (clamped), 0 and a negative one (empty rows); the columns beyond hold the WINNING infinity
        rn = np.array([nc, nc + 7, max(nc - 1, 0), nc // 2, 0, -3, 1, min(nc, k), min(nc, k + 1), nc, max(nc - 300, 0), nc // 3, nc, nc][:n],
                      dtype=np.int32)
        rn[[i for i, p in enumerate(patterns) if p.startswith("digit")]] = nc
        beyond = np.arange(nc)[None, :] >= rn[:, None]
        call["scores"] = np.where(beyond, -worst * col_sign[None, :], call["scores"]).astype(F32)
        call["row_ncols"] = rn
    return call


def neutralise(call, field):
    """the call with one field neutralised or shifted (test_topk_ref_cpu.py: the expected bits must change)"""
    c = dict(call)
    if field == "alpha":
        c["alpha"] = 1.0
    elif field in ("col_scale", "col_bias", "row_ncols"):
        c[field] = None
    elif field == "col0":
        c["col0"] = call["col0"] + 1
    elif field in ("col_ids", "ids"):
        c[field] = np.where(call[field] >= 0, call[field] + 1, call[field])
    elif field == "largest":
        c["largest"] = 1 - call["largest"]
    elif field == "k":
        c["k"] = call["k"] - 1 if call["k"] > 1 else 2
    else:
        raise ValueError(field)
    return c


def fields_of(call):
    """the fields a case sets and must therefore be able to notice"""
    if call["ncols"] == 0:
        return ["largest", "k"]
    f = ["largest", "k", "ids" if call["ids"] is not None else "col_ids" if call["col_ids"] is not None else "col0"]
    if call["alpha"] not in (0.0, 1.0):
        f.append("alpha")
    return f + [x for x in ("col_scale", "col_bias", "row_ncols") if call[x] is not None]


# ------------------------------------------------------------------------------------------------------ case tables
IDMODES = ("col0", "col_ids", "ids")
SELECT_KS = {64: (1, 2, 63, 64), 256: (65, 255, 256), 1024: (257, 1023, 1024), 2048: (1025, 2047, 2048)}
SELECT_WIDE = (0, 1, 4095, 4096, 4097, 5119, 5120, 5121, 16384)
MERGE_KS = {512: (1, 8, 255, 256), 1024: (257, 1000, 1024), 2048: (1025, 2047, 2048)}
STATES = ("empty", "half", "full", "tied")


def _select_cases():
    """Every k of the issue with ncols in {k - 1, k, k + 1}; the other widths are dealt round over the k of one KP, so every KP sees every
    boundary and both EPT.  Direction, id mode, transform, ragged rows and col0 cycle with periods 2 / 3 / 4 / 5 / 3 over the running
    index (test_topk_ref_cpu.py checks what that covers)."""
    out, i = [], 0
    for KP, ks in SELECT_KS.items():
        for j, k in enumerate(ks):
            widths = sorted({k - 1, k, k + 1} | set(SELECT_WIDE[j::len(ks)]))
            for nc in widths:
                out.append(dict(k=k, ncols=nc, largest=(i // 3) % 2, idmode=IDMODES[i % 3], xf=XF_NAMES[(i // 2) % 4], seed=1000 + i,
                                ragged=i % 5 == 3, col0=(7_000_000_000, -5 if nc > 8 else 0, 0)[(i // 3) % 3], init=1))
                i += 1
    return out


def _merge_cases():
    """init = 0: chunk widths x incoming states for every KP (k, direction, id mode, transform cycle); init = 1 with 16385 columns (the
    pre-pass); the round-2 fold of the IVF-PQ search in small (per-row ids, row_ncols in {0, 1, cap}, largest)."""
    out, i = [], 0
    for KP, ks in MERGE_KS.items():
        SB = sub_block(KP)
        for w in (0, 1, 255, 256, 257, SB, SB + 1, 3 * SB + 5):
            for st in STATES:
                out.append(dict(k=ks[i % len(ks)], chunk=w, state=st, largest=(i // 3) % 2, idmode=IDMODES[i % 3], xf=XF_NAMES[(i // 2) % 4],
                                seed=5000 + i, ragged=i % 5 == 3, col0=(7_000_000_000, -5 if w > 8 else 0, 0)[(i // 3) % 3], init=0))
                i += 1
    for k in (8, 1024, 2048):
        for largest in (1, 0):
            out.append(dict(k=k, chunk=16385, state=None, largest=largest, idmode=IDMODES[i % 3], xf=XF_NAMES[i % 4], seed=5000 + i,
                            ragged=False, col0=0, init=1))
            i += 1
    for k, cap in ((64, 300), (1000, 600), (2048, 1100)):
        out.append(dict(k=k, chunk=cap, state="full", largest=1, idmode="ids", xf="none", seed=5000 + i, ragged="cap", col0=0, init=0))
        i += 1
    return out


def _chunk_cases():
    """rows of 12000 columns (the select kernel with EPT = 20 in one call; 8200 of them, above 2 KP for every KP, behind a 16385-wide
    descriptor for the pre-pass of the merge kernel) and how to cut them"""
    W, W1 = 12000, 8200
    cuts = {"one": [(0, W)], "1+rest": [(0, 1), (1, W)],
            "ragged": [(0, 37), (37, 37), (37, 300), (300, 1324), (1324, 5000), (5000, 5001), (5001, 11999), (11999, W)],
            "wide+rest": [(0, W1), (W1, W)]}
    out = []
    for i, k in enumerate((8, 200, 1000, 2048)):
        for largest in (1, 0):
            j = 2 * i + largest
            out.append(dict(k=k, ncols=W, largest=largest, idmode=IDMODES[j % 3], xf=XF_NAMES[j % 4], seed=9000 + j, ragged=False,
                            col0=7_000_000_000, init=1, cuts=cuts, wide=16385))
    return out


SELECT_CASES = _select_cases()
MERGE_CASES = _merge_cases()
CHUNK_CASES = _chunk_cases()


def select_case_id(s):
    return f"k{s['k']}-nc{s['ncols']}-{'max' if s['largest'] else 'min'}-{s['idmode']}-{s['xf']}{'-ragged' if s['ragged'] else ''}"


def merge_case_id(s):
    return f"k{s['k']}-w{s['chunk']}-{s['state']}-{'max' if s['largest'] else 'min'}-{s['idmode']}-{s['xf']}{'-ragged' if s['ragged'] else ''}"


def chunk_case_id(s):
    return f"k{s['k']}-{'max' if s['largest'] else 'min'}-{s['idmode']}-{s['xf']}"


def state_width(spec):
    """columns that make the incoming state of a merge case"""
    k = spec["k"]
    return {None: 0, "empty": 0, "half": (k + 1) // 2, "full": k + 37, "tied": k + 37}[spec["state"]]


def make_merge_case(spec):
    """-> (call, state): the chunk as a call with init = spec['init'] and the incoming state (None with init = 1).  The row universe is
    state_width + chunk columns wide; the state is the reference's fold of the columns the chunk does not take -- the LEFT ones, for
    'tied' the RIGHT ones (with col0 ids every chunk id is then smaller than every state id; permuted ids lie on both sides anyway)."""
    sw, w = state_width(spec), spec["chunk"]
    uni = make_case(dict(spec, ncols=sw + w, ragged=False, init=1))
    lo, hi = ((w, sw + w), (0, w)) if spec["state"] == "tied" else ((0, sw), (sw, sw + w))
    state = None if spec["init"] else fold(split(uni, lo[0], lo[1], init=1))
    call = split(uni, hi[0], hi[1], init=spec["init"])
    n = call["scores"].shape[0]
    if spec["ragged"]:
        worst = F32(-np.inf if spec["largest"] else np.inf)
        if spec["ragged"] == "cap":                                      # cand_cnt.clamp(max = cap) of the search
            rn = np.resize(np.array([w, 0, 1, w, 17, 0, w, 1], dtype=np.int32), n)
        else:
            rn = np.resize(np.array([w, w + 7, max(w - 1, 0), w // 2, 0, -3, 1, w // 3], dtype=np.int32), n)
        sc = call["col_scale"] if call["col_scale"] is not None else np.ones(w, dtype=F32)
        col_sign = np.sign(F32(1.0 if call["alpha"] == 0 else call["alpha"]) * sc).astype(F32)
        beyond = np.arange(w)[None, :] >= rn[:, None]
        call["scores"] = np.where(beyond, -worst * col_sign[None, :], call["scores"]).astype(F32)
        call["row_ncols"] = rn
    return call, state
