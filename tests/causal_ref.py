"""float64 restatement of the causal ('tgt','intra','tgt') attention as the C ABI states it (include/gnnlm.h: gnnlm_causal_attn,
gnnlm_causal_attn_varlen, gnnlm_causal_softmax), a plain float32 restatement that only sets bars, and the case tables of
tests/test_causal_abi_gpu.py.  Plain numpy; nothing here imports gnnlm_amd, and the rule is the header's, not the kernels':

    out[w, h] = sum_{u in block(w), u <= w, (max_ctx == 0 or w - u < max_ctx)} softmax_u(Q_w . K_u) V_u

Inputs (make_attn_case).  Every profile starts from Q = 0.3 randn, K = 0.3 sqrt(128 / dk) randn, V = randn: scores ~ N(0, 1) at every head
width, the scale of test_causal_attn_fused at d_k = 128.  The profiles other than ``flat`` overwrite the first column of each head with a
constant c_Q in Q and b_u (u: the key's position in its block) in K, so the score gains c_Q * b_u:

    flat      -                 every key matters
    rising    8, -10 .. +10     each new key tile's maximum is far above the running one (the rescale by exp(m_old - m_new))
    falling   8, +10 .. -10     the oldest keys of the window dominate: sensitive to kt_lo and the window's lower edge
    saw       8, +-6 per 32     the maximum goes up and down from tile to tile
    high      16, 12.5          every score + 200: without the maximum subtracted, exp overflows
    low       16, -12.5         every score - 200: without the maximum subtracted, every term underflows (0 / 0)

Q, K, V are column views of ONE [rows, 3 H dk + 8] buffer (how the forward hands them over: ld > H dk, pointers 16-byte aligned); its padding
columns and the SLACK_ROWS rows behind the tokens are NaN: no rule reads them, and whatever did would show.  The varlen block offsets are
handed over as a pointer to entry OFF0 of a longer table, so block_off[0] != 0.

Bars (attn_bar).  ``flat``: 2e-5, the bar of test_causal_attn_fused / test_star_attn_* / test_chain_attn at this input scale.  Every other
profile: max(2e-5, 4 * e32), e32 = max |causal_f32 - causal_ref| of the case itself; the 4 is for the kernels' other summation order (MFMA
k pairs, a running softmax over tiles of 32) over sums of the same length.  e32 as tests/test_causal_ref_cpu.py prints it (numpy 2.x,
x86-64; the bar is computed from the live value, this table is for the reader):

    case (fused: n_blocks x 256, d_k 128; varlen: block lengths)     e32        bar
    fused   1x256    H1  ctx0   rising                               7.14e-05   2.86e-04
    fused   3x256    H2  ctx33  rising                               1.05e-04   4.22e-04
    fused   2x256    H8  ctx0   falling                              9.68e-05   3.87e-04
    fused   1x256    H1  ctx33  falling                              5.97e-05   2.39e-04
    fused   3x256    H2  ctx0   saw                                  2.65e-05   1.06e-04
    fused   2x256    H8  ctx33  saw                                  5.17e-05   2.07e-04
    fused   1x256    H1  ctx0   high                                 1.62e-04   6.47e-04
    fused   3x256    H2  ctx33  high                                 1.25e-04   4.99e-04
    fused   2x256    H8  ctx0   low                                  1.29e-04   5.16e-04
    fused   1x256    H1  ctx33  low                                  1.24e-04   4.95e-04
    both    256+256  dk128 H2 ctx33 falling                          6.44e-05   2.58e-04
    varlen  64+65+97 dk16  H1 ctx0  rising                           1.54e-05   6.17e-05
    varlen  257+40   dk32  H2 ctx0  rising                           2.76e-05   1.11e-04
    varlen  64+65+97 dk64  H8 ctx33 rising                           6.80e-05   2.72e-04
    varlen  257+40   dk128 H1 ctx33 rising                           7.76e-05   3.10e-04
    varlen  64+65+97 dk16  H8 ctx0  falling                          3.19e-05   1.28e-04
    varlen  257+40   dk32  H1 ctx0  falling                          3.70e-05   1.48e-04
    varlen  64+65+97 dk64  H2 ctx33 falling                          4.51e-05   1.80e-04
    varlen  257+40   dk128 H8 ctx33 falling                          7.77e-05   3.11e-04
    varlen  64+65+97 dk16  H2 ctx0  saw                              7.61e-06   3.04e-05
    varlen  257+40   dk32  H8 ctx0  saw                              1.39e-05   5.56e-05
    varlen  64+65+97 dk64  H1 ctx33 saw                              2.32e-05   9.27e-05
    varlen  257+40   dk128 H2 ctx33 saw                              3.05e-05   1.22e-04
    varlen  64+65+97 dk16  H1 ctx0  high                             2.50e-05   9.99e-05
    varlen  257+40   dk32  H2 ctx0  high                             6.06e-05   2.43e-04
    varlen  64+65+97 dk64  H8 ctx33 high                             8.91e-05   3.56e-04
    varlen  257+40   dk128 H1 ctx33 high                             1.21e-04   4.83e-04
    varlen  64+65+97 dk16  H8 ctx0  low                              3.94e-05   1.58e-04
    varlen  257+40   dk32  H1 ctx0  low                              5.18e-05   2.07e-04
    varlen  64+65+97 dk64  H2 ctx33 low                              9.24e-05   3.70e-04
    varlen  257+40   dk128 H8 ctx33 low                              1.60e-04   6.40e-04
    softmax, scores randn + 200 / - 200, the largest of all shapes   1.05e-07 / 8.90e-08   1e-06 (the floor: the existing bar)

(``flat``, for comparison, at max_ctx 0 and 33: e32 between 2.8e-7 and 1.7e-6.  The element-by-element chain of 128 products behind a first
term of +-200 or +-80 is what makes e32 of the other profiles this large: every partial sum is rounded to ulp(|score|).)  The softmax bar
is max(1e-6, 4 * e32) with softmax_f32: the subtraction of the row maximum is exact for scores that close, so a shift of +-200 costs
nothing and the existing bar of 1e-6 stays in force."""
import zlib

import numpy as np

TOL = 2e-5                  # the bar of test_causal_attn_fused at this input scale
SOFTMAX_TOL = 1e-6          # the bar of test_causal_softmax_and_layernorm
MARGIN = 4
SLACK_ROWS = 4              # NaN rows behind the tokens of every operand buffer
LD_PAD = 8                  # NaN columns behind Q | K | V in a buffer row
OFF0 = 2                    # the kernels get a pointer to this entry of the block-offset table
TABLE_HEAD = [0, 7]         # the entries in front of it (so block_off[0] = 19 with the 12 rows of the second)
TABLE_TAIL = 5              # and what follows the last block: another block of 5 rows that the call does not name
FUSED_T, FUSED_DK = 256, 128
PROFILES = {"flat": None, "rising": (8.0, "rising"), "falling": (8.0, "falling"), "saw": (8.0, "saw"), "high": (16.0, 12.5), "low": (16.0, -12.5)}


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


# ======================================================================================================== the references
def _keep(n, max_ctx, edit=None):
    """bool [n, n]: key u takes part in query w of a block of n tokens.  edit (the mutations below): "no-diagonal" drops u == w,
    "no-oldest-tile" the keys of the first tile of 32 that the window of w touches -- both only where a key is left."""
    w, u = np.arange(n)[:, None], np.arange(n)[None, :]
    ok = (u <= w) & ((w - u < max_ctx) if max_ctx > 0 else True)
    if edit == "no-diagonal":
        ok2 = ok & (u != w)
    elif edit == "no-oldest-tile":
        lo = np.maximum(0, w - max_ctx + 1) if max_ctx > 0 else np.zeros_like(w)
        ok2 = ok & (u // 32 != lo // 32)
    else:
        assert edit is None
        return ok
    return np.where(ok2.any(1, keepdims=True), ok2, ok)


def causal_ref(Q, K, V, lengths, H, max_ctx, edit=None):
    """float64.  Q, K, V: [n_tok, H * dk] (any float type, views welcome), lengths: tokens per block -> [n_tok, H * dk]."""
    n_tok, d = Q.shape
    dk = d // H
    assert sum(lengths) == n_tok and H * dk == d
    out, r0 = np.zeros((n_tok, d)), 0
    for n in lengths:
        q, k, v = (np.asarray(a[r0:r0 + n], dtype=np.float64).reshape(n, H, dk).transpose(1, 0, 2) for a in (Q, K, V))     # [H, n, dk]
        s = np.where(_keep(n, max_ctx, edit)[None], np.matmul(q, k.transpose(0, 2, 1)), -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        out[r0:r0 + n] = np.matmul(p / p.sum(-1, keepdims=True), v).transpose(1, 0, 2).reshape(n, d)
        r0 += n
    return out


def causal_f32(Q, K, V, lengths, H, max_ctx, subtract_max=True):
    """The same in plain float32, to set bars: every score accumulated element by element in ascending k (np.float32 products and sums,
    vectorised over the (w, u) pairs), one softmax per row with the maximum subtracted (or not: what high / low are there to catch), P.V in
    float32."""
    n_tok, d = Q.shape
    dk = d // H
    out, r0 = np.zeros((n_tok, d), dtype=np.float32), 0
    for n in lengths:
        q, k, v = (np.ascontiguousarray(np.asarray(a[r0:r0 + n], dtype=np.float32).reshape(n, H, dk).transpose(1, 0, 2)) for a in (Q, K, V))
        s = np.zeros((H, n, n), dtype=np.float32)
        for e in range(dk):
            s += q[:, :, e, None] * k[:, None, :, e]
        s = np.where(_keep(n, max_ctx)[None], s, np.float32(-np.inf))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            p = np.exp(s - s.max(-1, keepdims=True)) if subtract_max else np.exp(s)
            p = p / p.sum(-1, keepdims=True, dtype=np.float32)
            o = np.matmul(p, v)
        assert s.dtype == p.dtype == o.dtype == np.float32
        out[r0:r0 + n] = o.transpose(1, 0, 2).reshape(n, d)
        r0 += n
    return out


def softmax_ref(S, T, max_ctx):
    """float64.  S [n_mats, T, ld]: row w keeps the columns max(0, w - max_ctx + 1) .. w (0 .. w if max_ctx == 0), softmax over them;
    every other column, the padding T .. ld included, is zero."""
    n_mats, T_, ld = S.shape
    assert T_ == T and ld >= T
    ok = np.zeros((T, ld), dtype=bool)
    ok[:, :T] = _keep(T, max_ctx)
    s = np.where(ok[None], S.astype(np.float64), -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def softmax_f32(S, T, max_ctx):
    ok = np.zeros(S.shape[1:], dtype=bool)
    ok[:, :T] = _keep(T, max_ctx)
    s = np.where(ok[None], S.astype(np.float32), np.float32(-np.inf))
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True, dtype=np.float32)
    assert p.dtype == np.float32
    return p


def ragged_tiles(lengths):
    """int32 [n_tiles, 2]: the (block, tile of 32 queries) table as gnnlm_ragged_tiles writes it -- descending query tile, blocks in order
    among equals (the GPU test compares it with the library's)."""
    t = [(b, qt) for b, n in enumerate(lengths) for qt in range((n + 31) // 32)]
    t.sort(key=lambda e: -e[1])                             # (stable)
    return np.array(t, dtype=np.int32).reshape(-1, 2)


# ======================================================================================================== the case tables
# Each case names its route: what the launchers' conditions (causal_attn_fused_ok: T == 256 && d_k == 128; causal_attn_varlen_ok: d_k in
# {16, 32, 64, 128}) give for it, asserted by tests/test_causal_ref_cpu.py through attn_route().
FUSED_SHAPES = [(1, 1), (3, 2), (2, 8)]                     # (n_blocks, H)
FUSED_CTX = [0, 1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 1000]
LDO_PADS = [0, 12]                                          # ldo = H * dk + this
PROFILE_CTX = [0, 33]
VARLEN_DK = [16, 32, 64, 128]
VARLEN_H = [1, 2, 8]
VARLEN_LENGTHS = [[1], [1, 31, 32, 33], [64, 65, 97], [257, 40], [8, 8, 8, 8], [256, 256]]
VARLEN_CTX = [0, 1, 31, 32, 33, 40, 64, 65, 100, 10000]
# the smallest shapes at which a query tile starts above key tile 0 (kt_lo > 0: a block of >= 65 tokens, 2 <= max_ctx <= 64), at which its
# first key tile is wholly masked for its later queries (max_ctx = 33 on >= 97 tokens) and at which the window covers three key tiles with
# the first partly masked: every head width gets each of them
VARLEN_WINDOWS = [([64, 65, 97], 33), ([64, 65, 97], 40), ([257, 40], 65), ([257, 40], 0)]
PROFILE_LENGTHS = [[64, 65, 97], [257, 40]]


def _fused_cases():
    cases = []
    for j, ctx in enumerate(FUSED_CTX):                     # flat: every value of every argument
        nb, H = FUSED_SHAPES[j % 3]
        cases.append(dict(route="fused", n_blocks=nb, H=H, max_ctx=ctx, ldo_pad=LDO_PADS[j % 2], profile="flat"))
    n = 0
    for profile in PROFILES:
        for ctx in PROFILE_CTX:
            if profile != "flat":
                nb, H = FUSED_SHAPES[n % 3]
                cases.append(dict(route="fused", n_blocks=nb, H=H, max_ctx=ctx, ldo_pad=LDO_PADS[n % 2], profile=profile))
                n += 1
    return cases


def _varlen_cases():
    cases, seen = [], set()

    def add(lengths, dk, H, ctx, pad, profile):
        c = dict(route="fused+varlen" if lengths == [256, 256] and dk == 128 else "varlen", lengths=list(lengths), dk=dk, H=H, max_ctx=ctx,
                 ldo_pad=pad, profile=profile)
        if attn_case_id(c) not in seen:
            seen.add(attn_case_id(c))
            cases.append(c)

    for i, lengths in enumerate(VARLEN_LENGTHS):            # flat: every length set x every max_ctx; d_k, H and ldo go round
        for j, ctx in enumerate(VARLEN_CTX):
            add(lengths, VARLEN_DK[(i + j) % 4], VARLEN_H[(i + 2 * j) % 3], ctx, LDO_PADS[(i + j) % 2], "flat")
    for i, dk in enumerate(VARLEN_DK):
        for j, (lengths, ctx) in enumerate(VARLEN_WINDOWS):
            add(lengths, dk, VARLEN_H[(i + j) % 3], ctx, LDO_PADS[j % 2], "flat")
    add([256, 256], 128, 2, 0, 12, "flat")                  # the shape both routes take
    add([256, 256], 128, 2, 33, 0, "falling")
    n = 0
    for profile in PROFILES:
        for ctx in PROFILE_CTX:
            for lengths in PROFILE_LENGTHS:
                if profile != "flat":
                    add(lengths, VARLEN_DK[n % 4], VARLEN_H[(n // 4 + n) % 3], ctx, LDO_PADS[n % 2], profile)
                    n += 1
    return cases


def attn_case_id(c):
    shape = f"{c['n_blocks']}x256" if "n_blocks" in c else "+".join(map(str, c["lengths"]))
    return f"{c['route']}-{shape}-dk{c.get('dk', FUSED_DK)}-H{c['H']}-ctx{c['max_ctx']}-ldo+{c['ldo_pad']}-{c['profile']}"


FUSED_CASES = _fused_cases()
VARLEN_CASES = _varlen_cases()
CROSS_ROUTE_CASES = [c for c in VARLEN_CASES if c["route"] == "fused+varlen"]

SOFTMAX_SHAPES = [(1, 4, 1), (5, 8, 3), (37, 40, 6), (64, 64, 2), (65, 68, 3), (130, 132, 5), (256, 256, 2)]       # (T, ld, n_mats)
SOFTMAX_SHIFTS = [0.0, 200.0, -200.0]
SOFTMAX_CASES = [dict(route="softmax", T=T, ld=ld, n_mats=m, max_ctx=ctx, shift=sh)
                 for T, ld, m in SOFTMAX_SHAPES for ctx in sorted({0, 1, 5, T - 1, T, T + 5}) for sh in SOFTMAX_SHIFTS]


def softmax_case_id(c):
    return f"softmax-T{c['T']}-ld{c['ld']}-m{c['n_mats']}-ctx{c['max_ctx']}-shift{c['shift']:+.0f}"


def attn_route(T_or_lengths, dk):
    """The kernels a shape can go through, from the launchers' own conditions."""
    routes = []
    lengths = [T_or_lengths] if isinstance(T_or_lengths, int) else list(T_or_lengths)
    if all(n == FUSED_T for n in lengths) and dk == FUSED_DK:
        routes.append("fused")
    if dk in (16, 32, 64, 128) and not isinstance(T_or_lengths, int):
        routes.append("varlen")
    return "+".join(routes)


# ======================================================================================================== the inputs
def _bias(profile, n):
    """b_u of a block of n tokens"""
    kind = PROFILES[profile][1]
    u = np.arange(n)
    if kind == "rising":
        return -10.0 + 20.0 * u / max(n - 1, 1)
    if kind == "falling":
        return 10.0 - 20.0 * u / max(n - 1, 1)
    if kind == "saw":
        return np.where((u // 32) % 2 == 0, 6.0, -6.0)
    return np.full(n, float(kind))


def make_attn_case(c):
    """-> dict(buf [rows, ld] float32 (NaN outside the Q | K | V columns of the token rows), Q / K / V (views of it, [n_tok, H * dk]), ld, ldo,
    lengths, H, dk, max_ctx, n_tok, and for the varlen kernel table (int32, the whole block-offset table; the kernel gets table[OFF0:]) and
    tiles (int32 [n_tiles, 2], as gnnlm_ragged_tiles writes them))."""
    lengths = list(c["lengths"]) if "lengths" in c else [FUSED_T] * c["n_blocks"]
    H, dk = c["H"], c.get("dk", FUSED_DK)
    d, n_tok = H * dk, sum(lengths)
    rs = _rs("attn", attn_case_id(c))
    ld = 3 * d + LD_PAD
    buf = np.full((n_tok + SLACK_ROWS, ld), np.nan, dtype=np.float32)
    Q, K, V = (buf[:n_tok, j * d:(j + 1) * d] for j in range(3))
    Q[:] = 0.3 * rs.randn(n_tok, d)
    K[:] = 0.3 * np.sqrt(128.0 / dk) * rs.randn(n_tok, d)
    V[:] = rs.randn(n_tok, d)
    if PROFILES[c["profile"]] is not None:
        Q[:, ::dk] = PROFILES[c["profile"]][0]
        K[:, ::dk] = np.concatenate([_bias(c["profile"], n) for n in lengths])[:, None]
    table = np.array(TABLE_HEAD + list(TABLE_HEAD[-1] + 12 + np.concatenate([[0], np.cumsum(lengths)])), dtype=np.int64)
    table = np.concatenate([table, [table[-1] + TABLE_TAIL]]).astype(np.int32)
    return dict(buf=buf, Q=Q, K=K, V=V, ld=ld, ldo=d + c["ldo_pad"], lengths=lengths, H=H, dk=dk, max_ctx=c["max_ctx"], n_tok=n_tok,
                table=table, tiles=ragged_tiles(lengths))


def make_softmax_case(c):
    """-> S [n_mats, T, ld] float32: randn + shift in every column (the padding included: the kernel must zero it, not keep it)."""
    rs = _rs("softmax", softmax_case_id(c))
    return (rs.randn(c["n_mats"], c["T"], c["ld"]) + c["shift"]).astype(np.float32)


def tile_orders(tiles):
    """[(name, table)]: as written, reversed, and in a seeded shuffle -- a work list, so the result may not depend on its order"""
    perm = _rs("tiles", tiles.shape[0]).permutation(tiles.shape[0])
    return [("as-written", tiles), ("reversed", tiles[::-1].copy()), ("shuffled", tiles[perm].copy())]


# ======================================================================================================== bars
_BARS = {}


def attn_e32(c, case=None):
    key = attn_case_id(c)
    if key not in _BARS:
        a = case or make_attn_case(c)
        args = (a["Q"], a["K"], a["V"], a["lengths"], a["H"], a["max_ctx"])
        _BARS[key] = float(np.abs(causal_f32(*args).astype(np.float64) - causal_ref(*args)).max())
    return _BARS[key]


def attn_bar(c, case=None):
    """flat: TOL.  Every other profile: max(TOL, MARGIN * e32) of the case itself."""
    return TOL if c["profile"] == "flat" else max(TOL, MARGIN * attn_e32(c, case))


def softmax_e32(c, S=None):
    S = make_softmax_case(c) if S is None else S
    return float(np.abs(softmax_f32(S, c["T"], c["max_ctx"]).astype(np.float64) - softmax_ref(S, c["T"], c["max_ctx"])).max())


def softmax_bar(c, S=None):
    """randn scores: SOFTMAX_TOL.  Shifted by +-200: max(SOFTMAX_TOL, MARGIN * e32)."""
    return SOFTMAX_TOL if c["shift"] == 0 else max(SOFTMAX_TOL, MARGIN * softmax_e32(c, S))


# ======================================================================================================== mutations
def attn_mutations(a):
    """[(what, keyword arguments of causal_ref)] for a case of make_attn_case: neutral-looking changes of the reference's arguments, each
    listed only where it changes which keys a query sees (max_ctx acts as min(max_ctx, longest block); with one key per query -- max_ctx = 1
    or blocks of one token -- the softmax is 1 whatever else changes, and only max_ctx + 1 is left)."""
    lengths, H, dk, ctx = a["lengths"], a["H"], a["dk"], a["max_ctx"]
    longest = max(lengths)
    eff = longest if ctx == 0 else min(ctx, longest)
    base = dict(Q=a["Q"], K=a["K"], V=a["V"], lengths=lengths, H=H, max_ctx=ctx)
    res = []
    if ctx > 0:
        for c2 in (ctx - 1, ctx + 1):
            if c2 >= 1 and min(c2, longest) != eff:
                res.append((f"max_ctx -> {c2}", dict(base, max_ctx=c2)))
    elif longest >= 2:
        res.append((f"max_ctx -> {longest - 1}", dict(base, max_ctx=longest - 1)))
    if eff >= 2:
        if len(lengths) > 1:                                # the first token of block 1 becomes the last of block 0 (or the other way)
            l2 = list(lengths)
            l2[0], l2[1] = (l2[0] + 1, l2[1] - 1) if l2[1] > 1 else (l2[0] - 1, l2[1] + 1)
            res.append(("a token moved across the first block boundary", dict(base, lengths=l2)))
        if H > 1:
            res.append(("K read from the neighbouring head", dict(base, K=np.roll(a["K"], dk, axis=1))))
        res.append(("the diagonal key dropped", dict(base, edit="no-diagonal")))
        if longest > 32:
            res.append(("the oldest key tile of the window dropped", dict(base, edit="no-oldest-tile")))
    return res


# ======================================================================================================== the varlen table contract
CONTRACT_LENGTHS = [8, 8, 8, 8]                             # n_tiles <= n_tok / 32 + n_blocks = 5 leaves room for one entry more
CONTRACT_EXTRA = [(-1, 0), (4, 0), (0, -1), (0, 5)]         # no block / past the last block / no tile / past the block's end
CONTRACT_AT = 1                                             # where the extra entry goes into the table
# a last block that claims rows 24 .. 40 of a call that declares n_tok = 32: the entry is skipped.  The buffers hold OVERCLAIM_ROWS rows
# (poison, finite) so that a kernel that followed it would write where the test sees it, inside the allocation
OVERCLAIM_OFF = [19, 27, 35, 43, 59]
OVERCLAIM_N_TOK = 32
OVERCLAIM_ROWS = 48
POISON = 1e4


def attn_extent(a, n_rows=None, tables=None, n_tok=None):
    """What a call with the case's arguments can address, for every tile entry that passes the kernel's guards: -> dict(rows: the highest
    operand / output row + 1, in_cols: the highest column of a buffer row + 1, out_cols, ok: whether every entry the guards let through
    stays inside block_off[OFF0:] and the n_rows rows of the buffers)."""
    n_rows = a["buf"].shape[0] if n_rows is None else n_rows
    n_tok = a["n_tok"] if n_tok is None else n_tok
    off, tiles = tables or (a["table"][OFF0:], a["tiles"])
    n_blocks = len(a["lengths"])
    top, ok = 0, len(off) >= n_blocks + 1
    for blk, qt in np.asarray(tiles).reshape(-1, 2).tolist():
        if blk < 0 or blk >= n_blocks or qt < 0:
            continue
        r0, r1 = int(off[blk]) - int(off[0]), int(off[blk + 1]) - int(off[0])
        if r0 < 0 or r1 > n_tok or r1 <= r0 or 32 * qt >= r1 - r0:
            continue
        top = max(top, r1)
    d = a["H"] * a["dk"]
    return dict(rows=top, in_cols=3 * d, out_cols=d, ok=ok and top <= n_rows and 3 * d <= a["ld"] and d <= a["ldo"])
