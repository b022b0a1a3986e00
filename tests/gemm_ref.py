"""numpy restatement of gnnlm_gemm_nt and gnnlm_lse_reduce (include/gnnlm.h: gnnlm_gemm_t), of the dispatcher and the tile walk of
csrc/gemm_route.h; and the case table of tests/test_gemm_abi_gpu.py.  No torch, no device code.

A descriptor is a dict (``DESC_DEFAULTS``): every buffer is the flat float32 / int32 array that starts AT the descriptor's pointer,
so the strides, leading dimensions and batch offsets of the header are plain index arithmetic here.

  gemm_ref(d)        what the header promises, in float64: the whole C image (the bytes the call must leave untouched included),
                     or lse_part / lse_picked with the rows and entries that stay untouched
  lse_reduce_ref     log sum exp of the (max, sum) pairs
  route(d)           the kernel gemm_nt() launches: gemm_route() restated, and compared with it by test_gemm_ref_cpu.py
                     (GNNLM_GEMM_SCHED, GNNLM_GEMM_SCHED_MINK and GNNLM_GEMM_SKINNY unset)
  tile_walk          list position -> (tm, tn) of the four kernels that walk a tile list
  CASES / make_case  the table: per route exact data (small integers: every partial sum is exact in float32 in any order, the result
                     is the reference bit for bit at every precision) and random data (held to the accuracy bars)

The contract restated (the header says the same):
  store:  C[b][c_rows[r], n] = alpha * <A[b][a_rows[r]], W[b][n]> + gate[r] * bias + R[b][c_rows[r], n]   for r < min(M, *m_dev);
          a_rows[r] < 0 is a zero product row (bias and R still apply); a_rows, c_rows, gate and m_dev are shared by the batches;
          nothing else of C is written.
  LSE:    lse_part[r][p] = (alpha * max, sum exp(alpha x - alpha max)) over the columns [64 p, 64 p + 64) below N, (-inf, 0) for a
          part without a column; lse_picked[r] = alpha * x[r, lse_pick[r]] where 0 <= lse_pick[r] < N and untouched elsewhere; C is
          ignored; bias, gate, R, c_rows and batches are refused; every a_rows entry must be >= 0."""
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------ dispatch constants (csrc/gemm_route.h has
# the same names; test_gemm_ref_cpu.py compares the values)
DMA_BK = 32                  # the LDS-DMA kernel
DMA_BIG_TILES = 2048         # 256x256 tiles from this many of them on
DMA_MIN_K = 128
DMA_STORE_MIN_K = 512        # store problems below it only with the big tiles
ASTAT_K = 64                 # the A-stationary log-sum-exp kernel
ASTAT_MAX_M = 128 * 768
SCHED_MIN_K = 256            # the hand-placed loop
SCHED_K_MULT = 64
SCHED_HEAD_TILES = 2048      # log-sum-exp problems of this many 256x256 tiles stay on the LDS-DMA kernel
SKINNY_MAX_N = 256           # narrow outputs
SKINNY_K_MULT = 32
SKINNY_MIN_K = 512
SPLIT_MIN_K = 256            # pre-split planes
SPLIT_MIN_TILES = 256        # 128x128 tiles
SPLIT_BIG_TILES = 512        # 256x256 tiles
SPLIT_MDEV_BIG_M = 1 << 17
SMALL_TILES = 256            # fewer 128x128 tiles than this -> 64x64 tiles (store only)
MAX_TILE_ORDER = 66

SENT_BITS = 0x7FC0BEEF       # a NaN with a payload of its own: "untouched" is compared as bits

DESC_DEFAULTS = dict(
    A=None, lda=0, a_rows=None, W=None, ldw=0, C=None, ldc=0, c_rows=None, bias=None, bias_mode=0, gate=None, R=None, ldr=0,
    alpha=0.0, M=0, N=0, K=0, m_dev=None, m_out=False, batch1=0, batch2=0,
    sA1=0, sA2=0, sW1=0, sW2=0, sC1=0, sC2=0, sB1=0, sB2=0, sR1=0, sR2=0, precision=0, tile_order=0,
    lse=False, lse_pick=None, a_rows_bound=0,
    a_panel_rows=0,          # rows of one batch's A panel (what a_rows may index)
    c_panel_rows=0,          # rows of one batch's C (and R) panel (what c_rows may index)
    exact=False)             # small-integer data: products are taken in float32 (exact, and fast at the big shapes)
# R may be the string "C": the R pointer is the C pointer (in place)


def cdiv(a, b):
    return -(-a // b)


def sentinel(n):
    return np.full(n, SENT_BITS, dtype=np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def norm(d):
    """the descriptor as gemm_nt() reads it: alpha 0 -> 1, batch counts 0 -> 1"""
    p = dict(DESC_DEFAULTS)
    p.update(d)
    p["alpha"] = np.float32(1.0) if np.float32(p["alpha"]) == 0 else np.float32(p["alpha"])
    p["batch1"], p["batch2"] = p["batch1"] or 1, p["batch2"] or 1
    return p


def refusal(d):
    """The reason gemm_nt() returns GNNLM_E_INVALID (None: the call is accepted).  Pointer alignment is the caller's to check."""
    p = norm(d)
    if p["A"] is None or p["W"] is None or (p["C"] is None and not p["lse"]):
        return "null operand"
    if p["M"] < 0 or p["N"] <= 0 or p["K"] <= 0:
        return "bad shape"
    if p["K"] % 4 or p["lda"] % 4 or p["ldw"] % 4:
        return "K, lda, ldw must be multiples of 4"
    if any(p[s] % 4 for s in ("sA1", "sA2", "sW1", "sW2")):
        return "batch strides must be multiples of 4"
    if p["batch1"] < 1 or p["batch2"] < 1:
        return "bad batch"
    if not 0 <= p["precision"] <= 3:
        return "precision"
    if p["lse"] and p["batch1"] * p["batch2"] != 1:
        return "the LSE epilogue does not support batches"
    if p["lse"] and not p["alpha"] > 0:
        return "the LSE epilogue needs alpha > 0"
    if p["lse"] and any(p[f] is not None for f in ("bias", "gate", "R", "c_rows")):
        return "the LSE epilogue takes no bias, gate, R or c_rows"
    if not 0 <= p["tile_order"] <= MAX_TILE_ORDER:
        return "tile_order"
    return None


# ------------------------------------------------------------------------------------------ operand rounding
def _bf16_rn(x):
    u = bits(x)
    return (((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)).view(np.float32)


def _bf16_trunc(x):
    return (bits(x) & np.uint32(0xFFFF0000)).view(np.float32)


def planes(x, precision):
    """float32 operand -> the planes the matrix cores multiply (gemm_split.hip: split8; gemm_f32.hip: GNNLM_SPLIT_STORE).
    0: the value; 3: IEEE half, nearest even, overflow to inf; 1: two bf16 planes, value and residual both rounded to nearest;
    2: three bf16 planes by truncation (they add up to the value exactly)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if precision == 0:
        return [x]
    if precision == 3:
        with np.errstate(over="ignore"):
            return [x.astype(np.float16).astype(np.float32)]
    cut = _bf16_rn if precision == 1 else _bf16_trunc
    out = []
    for _ in range(2 if precision == 1 else 3):
        out.append(cut(x))
        x = x - out[-1]                              # exact in float32
    return out


# cross products kept: (plane of A, plane of W)
PRODUCTS = {0: [(0, 0)], 3: [(0, 0)], 1: [(0, 0), (0, 1), (1, 0)], 2: [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]}


def _panel(buf, off, rows, ld, cols):
    return buf[off:off + rows * ld].reshape(rows, ld)[:, :cols]


def products(d):
    """Per batch (b1 slow, b2 fast): (P, S) with P[i, n] = <A panel row i, W row n> under the precision's operand rounding, float64
    (float32 for exact data), and S = sum |a||w| (None for exact data).  The gather commutes with the product, so it is applied
    afterwards; the A panel has a_panel_rows rows."""
    p = norm(d)
    out = []
    dt = np.float32 if p["exact"] else np.float64
    for b1 in range(p["batch1"]):
        for b2 in range(p["batch2"]):
            A = _panel(p["A"], b1 * p["sA1"] + b2 * p["sA2"], p["a_panel_rows"], p["lda"], p["K"])
            W = _panel(p["W"], b1 * p["sW1"] + b2 * p["sW2"], p["N"], p["ldw"], p["K"])
            pa, pw = planes(A, p["precision"]), planes(W, p["precision"])
            P = None
            with np.errstate(invalid="ignore"):
                for i, j in PRODUCTS[p["precision"]]:
                    t = pa[i].astype(dt) @ pw[j].astype(dt).T
                    P = t if P is None else P + t
            S = None if p["exact"] else np.abs(A).astype(dt) @ np.abs(W).astype(dt).T
            out.append((P, S))
    return out


def check_exact(d):
    """The condition of the exact cases: integer operands in [-2, 2], so every partial sum is an integer below 2^24."""
    p = norm(d)
    for b1 in range(p["batch1"]):
        for b2 in range(p["batch2"]):
            for X in (_panel(p["A"], b1 * p["sA1"] + b2 * p["sA2"], p["a_panel_rows"], p["lda"], p["K"]),
                      _panel(p["W"], b1 * p["sW1"] + b2 * p["sW2"], p["N"], p["ldw"], p["K"])):
                if not (np.abs(X) <= 2).all() or not (X == np.round(X)).all():
                    return False
    return 4 * p["K"] < 2 ** 20


# ------------------------------------------------------------------------------------------ the contract
def m_effective(d):
    """min(M, *m_dev): a count above M is read as M, 0 is an empty problem; a negative one is outside the contract"""
    assert d.get("m_dev") is None or int(d["m_dev"]) >= 0, "m_dev must be >= 0"
    return d["M"] if d.get("m_dev") is None else min(d["M"], int(d["m_dev"]))


def gemm_ref(d, prods=None, strict=True):
    """-> dict.  store: C (float32 image of the whole buffer: the initial bytes where the call writes nothing), C64 (float64 values),
    scale (per element |alpha| sum |a||b| + |gate * bias| + |R|, the magnitude of the terms summed; None for exact data), written (mask).  LSE: part [M, n_parts, 2] float64, part_rows (rows
    written), logits are reduced per 64-column part; picked [M] float64, picked_written (mask).  Both: m_out, n_parts."""
    assert refusal(d) is None, refusal(d)
    p = norm(d)
    M, N = p["M"], p["N"]
    mo = m_effective(p)
    alpha = float(p["alpha"])
    out = {"m_out": mo, "n_parts": 2 * cdiv(N, 128)}
    if M == 0:
        mo = 0
    if prods is None and mo > 0:
        prods = products(p)
    rows = np.arange(mo)
    src = rows if p["a_rows"] is None else p["a_rows"][:mo].astype(np.int64)
    assert (src < p["a_panel_rows"]).all()
    cols = np.arange(N)

    if p["lse"]:
        assert (src >= 0).all(), "LSE: every a_rows entry must be >= 0"
        npart = out["n_parts"]
        part = np.full((M, npart, 2), np.nan)
        picked = np.full(M, np.nan)
        pw = np.zeros(M, dtype=bool)
        pick = None if p["lse_pick"] is None else p["lse_pick"].astype(np.int64)
        for r0 in range(0, mo, 256):
            r1 = min(mo, r0 + 256)
            x = prods[0][0][src[r0:r1]].astype(np.float64) * alpha
            xp = np.full((r1 - r0, npart * 64), -np.inf)
            xp[:, :N] = x
            xp = xp.reshape(r1 - r0, npart, 64)
            mx = xp.max(-1)
            with np.errstate(invalid="ignore"):
                s = np.where(np.isinf(xp), 0.0, np.exp(xp - mx[..., None])).sum(-1)
            part[r0:r1, :, 0], part[r0:r1, :, 1] = mx, s
            if pick is not None:
                pk = pick[r0:r1]
                ok = (pk >= 0) & (pk < N)
                picked[r0:r1][ok] = x[np.nonzero(ok)[0], pk[ok]]
                pw[r0:r1] = ok
        out.update(part=part, part_rows=mo, picked=picked, picked_written=pw)
        return out

    init = p["C"]
    img, C64 = init.copy(), np.zeros(len(init))
    scale = None if p["exact"] else np.zeros(len(init))
    written = np.zeros(len(init), dtype=bool)
    crow = rows if p["c_rows"] is None else p["c_rows"][:mo].astype(np.int64)
    rc = p["c_panel_rows"]
    assert (crow < rc).all() and len(set(crow.tolist())) == mo
    gate = 1.0 if p["gate"] is None else p["gate"][:mo].astype(np.float64)
    Rbuf = None if p["R"] is None else (init if isinstance(p["R"], str) else p["R"])

    def panel(buf, off, ld):                          # the rows x N window of a batch in a flat buffer
        return buf[off:off + rc * ld].reshape(rc, ld)[:, :N]

    for b1 in range(p["batch1"]):
        for b2 in range(p["batch2"]):
            if mo == 0:
                break
            P, S = prods[b1 * p["batch2"] + b2]
            x = P[np.maximum(src, 0)].astype(np.float64) * alpha
            x[src < 0] = 0.0
            extra = None if scale is None else np.zeros_like(x)      # |gate * bias| + |R|: the other terms of the sum, for the error scale
            if p["bias"] is not None:
                bb = p["bias"][b1 * p["sB1"] + b2 * p["sB2"]:].astype(np.float64)
                assert p["bias_mode"] in (1, 2)
                t = (gate * np.ones(mo))[:, None] * bb[:N][None, :] if p["bias_mode"] == 1 else (gate * bb[:mo])[:, None]
                x += t
                if extra is not None:
                    extra += np.abs(t)
            if Rbuf is not None:
                t = panel(Rbuf, b1 * p["sR1"] + b2 * p["sR2"], p["ldr"])[crow].astype(np.float64)
                x += t
                if extra is not None:
                    extra += np.abs(t)
            off = b1 * p["sC1"] + b2 * p["sC2"]
            w = panel(written, off, p["ldc"])
            assert not strict or not w[crow].any(), "two logical elements store to one address"
            panel(C64, off, p["ldc"])[crow] = x
            w[crow] = True
            if scale is not None:
                sc = S[np.maximum(src, 0)] * abs(alpha)
                sc[src < 0] = 0.0
                panel(scale, off, p["ldc"])[crow] = sc + extra
    img[written] = C64[written].astype(np.float32)
    out.update(C=img, C64=C64, scale=scale, written=written)
    return out


def lse_reduce_ref(part, m_dev=None):
    """part [rows, n_parts, 2] (max, sum) -> float64 [rows] log sum exp; rows >= m_dev are NaN here (untouched on the device).  A
    (-inf, 0) part adds nothing; a row of such parts only is -inf."""
    part = np.asarray(part, dtype=np.float64)
    rows = part.shape[0]
    m = rows if m_dev is None else max(0, min(rows, int(m_dev)))
    out = np.full(rows, np.nan)
    mx = part[:m, :, 0].max(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = np.where(np.isneginf(part[:m, :, 0]), 0.0, part[:m, :, 1] * np.exp(part[:m, :, 0] - mx[:, None]))
        out[:m] = np.where(np.isneginf(mx), -np.inf, mx + np.log(w.sum(-1)))
    return out


def part_lse(part):
    """m + log s per part, float64; -inf for a (-inf, 0) part"""
    part = np.asarray(part, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isneginf(part[..., 0]), -np.inf, part[..., 0] + np.log(part[..., 1]))


# ------------------------------------------------------------------------------------------ the dispatcher
def route(d):
    """The kernel gemm_nt() launches and its tile: 'reg64', 'reg128' (gemm_f32.hip, in-kernel split at precisions 1..3), 'sched128',
    'dma128', 'dma256', 'astat128' (gemm_f32_dma.hip), 'skinny32', 'split128', 'split256'; 'none' for M = 0."""
    p = norm(d)
    M, N, K, prec, lse = p["M"], p["N"], p["K"], p["precision"], bool(p["lse"])
    m_dev = p["m_dev"] is not None
    nb = p["batch1"] * p["batch2"]
    if M == 0:
        return "none"
    tiles128, tiles256 = cdiv(M, 128) * cdiv(N, 128), cdiv(M, 256) * cdiv(N, 256)
    # pre-split planes and their tile
    if prec != 0 and nb == 1 and K >= SPLIT_MIN_K and tiles128 >= SPLIT_MIN_TILES:
        big = (not m_dev or M >= SPLIT_MDEV_BIG_M) and tiles256 >= SPLIT_BIG_TILES
        return "split256" if big else "split128"
    # narrow outputs
    if prec == 0 and not lse and nb == 1 and N <= SKINNY_MAX_N and K % SKINNY_K_MULT == 0 and K >= SKINNY_MIN_K:
        return "skinny32"
    small = not lse and tiles128 * nb < SMALL_TILES
    if not small:
        # the hand-placed loop
        a_rows = p["a_rows_bound"] if p["a_rows"] is not None else M
        sched = (prec == 0 and not (lse and not m_dev and tiles256 >= SCHED_HEAD_TILES)
                 and K % SCHED_K_MULT == 0 and K >= SCHED_MIN_K and tiles128 * nb >= SMALL_TILES
                 and N * p["ldw"] * 4 < 2 ** 32 and a_rows > 0 and a_rows * p["lda"] * 4 < 2 ** 32)
        if sched:
            return "sched128"
        # LDS-DMA staging, the A-stationary kernel, the tile
        dma = True
        if not lse and (m_dev or (K < DMA_STORE_MIN_K and tiles256 * nb < DMA_BIG_TILES)):
            dma = False
        elif prec == 0 and K == ASTAT_K and lse and nb == 1 and M <= ASTAT_MAX_M:
            dma = True
        else:
            dma = prec == 0 and K % DMA_BK == 0 and K >= DMA_MIN_K
        if dma:
            if K == ASTAT_K and lse:
                return "astat128"
            return "dma256" if (not m_dev and tiles256 * nb >= DMA_BIG_TILES) else "dma128"
    return "reg64" if small else "reg128"


def resolved_tile_order(d):
    p = norm(d)
    return p["tile_order"] or (1 if (p["m_dev"] is None and p["M"] > p["N"]) else 2)


WALKS = ("reg64", "reg128", "sched128", "dma128", "dma256", "split128", "split256")     # routes that walk a tile list by tile_order
ROUTE_TILE = {"reg64": 64, "reg128": 128, "sched128": 128, "dma128": 128, "dma256": 256, "astat128": 128, "skinny32": 32,
              "split128": 128, "split256": 256}
# (route, lse) -> (kernel function, leading template arguments) for the profiler's kernel names; NS of the register-staged kernel:
# precision 0 -> 0, 1 -> 2, 2 -> 3, 3 -> 1; planes of the split kernel: 3 -> 1, 1 -> 2, 2 -> 3
_NS_REG = {0: 0, 1: 2, 2: 3, 3: 1}
_NS_SPLIT = {3: 1, 1: 2, 2: 3}


def kernel_symbol(rt, lse, precision):
    e = int(bool(lse))
    return {"reg64": ("gemm_nt_f32_kernel", (64, 64, e, _NS_REG[precision])),
            "reg128": ("gemm_nt_f32_kernel", (128, 128, e, _NS_REG[precision])),
            "sched128": ("gemm_nt_f32_sched_kernel", (e,)),
            "dma128": ("gemm_nt_f32_dma_kernel", (e, DMA_BK, 128)),
            "dma256": ("gemm_nt_f32_dma_kernel", (e, DMA_BK, 256)),
            "astat128": ("gemm_lse_astationary_kernel", (ASTAT_K,)),
            "skinny32": ("gemm_nt_f32_skinny_kernel", ()),
            "split128": ("gemm_planes_kernel", (128, _NS_SPLIT.get(precision, 0), e)),
            "split256": ("gemm_planes_kernel", (256, _NS_SPLIT.get(precision, 0), e))}[rt]


def tile_walk(tile_order, tiles_m, tiles_n):
    """[(tm, tn)] by list position, tile_order resolved (1: n fastest, 2: m fastest, 2 + GM: bands of GM m-tiles, n slow inside a
    band, the last band short)"""
    assert 1 <= tile_order <= MAX_TILE_ORDER
    out = []
    for t in range(tiles_m * tiles_n):
        if tile_order == 1:
            tm, tn = t // tiles_n, t % tiles_n
        elif tile_order == 2:
            tn, tm = t // tiles_m, t % tiles_m
        else:
            GM = tile_order - 2
            band = t // (GM * tiles_n)
            m_in = min(GM, tiles_m - band * GM)
            r = t - band * GM * tiles_n
            tn, tm = r // m_in, band * GM + r % m_in
        out.append((tm, tn))
    return out


# ------------------------------------------------------------------------------------------ the case table
SPEC_DEFAULTS = dict(flavour="store", precision=0, data="exact", a_rows=None, a_bound=False, c_rows=False, bias_mode=0, gate=False,
                     R=None, alpha=0.0, m_dev=None, m_out=False, batch=(0, 0), w_bcast=False, tile_order=0, pick=None)
GATES = np.array([0.0, 1.0, 0.5, -2.0, 1.5], dtype=np.float32)
PICK_EDGES = (0, 63, 64, 127, 128, "N-1", -1, "N", "N+5", -7)


def _m_dev_value(v, M):
    return None if v is None else (M + int(v[1:]) if isinstance(v, str) else v)      # "M-1", "M+5", "M+0"


def shape_desc(spec):
    """The descriptor of a case without its data: enough for route() and refusal()"""
    s = dict(SPEC_DEFAULTS)
    s.update(spec)
    M, N, K = s["M"], s["N"], s["K"]
    b1, b2 = s["batch"][0] or 1, s["batch"][1] or 1
    lse = s["flavour"] == "lse"
    d = dict(DESC_DEFAULTS)
    d.update(M=M, N=N, K=K, lda=K + 4, ldw=K + 8, precision=s["precision"], tile_order=s["tile_order"], alpha=s["alpha"],
             batch1=s["batch"][0], batch2=s["batch"][1], lse=lse, m_dev=_m_dev_value(s["m_dev"], M), m_out=s["m_out"],
             exact=s["data"] == "exact", bias_mode=s["bias_mode"])
    d["a_panel_rows"] = M + 7                                         # taller than M: the rows beyond it are for a_rows only
    d["a_rows"] = True if s["a_rows"] else None                       # placeholders: route() only asks whether they are there
    d["a_rows_bound"] = d["a_panel_rows"] if (s["a_rows"] and s["a_bound"]) else 0
    d["A"] = d["W"] = True
    d["C"] = None if lse else True
    PA, PW = d["a_panel_rows"] * d["lda"], N * d["ldw"]
    if b1 * b2 > 1:                                                   # every stride its own; b2 is the slow index of W and C
        d["sA2"], d["sA1"] = PA + 8, b2 * (PA + 8) + 4
        if not s["w_bcast"]:
            d["sW1"], d["sW2"] = PW + 4, b1 * (PW + 4) + 12
    if not lse:
        d["c_panel_rows"] = M + 5 if s["c_rows"] else M
        d["ldc"] = N + 1
        PC = d["c_panel_rows"] * d["ldc"]
        if b1 * b2 > 1:
            d["sC1"], d["sC2"] = PC + 3, b1 * (PC + 3) + 5
        if s["R"] == "alias":
            d["ldr"], d["sR1"], d["sR2"] = d["ldc"], d["sC1"], d["sC2"]
        elif s["R"]:
            d["ldr"] = N + 3
            PR = d["c_panel_rows"] * d["ldr"]
            if b1 * b2 > 1:
                d["sR2"], d["sR1"] = PR + 1, b2 * (PR + 1) + 2
        if s["bias_mode"] and b1 * b2 > 1:
            nbias = N if s["bias_mode"] == 1 else M
            d["sB1"], d["sB2"] = nbias + 2, b1 * (nbias + 2) + 1
    return d, s


def make_case(spec):
    """The descriptor of a case, data included (deterministic per name)."""
    d, s = shape_desc(spec)
    seed = s.get("seed") or s["name"]                                 # cases of one seed share A and W (and their products)
    rs = np.random.RandomState(zlib.crc32(s["name"].encode()) & 0x7FFFFFFF)
    rs_op = {w: np.random.RandomState(zlib.crc32((seed + w).encode()) & 0x7FFFFFFF) for w in "AW"}
    M, N, K = s["M"], s["N"], s["K"]
    b1, b2 = s["batch"][0] or 1, s["batch"][1] or 1
    lse, exact = d["lse"], d["exact"]
    ra = d["a_panel_rows"]
    krange = np.logspace(-2, 2, K).astype(np.float32)

    def operand(rows, ld, s1, s2, n1, n2, which):
        rs = rs_op[which]
        buf = np.full((n1 - 1) * s1 + (n2 - 1) * s2 + rows * ld, np.nan, dtype=np.float32)     # the pad columns are never read
        for i in range(n1):
            for j in range(n2):
                if exact:
                    x = rs.randint(-2, 3, (rows, K)).astype(np.float32)
                    if lse and which == "A":          # three entries per row: logits of order 1, so exp() keeps its accuracy
                        keep = np.zeros((rows, K), dtype=bool)
                        keep[np.arange(rows)[:, None], rs.randint(0, K, (rows, 3))] = True
                        x = np.where(keep, np.where(x == 0, 1.0, x), 0.0).astype(np.float32)
                else:
                    x = rs.standard_normal((rows, K)).astype(np.float32)
                    if which == "A":
                        x *= krange                  # a wide dynamic range along k
                _panel(buf, i * s1 + j * s2, rows, ld, K)[:] = x
        return buf

    d["A"] = operand(ra, d["lda"], d["sA1"], d["sA2"], b1, b2, "A")
    d["W"] = operand(N, d["ldw"], d["sW1"], d["sW2"], 1 if s["w_bcast"] else b1, 1 if s["w_bcast"] else b2, "W")
    if s["alpha"] == "unit":                          # random LSE data: logits of order 1
        d["alpha"] = float(np.float32(1.0 / np.sqrt(float((krange.astype(np.float64) ** 2).sum()))))

    def values(n, step, lim):
        if exact:
            return (rs.randint(-lim, lim + 1, n) * step).astype(np.float32)
        return rs.standard_normal(n).astype(np.float32)

    kind = s["a_rows"]
    if kind:
        if kind == "identity":
            a = np.arange(M)
        else:                                         # a permutation of the panel with repeats
            a = rs.permutation(ra)[:M]
            a[rs.rand(M) < 0.2] = a[0]
            a[M // 2] = ra - 1
            if kind == "neg":                         # zero rows, first and last row among them
                a[rs.rand(M) < 0.2] = -1
                a[0] = a[M - 1] = -1
                if M > 3:
                    a[1] = 3
        d["a_rows"] = a.astype(np.int32)
    if lse:
        if s["pick"] == "edges":
            ev = [N - 1 if e == "N-1" else N if e == "N" else N + 5 if e == "N+5" else e for e in PICK_EDGES]
            d["lse_pick"] = np.array([ev[(r + r // 128) % len(ev)] for r in range(M)], dtype=np.int32)
        elif s["pick"] == "random":
            d["lse_pick"] = rs.randint(0, N, M).astype(np.int32)
        return d

    rc = d["c_panel_rows"]
    if s["c_rows"]:
        d["c_rows"] = rs.permutation(rc)[:M].astype(np.int32)
    nC = (b1 - 1) * d["sC1"] + (b2 - 1) * d["sC2"] + rc * d["ldc"]
    if s["R"] == "alias":
        d["C"], d["R"] = values(nC, 0.125, 64), "C"
    else:
        d["C"] = sentinel(nC)
        if s["R"]:
            d["R"] = values((b1 - 1) * d["sR1"] + (b2 - 1) * d["sR2"] + rc * d["ldr"], 0.125, 64)
    if s["bias_mode"]:
        nbias = N if s["bias_mode"] == 1 else M
        d["bias"] = values((b1 - 1) * d["sB1"] + (b2 - 1) * d["sB2"] + nbias, 0.25, 16)
        if s["gate"]:
            g = GATES[rs.randint(0, len(GATES), M)]
            g[:min(M, 5)] = GATES[:min(M, 5)]
            d["gate"] = g if exact else (g * rs.standard_normal(M)).astype(np.float32)
    return d


_PRODUCTS = {}


def case_products(spec, d):
    """products(d) of a case of the table, kept for the next cases of the same seed (they share A and W)"""
    s = dict(SPEC_DEFAULTS)
    s.update(spec)
    key = (s.get("seed") or s["name"], s["M"], s["N"], s["K"], s["precision"], s["batch"], s["w_bcast"], s["flavour"], s["data"])
    if key not in _PRODUCTS:
        _PRODUCTS.clear()
        _PRODUCTS[key] = products(d)
    return _PRODUCTS[key]


# the smallest shapes that reach each route: M and N no multiples of the tile, K the smallest the route takes
BIG = (2050, 1990)                                                   # 17 x 16 tiles of 128: >= 256 of them
STORE_ROUTES = [                                                      # (tag, route, M, N, K, precision, extra)
    ("reg64", "reg64", 70, 130, 36, 0, {}),
    ("reg64ns2", "reg64", 70, 130, 36, 1, {}),
    ("reg64ns3", "reg64", 70, 130, 36, 2, {}),
    ("reg64ns1", "reg64", 70, 130, 36, 3, {}),
    ("reg128", "reg128", *BIG, 100, 0, {}),
    ("reg128ns2", "reg128", *BIG, 100, 1, {}),
    ("reg128ns3", "reg128", *BIG, 100, 2, {}),
    ("reg128ns1", "reg128", *BIG, 100, 3, {}),
    ("sched", "sched128", *BIG, 256, 0, {}),
    ("dma128", "dma128", *BIG, 544, 0, {}),
    ("dma256", "dma256", 257, 261, 128, 0, dict(batch=(16, 32))),    # 2048 tiles of 256 through the batch count: 4 per batch
    ("skinny", "skinny32", 70, 40, 512, 0, {}),
    ("split128p1", "split128", *BIG, 256, 1, {}),
    ("split128p2", "split128", *BIG, 256, 2, {}),
    ("split128p3", "split128", *BIG, 256, 3, {}),
    ("split256p1", "split256", 5900, 5900, 256, 1, {}),
    ("split256p2", "split256", 5900, 5900, 256, 2, {}),
    ("split256p3", "split256", 5900, 5900, 256, 3, {}),
]
LSE_ROUTES = [
    ("reg128", "reg128", 130, 300, 100, 0, {}),
    ("reg128ns2", "reg128", 130, 300, 100, 1, {}),
    ("reg128ns3", "reg128", 130, 300, 100, 2, {}),
    ("reg128ns1", "reg128", 130, 300, 100, 3, {}),
    ("sched", "sched128", *BIG, 256, 0, {}),
    ("dma128", "dma128", 130, 300, 160, 0, {}),
    ("astat", "astat128", 129, 300, 64, 0, {}),
    ("dma256", "dma256", 2049, 58200, 128, 0, {}),                   # 9 x 228 tiles of 256; exact data only (the reference's cost)
    ("split128p1", "split128", *BIG, 256, 1, {}),
    ("split128p2", "split128", *BIG, 256, 2, {}),
    ("split128p3", "split128", *BIG, 256, 3, {}),
    ("split256p1", "split256", 5900, 5900, 256, 1, {}),
    ("split256p2", "split256", 5900, 5900, 256, 2, {}),
    ("split256p3", "split256", 5900, 5900, 256, 3, {}),
]
# fields of the store flavour, one at a time and in the pairs that interact; every case also carries lda = K + 4, ldw = K + 8,
# ldc = N + 1 and (on the device) C, R and bias one float off a 16-byte boundary
STORE_FIELDS = [
    ("plain", {}),
    ("a_id", dict(a_rows="identity")),
    ("a_neg", dict(a_rows="neg")),
    ("a_neg_bound", dict(a_rows="neg", a_bound=True)),
    ("c_rows", dict(c_rows=True)),
    ("c_rows_inplace", dict(c_rows=True, R="alias")),
    ("R", dict(R="sep")),
    ("bias1", dict(bias_mode=1)),
    ("bias1_gate", dict(bias_mode=1, gate=True)),
    ("bias2", dict(bias_mode=2)),
    ("bias2_gate", dict(bias_mode=2, gate=True)),
    ("alpha_half", dict(alpha=0.5)),
    ("alpha_neg", dict(alpha=-2.0)),
    ("m_dev0", dict(m_dev=0, m_out=True)),
    ("m_dev1", dict(m_dev=1, m_out=True)),
    ("m_devM-1", dict(m_dev="M-1", m_out=True)),
    ("m_devM", dict(m_dev="M+0", m_out=True)),
    ("m_devM+5", dict(m_dev="M+5", m_out=True)),
    ("a_neg_bias1_gate_R", dict(a_rows="neg", bias_mode=1, gate=True, R="sep", alpha=0.5)),
    ("all", dict(a_rows="neg", a_bound=True, c_rows=True, bias_mode=2, gate=True, R="sep", alpha=2.0, m_dev="M-1", m_out=True)),
]
BATCH_FIELDS = [                                                      # batch1 x batch2, every stride its own
    ("batch", dict(batch=(2, 3))),
    ("batch_wbcast", dict(batch=(3, 2), w_bcast=True)),
    ("batch_bias2", dict(batch=(2, 3), bias_mode=2, gate=True)),
    ("batch_bias1_R", dict(batch=(2, 2), bias_mode=1, R="sep")),
    ("batch_rows", dict(batch=(2, 3), a_rows="neg", a_bound=True, c_rows=True, m_dev="M-1", m_out=True)),
    ("batch_inplace", dict(batch=(3, 2), c_rows=True, R="alias", m_dev="M-1")),
]
LSE_FIELDS = [
    ("plain", {}),
    ("pick", dict(pick="edges")),
    ("alpha_half", dict(alpha=0.5, pick="random")),
    ("alpha2", dict(alpha=2.0, pick="edges")),
    ("a_rows", dict(a_rows="repeat", pick="edges")),
    ("a_rows_bound", dict(a_rows="repeat", a_bound=True, pick="edges")),
    ("m_dev0", dict(m_dev=0, m_out=True, pick="edges")),
    ("m_dev1", dict(m_dev=1, m_out=True, pick="edges")),
    ("m_devM-1", dict(m_dev="M-1", m_out=True, pick="edges")),
    ("m_devM", dict(m_dev="M+0", m_out=True, pick="edges")),
    ("m_devM+5", dict(m_dev="M+5", m_out=True, pick="edges")),
]
HEAVY = ("dma256", "split256p1", "split256p2", "split256p3")          # the big shapes carry a short list of field sets,
HEAVY_STORE = ("plain", "a_neg_bound", "bias1_gate", "all")
HEAVY_LSE = ("pick", "m_devM-1")
# ... and so do the other precisions of a kernel whose epilogue one precision already takes through the whole list
SHORT = ("reg64ns2", "reg64ns3", "reg64ns1", "reg128ns2", "reg128ns3", "reg128ns1", "split128p2", "split128p3")


def _route_with(opts, M, N, K, prec, lse, extra):
    """The route a field set turns a base case into: m_dev and a_rows without a bound change the dispatch."""
    spec = dict(name="x", route=None, M=M, N=N, K=K, precision=prec, flavour="lse" if lse else "store", **{**extra, **opts})
    return route(shape_desc(spec)[0])


def _build_cases():
    cases = []

    def add(name, rt, M, N, K, **kw):
        cases.append(dict(name=name, route=rt, M=M, N=N, K=K, **kw))

    for tag, rt, M, N, K, prec, extra in STORE_ROUTES:
        seed = f"store-{tag}"
        for fname, opts in STORE_FIELDS:
            if tag in HEAVY + SHORT and fname not in HEAVY_STORE:
                continue
            if tag in HEAVY and opts.get("m_dev") is not None:                              # m_dev leaves these routes: it has
                opts = {k: v for k, v in opts.items() if k not in ("m_dev", "m_out")}       # cases of its own below
            add(f"store-{tag}-{fname}", _route_with(opts, M, N, K, prec, False, extra), M, N, K, precision=prec, seed=seed,
                **{**extra, **opts})
        if tag == "sched":
            assert cases[-1]["route"] == "sched128" and CASE_ROUTE(cases, "store-sched-a_neg") == "reg128"    # both routes shown
        if tag not in HEAVY:
            add(f"store-{tag}-random", rt, M, N, K, precision=prec, data="random", seed=seed + "r", **extra)
            add(f"store-{tag}-random_all", None, M, N, K, precision=prec, data="random", seed=seed + "r",
                **{**extra, **dict(STORE_FIELDS)["all"]})
        if tag.startswith("split256"):
            add(f"store-{tag}-random", "split256", M, N, K, precision=prec, data="random", seed=seed + "r")
            add(f"store-{tag}-m_dev_falls_to_128", "split128", M, N, K, precision=prec, seed=seed, m_dev="M-1", m_out=True)
    # batches: the routes that take them (skinny and the split kernels do not; a batched precision-1..3 problem stays register-staged)
    for tag, M, N, K, prec in (("reg64", 70, 130, 36, 0), ("reg64ns3", 70, 130, 36, 2), ("reg128", 700, 650, 100, 0),
                               ("reg128ns1", 700, 650, 100, 3), ("sched", 700, 650, 256, 0), ("dma128", 700, 650, 544, 0),
                               ("skinnyshape", 70, 40, 512, 0), ("splitshape", 700, 650, 256, 1)):
        for fname, opts in BATCH_FIELDS:
            b = opts["batch"]
            if M == 700:
                opts = {**opts, "batch": (b[0] * 2, b[1] * 2)}         # 6 x 6 tiles of 128 per batch: >= 256 over the batches
            add(f"store-{tag}-{fname}", _route_with(opts, M, N, K, prec, False, {}), M, N, K, precision=prec, **opts)
    add("store-dma256-batch_bias2_R", "dma256", 257, 261, 128, batch=(16, 32), bias_mode=2, gate=True, R="sep", alpha=0.5,
        seed="store-dma256")
    add("store-dma256_mdev-leaves", "reg128", 257, 261, 128, batch=(16, 32), m_dev="M-1", m_out=True, seed="store-dma256")
    # the edges of the skinny route and of K
    add("store-skinny-N256", "skinny32", 70, 256, 512, bias_mode=1, gate=True)
    add("store-skinny-N257-leaves", "reg64", 70, 257, 512, bias_mode=1, gate=True)
    add("store-skinny-K1024-random", "skinny32", 300, 250, 1024, data="random")
    add("store-reg64-K4", "reg64", 70, 130, 4, bias_mode=1)
    add("store-reg64-K4-random", "reg64", 70, 130, 4, data="random")
    add("store-reg64-M1N1", "reg64", 1, 1, 8, bias_mode=2, R="sep")
    for tag, rt, M, N, K, prec, extra in LSE_ROUTES:
        seed = f"lse-{tag}"
        for fname, opts in LSE_FIELDS:
            if tag in HEAVY + SHORT and fname not in HEAVY_LSE:
                continue
            add(f"lse-{tag}-{fname}", _route_with(opts, M, N, K, prec, True, extra), M, N, K, precision=prec, flavour="lse", seed=seed,
                **{**extra, **opts})
        if tag == "sched":
            assert CASE_ROUTE(cases, "lse-sched-a_rows") == "dma128" and CASE_ROUTE(cases, "lse-sched-a_rows_bound") == "sched128"
        if tag not in HEAVY:
            add(f"lse-{tag}-random", rt, M, N, K, precision=prec, flavour="lse", data="random", alpha="unit", pick="random")
    # the part layout: an empty last part (N <= 64 mod 128), one column, and the pick at every part edge
    for N in (1, 5, 64, 65, 128, 129):
        add(f"lse-reg128-N{N}", "reg128", 130, N, 36, flavour="lse", pick="edges", alpha=0.5)
        add(f"lse-dma128-N{N}", "dma128", 130, N, 160, flavour="lse", pick="edges")
        add(f"lse-astat-N{N}", "astat128", 129, N, 64, flavour="lse", pick="edges", m_dev="M-1")
    add("lse-astat-M300", "astat128", 300, 700, 64, flavour="lse", pick="edges", a_rows="repeat")
    for c in cases:
        if c["route"] is None:
            c["route"] = route(shape_desc(c)[0])
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def CASE_ROUTE(cases, name):
    return [c["route"] for c in cases if c["name"] == name][0]


CASES = _build_cases()
CASE_BY_NAME = {c["name"]: c for c in CASES}
# tile_order: one exact case per route that walks tiles and per flavour; {0, 1, 2, 3, 6, 66} must give the bits of order 0
TILE_ORDERS = (0, 1, 2, 3, 6, 66)
TILE_ORDER_CASES = ["store-reg64-a_neg_bias1_gate_R", "store-reg64ns3-plain", "store-reg128-a_neg_bias1_gate_R", "store-reg128ns2-plain",
                    "store-sched-all", "store-dma128-a_neg_bias1_gate_R", "store-dma256-bias1_gate", "store-split128p1-all",
                    "store-split128p3-all", "store-split256p2-bias1_gate",
                    "lse-reg128-pick", "lse-reg128ns1-pick", "lse-sched-m_devM-1", "lse-dma128-pick", "lse-dma256-pick",
                    "lse-split128p2-pick", "lse-split256p1-pick"]


def flavour_of(c):
    return c.get("flavour", "store")
