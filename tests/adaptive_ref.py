"""numpy restatement of gnnlm_adaptive_target_logp (include/gnnlm.h: gnnlm_adaptive_softmax_t), of the kernels its GEMMs and
reductions reach (through gemm_ref.route), a derived per-row error bound, and the case table of tests/test_adaptive_abi_gpu.py.
No torch, no device code.  oracle/adaptive_softmax.target_log_prob is the arithmetic; here it is spelled the way the call works, so
that a wrong step of the call can be restated as a wrong reference (``mutate``, used by test_adaptive_ref_cpu.py):

  compact(case)      band_split: head_pick per row (-1 for a target outside [0, vocab)), and per tail band the compacted (row, pick)
                     list, rows in ascending order
  adaptive_ref(case) head: picked - lse over [E_0 ; class_proj] for every valid row, -inf for the others; per tail band and per list
                     entry lm_logp[row] += picked - lse of (x[row] . proj_t^T) . emb^T.  float64; operands rounded as
                     gnnlm_gemm_t.precision says (gemm_ref.planes); the projection is a float32 tensor in memory and is rounded
                     again at precisions 1..3 as an operand of the band GEMM.  Returns the whole lm_logp image (every one of the n
                     floats is written: no byte of it stays), the float64 values and the bound.
  routes(case)       the kernel of every GEMM of the call and of every lse_reduce
  bound(case)        see below

The bound, per valid row (BAR and LSE_BAR are the bars of test_gemm_abi_gpu.py, restated here and pinned by the CPU test):
  a picked logit     BAR[precision] * (sum |a||b| + 1)                          (the GEMM's bar on one element)
  a log-sum-exp      LSE_BAR
  band 0 row         one of each, over the head.
  tail row           two of each (head: the class logit; band: the word), and the projection's error carried through the band:
      the projection xi[j] the device holds differs from the reference's by at most
          delta[j] = BAR * (sum_k |x[k]||proj_t[j, k]| + 1) + 2^-24 |xi[j]|     (the GEMM's bar + the reference's own float32 rounding)
      the band GEMM multiplies the operand planes of xi, so the value it sees moves by delta'[j]:
          precision 0, 2:  delta' = delta          (the planes add up to the float32 value)
          precision 1:     delta' = delta + 2^-17 |xi[j]|   (two bf16 planes, both rounded to nearest, represent a value to 2^-18
                                                             of it; two different values: twice that)
          precision 3:     rounding to half is monotone, so the device's half lies between half(xi - delta) and half(xi + delta):
                           delta' = the larger distance of those two from half(xi) -- 0 unless a rounding boundary lies within
                           delta of xi, one half-precision ulp where it does
      every band logit c then moves by at most D[c] = sum_j delta'[j] |e[c, j]| (1 + 2^-10) (the factor: |rounded e| <= that), the
      picked logit by D[t] and the log-sum-exp by at most max_c D[c] (it is 1-Lipschitz in the maximum norm): picked - lse by at
      most 2 max_c D[c].
  the float32 epilogue  picked - lse, and the sum of the head and tail terms: three roundings, each 2^-24 of a value no larger
      than |picked| + |lse| of the head plus that of the band: 3 * 2^-24 * (|picked_h| + |lse_h| + |picked_t| + |lse_t|).
A row outside the vocabulary has no bound: it is -inf exactly."""
import zlib

import numpy as np

import gemm_ref

BAR = {0: 5e-7, 1: 4e-5, 2: 5e-7, 3: 5e-7}       # test_gemm_abi_gpu.py: BAR, LSE_BAR
LSE_BAR = 2e-5
BS_WAVES = 16                                    # rowops.hip: band_split_kernel takes rows in chunks of 64 * BS_WAVES
CHUNK = 64 * BS_WAVES
REDUCE4_MIN_PARTS = 1024                         # gemm_f32.hip: lse_reduce() launches the four-wave kernel from this many parts on
HEAD_ORDER_MIN_N = 1024                          # adaptive_logp.hip: adaptive_impl sets tile_order = 2 + 4 on the head from this many rows on
HEAD_TILE_ORDER = 6
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
OOR_TARGETS = ("-1", "V", "V+1", 2 ** 31, 2 ** 32 + 3, INT64_MIN, INT64_MAX)

MUTATIONS = ("shift_picks", "no_carry", "gt_cutoff", "no_class", "tail_assigned", "one_part_fewer", "no_max", "no_reround_p3",
             "clamp_oor")

cdiv = gemm_ref.cdiv


def n_parts(N):
    return 2 * cdiv(N, 128)


# ------------------------------------------------------------------------------------------ band_split
def compact(case, mutate=None):
    """-> (head_pick [n] int64, -1 where the target is outside the vocabulary; [(rows, picks)] per tail band).  Mutations: 'gt_cutoff'
    (t > cutoff), 'clamp_oor', 'shift_picks' (every list entry takes the next entry's pick), 'no_carry' (the slot of a row counts
    only the rows of its own 1024-row chunk: later chunks overwrite the list from slot 0, the count is still the total)."""
    t = case["target"].astype(np.int64)
    cut = np.asarray(case["cutoff"], dtype=np.int64)
    nb, V = len(cut), int(cut[-1])
    if mutate == "clamp_oor":
        t = np.clip(t, 0, V - 1)
    ok = (t >= 0) & (t < V)
    band = np.searchsorted(cut[:-1], t, side="left" if mutate == "gt_cutoff" else "right")      # cutoffs <= t (< t: the mutation)
    head_pick = np.where(ok, np.where(band == 0, t, cut[0] + band - 1), -1)
    lists = []
    for b in range(1, nb):
        rows = np.nonzero(ok & (band == b))[0]
        picks = t[rows] - cut[b - 1]
        if mutate == "shift_picks" and len(rows):
            picks = np.roll(picks, -1)
        if mutate == "no_carry" and len(rows):
            slot_rows = np.full(len(rows), -1, dtype=np.int64)
            slot_picks = np.zeros(len(rows), dtype=np.int64)
            for c in range(0, len(t), CHUNK):
                sel = (rows >= c) & (rows < c + CHUNK)
                k = int(sel.sum())
                slot_rows[:k], slot_picks[:k] = rows[sel], picks[sel]
            keep = slot_rows >= 0                                       # a slot nobody wrote holds a stale entry: left out here
            rows, picks = slot_rows[keep], slot_picks[keep]
        lists.append((rows, picks))
    return head_pick, lists


# ------------------------------------------------------------------------------------------ one GEMM + log-sum-exp epilogue + reduce
def _planes64(x, precision):
    return [p.astype(np.float64) for p in gemm_ref.planes(x, precision)]


def _logits(pa, pw, precision):
    out = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j in gemm_ref.PRODUCTS[precision]:
            t = pa[i] @ pw[j].T
            out = t if out is None else out + t
    return out


def lse_pick(A, W, pick, precision, a_planes=None, mutate=None, shift=None):
    """Rows of A against W [N, K]: -> (picked, lse, S_pick, max_c shift @ |W|^T) per row, float64.  A pick outside [0, N) gives NaN
    (the device leaves the value it found).  Mutations: 'one_part_fewer' (the last 64-column part is not reduced), 'no_max' (the sum
    of exp(x) is taken in float32 without the maximum)."""
    m, N = A.shape[0], W.shape[0]
    pw = _planes64(W, precision)
    absW = np.abs(W).astype(np.float64)
    picked, lse, S, D = np.full(m, np.nan), np.full(m, np.nan), np.zeros(m), np.zeros(m)
    okp = (pick >= 0) & (pick < N)
    cols = (n_parts(N) - 1) * 64 if mutate == "one_part_fewer" else N
    step = max(1, min(256, (1 << 24) // max(N, 1)))
    for r0 in range(0, m, step):
        r1 = min(m, r0 + step)
        pa = _planes64(A[r0:r1], precision) if a_planes is None else [p[r0:r1].astype(np.float64) for p in a_planes]
        x = _logits(pa, pw, precision)
        ok = okp[r0:r1]
        idx = np.nonzero(ok)[0]
        picked[r0:r1][ok] = x[idx, pick[r0:r1][ok]]
        S[r0:r1][ok] = (np.abs(A[r0:r1][idx]).astype(np.float64) * absW[pick[r0:r1][ok]]).sum(-1)
        xs = x[:, :cols]
        if mutate == "no_max":
            with np.errstate(over="ignore", divide="ignore"):
                lse[r0:r1] = np.log(np.exp(xs.astype(np.float32)).sum(-1, dtype=np.float32).astype(np.float64))
        else:
            mx = xs.max(-1)
            with np.errstate(invalid="ignore", divide="ignore"):
                lse[r0:r1] = mx + np.log(np.exp(xs - mx[:, None]).sum(-1))
        if shift is not None:
            D[r0:r1] = (shift[r0:r1] @ absW.T).max(-1) * (1.0 + 2.0 ** -10)
    return picked, lse, S, D


def _reround_shift(xi32, delta, precision):
    """delta' of the module docstring: how far the value the band GEMM sees can move when xi moves by delta"""
    a = np.abs(xi32).astype(np.float64)
    if precision in (0, 2):
        return delta
    if precision == 1:
        return delta + 2.0 ** -17 * a
    half = lambda v: v.astype(np.float32).astype(np.float16).astype(np.float64)
    with np.errstate(over="ignore"):
        v = xi32.astype(np.float64)
        h = half(v)
        return np.maximum(np.abs(half(v - delta) - h), np.abs(half(v + delta) - h))


# ------------------------------------------------------------------------------------------ the call
def adaptive_ref(case, mutate=None):
    """-> dict: logp (float64 [n], -inf for a row outside the vocabulary), image (float32: lm_logp after the call), valid (mask),
    bound (float64 [n], per valid row; 0 elsewhere), band (per row, -1 outside the vocabulary)."""
    assert mutate in (None,) + MUTATIONS
    n, prec = case["n"], case["precision"]
    cut = list(case["cutoff"])
    nb = len(cut)
    x = case["x"]
    out, bnd = np.full(n, -np.inf), np.zeros(n)
    band_of = np.full(n, -1)
    if n == 0:
        return dict(logp=out, image=out.astype(np.float32), valid=np.zeros(0, dtype=bool), bound=bnd, band=band_of)
    head_pick, lists = compact(case, mutate if mutate in ("gt_cutoff", "clamp_oor", "shift_picks", "no_carry") else None)
    valid = head_pick >= 0
    rows = np.nonzero(valid)[0]
    gm = mutate if mutate in ("one_part_fewer", "no_max") else None
    ph, lh, Sh, _ = lse_pick(x[rows], case["head_w"], head_pick[rows], prec, mutate=gm)
    band_of[rows] = np.where(head_pick[rows] < cut[0], 0, head_pick[rows] - cut[0] + 1)
    if mutate == "no_class":
        ph = np.where(band_of[rows] > 0, 0.0, ph)
    out[rows] = ph - lh
    mag = np.zeros(n)
    mag[rows] = np.abs(ph) + np.abs(lh)
    bnd[rows] = BAR[prec] * (Sh + 1.0) + LSE_BAR
    for b in range(1, nb):
        br, bp = lists[b - 1]
        if not len(br):
            continue
        P, E = case["proj_t"][b], case["emb"][b]
        xb = x[br]
        xi = _logits(_planes64(xb, prec), _planes64(P, prec), prec)
        with np.errstate(over="ignore"):
            xi32 = xi.astype(np.float32)
        delta = BAR[prec] * (np.abs(xb).astype(np.float64) @ np.abs(P).astype(np.float64).T + 1.0) + 2.0 ** -24 * np.abs(xi)
        shift = _reround_shift(xi32, delta, prec)
        a_planes = [xi32] if (mutate == "no_reround_p3" and prec == 3) else None
        pt, lt, St, D = lse_pick(xi32, E, bp, prec, a_planes=a_planes, mutate=gm, shift=shift)
        term = pt - lt
        if mutate == "tail_assigned":
            out[br] = term
        else:
            np.add.at(out, br, term)
        np.add.at(bnd, br, BAR[prec] * (St + 1.0) + LSE_BAR + 2.0 * D)
        np.add.at(mag, br, np.abs(pt) + np.abs(lt))
    bnd += 3.0 * 2.0 ** -24 * np.where(np.isfinite(mag), mag, 0.0)
    bnd[~valid] = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        image = out.astype(np.float32)
    return dict(logp=out, image=image, valid=valid, bound=bnd, band=band_of)


_REF = {}


def case_ref(case):
    """adaptive_ref(case) of a case of the table, kept for the next test of the same case"""
    if case["name"] not in _REF:
        _REF.clear()
        _REF[case["name"]] = adaptive_ref(case)
    return _REF[case["name"]]


def bound(case):
    return case_ref(case)["bound"]


def outside(got, want, bnd, valid):
    """rows where ``got`` leaves the bound around ``want`` (a NaN, or an infinity the reference does not have, leaves it)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - want) <= bnd)
    bad[~valid] = ~(np.isneginf(got[~valid]))
    same_inf = valid & np.isinf(want) & (got == want)
    bad[same_inf] = False
    return np.nonzero(bad)[0]


# ------------------------------------------------------------------------------------------ the dispatch
def gemm_descs(case):
    """The descriptors adaptive_impl fills, as far as gemm_ref.route() reads them: 'head', ('proj', b), ('band', b)"""
    n, d, prec, cut, dim = case["n"], case["d"], case["precision"], case["cutoff"], case["dim"]
    nb = len(cut)
    base = dict(gemm_ref.DESC_DEFAULTS, A=True, W=True, M=n, precision=prec)
    out = {"head": dict(base, N=cut[0] + nb - 1, K=d, lda=d + 4, ldw=d, lse=True,
                        tile_order=HEAD_TILE_ORDER if n >= HEAD_ORDER_MIN_N else 0)}
    for b in range(1, nb):
        out[("proj", b)] = dict(base, N=dim[b], K=d, lda=d + 4, ldw=d, C=True, ldc=dim[b], a_rows=True, m_dev=0)
        out[("band", b)] = dict(base, N=cut[b] - cut[b - 1], K=dim[b], lda=dim[b], ldw=dim[b], lse=True, m_dev=0)
    return out


def routes(case):
    """-> dict: head, proj [per tail band], band [per tail band]: gemm_ref.route() of each GEMM (n = 0: nothing is launched);
    reduce: the lse_reduce kernel of the head and of every band, 1 (one wave per row) or 4 (four waves)"""
    if case["n"] == 0:
        return dict(head="none", proj=[], band=[], reduce=[])
    g = gemm_descs(case)
    nb = len(case["cutoff"])
    red = lambda desc: 4 if n_parts(desc["N"]) >= REDUCE4_MIN_PARTS else 1
    return dict(head=gemm_ref.route(g["head"]), proj=[gemm_ref.route(g[("proj", b)]) for b in range(1, nb)],
                band=[gemm_ref.route(g[("band", b)]) for b in range(1, nb)],
                reduce=[red(g["head"])] + [red(g[("band", b)]) for b in range(1, nb)])


def head_tile_order(case):
    return gemm_descs(case)["head"]["tile_order"]


# ------------------------------------------------------------------------------------------ the case table
def _targets(pattern, n, cut, rs):
    """Target patterns of the compaction cases.  Band b of a row is drawn first, the word inside it at random."""
    nb, V = len(cut), cut[-1]
    lo = [0] + list(cut[:-1])
    r = np.arange(n)
    t = None
    if pattern == "uniform":
        band = rs.randint(0, nb, n)
    elif pattern.startswith("all"):                               # every row in band b: all other bands have count 0
        band = np.full(n, int(pattern[3:]))
    elif pattern == "row0":                                       # band 1 holds only row 0 (the last band only row n - 1)
        band = np.zeros(n, dtype=int)
        band[0] = 1 % nb
    elif pattern == "rowlast":
        band = np.zeros(n, dtype=int)
        band[n - 1] = nb - 1
    elif pattern == "mod":
        band = r % nb
    elif pattern == "late":                                       # the last band's rows all lie at r >= 1024: the carry across chunks
        band = np.where(r >= CHUNK, np.where(r % 3 == 0, nb - 1, r % max(nb - 1, 1)), r % max(nb - 1, 1))
    elif pattern == "wave":                                       # band 1's rows fill exactly the second wave of the second chunk
        band = np.where((r >= CHUNK + 64) & (r < CHUNK + 128), 1, np.where(r % 2 == 0, 0, nb - 1))
    elif pattern == "chunk":                                      # band 1's rows fill exactly the second chunk
        band = np.where((r >= CHUNK) & (r < 2 * CHUNK), 1, np.where(r % 2 == 0, 0, nb - 1))
    elif pattern == "edges":                                      # 0, cutoff[b] - 1, cutoff[b], V - 1 for every b
        vals = sorted({0, V - 1} | {c - 1 for c in cut} | {c for c in cut[:-1]})
        t = np.array([vals[(i + i // CHUNK) % len(vals)] for i in range(n)], dtype=np.int64)
    else:
        raise KeyError(pattern)
    if t is None:
        band = np.asarray(band) % nb
        lo_, hi_ = np.asarray(lo)[band], np.asarray(cut)[band]
        t = (lo_ + (rs.randint(0, 1 << 30, n) % (hi_ - lo_))).astype(np.int64)
    return t


def _oor_value(v, V):
    return {"-1": -1, "V": V, "V+1": V + 1}.get(v, v)


def make_case(spec):
    """The case of a spec of the table, data included (deterministic per name).
    Data: weight rows of norm sqrt(3.5) (projection rows: 1) and x entries of size sqrt(3.5): every head logit, projected entry and
    band logit is a sum of independent terms with a standard deviation of 3.5 (sqrt(3.5) for the projection), so head and band
    logits span roughly +-10.  Rows with r % 4 == 1 are then moved by 25 towards their target (the word's row of E_0; for a tail word
    proj_t^T e and the class row of the head), rows with r % 4 == 3 by 25 away from it: the target is the arg-max on many of the
    former and 20 to 30 nats below it on most of the latter.  Every row keeps noise of its own, so no two rows are equal.
    ``special``: row 2 is all zero (-log N in closed form) and rows 5 / 6 are scaled until the target's band / head logit is +90."""
    s = dict(precision=0, pattern="uniform", special=False, oor=False, push=True)
    s.update(spec)
    rs = np.random.RandomState(zlib.crc32(s["name"].encode()) & 0x7FFFFFFF)
    n, d, cut, dim, prec = s["n"], s["d"], list(s["cut"]), [0] + list(s["dim"]), s["precision"]
    nb = len(cut)
    assert len(dim) == nb and all(c2 > c1 for c1, c2 in zip(cut, cut[1:]))
    sizes = [cut[0]] + [cut[b] - cut[b - 1] for b in range(1, nb)]
    sd = 3.5                                                      # the logits' standard deviation

    def rows_of_norm(m, k, norm):
        w = rs.standard_normal((m, k)).astype(np.float32)
        return (w * (norm / np.sqrt(k))).astype(np.float32)

    head_w = rows_of_norm(cut[0] + nb - 1, d, np.sqrt(sd))       # x entries of size sqrt(sd): logits of deviation sd
    proj_t = [None] + [rows_of_norm(dim[b], d, 1.0) for b in range(1, nb)]       # xi entries of size sqrt(sd) again
    emb = [None] + [rows_of_norm(sizes[b], dim[b], np.sqrt(sd)) for b in range(1, nb)]
    x = (rs.standard_normal((n, d)) * np.sqrt(sd)).astype(np.float32)
    target = _targets(s["pattern"], n, cut, rs) if n else np.zeros(0, dtype=np.int64)
    case = dict(name=s["name"], n=n, d=d, cutoff=cut, dim=dim, precision=prec, head_w=head_w, proj_t=proj_t, emb=emb, spec=s)
    band = np.searchsorted(np.asarray(cut[:-1]), target, side="right")
    if s["push"] and n:
        # the direction of x that raises the target's own logit: the word's row of E_0, or proj_t^T e for a tail word
        dirs = np.empty((n, d), dtype=np.float64)
        for b in range(nb):
            m = band == b
            if m.any():
                w = head_w[target[m]] if b == 0 else emb[b][target[m] - cut[b - 1]].astype(np.float64) @ proj_t[b].astype(np.float64)
                dirs[m] = w
        gain = (dirs * dirs).sum(-1)                              # the logit one unit of the direction adds
        sign = np.where(np.arange(n) % 4 == 1, 1.0, np.where(np.arange(n) % 4 == 3, -1.0, 0.0))
        push = (sign * 25.0 / np.maximum(gain, 1e-6))[:, None] * dirs
        tail = band > 0                                           # a tail row's class logit in the head goes the same way
        cls = head_w[np.minimum(cut[0] + np.maximum(band, 1) - 1, len(head_w) - 1)].astype(np.float64)
        push += np.where(tail, sign * 25.0 / (cls * cls).sum(-1), 0.0)[:, None] * cls
        x = (x + push).astype(np.float32)
    if s["special"]:
        assert n > 6
        x[2] = 0.0
        for r in (5, 6):                                          # scaled until the target's logit is +90 (float64 arithmetic)
            b = band[r]
            xr = x[r].astype(np.float64)
            if b == 0:
                lg = xr @ head_w[target[r]].astype(np.float64)
            else:
                lg = (proj_t[b].astype(np.float64) @ xr) @ emb[b][target[r] - cut[b - 1]].astype(np.float64)
            assert abs(lg) > 1e-3
            x[r] = (xr * (90.0 / lg)).astype(np.float32)
    if s["oor"]:                                                  # the targets outside the vocabulary, mixed among valid rows
        pos = [(3 + 9 * i) % n for i in range(len(OOR_TARGETS))] + ([n - 1, CHUNK, CHUNK + 65] if n > CHUNK + 65 else [n - 1])
        vals = [_oor_value(v, cut[-1]) for v in OOR_TARGETS]
        for i, p in enumerate(pos):
            target[p] = vals[i % len(vals)]
        case["oor_rows"] = sorted(set(pos))
    case["x"], case["target"] = x, target
    return case


def _spec(name, n, d=16, cut=(40, 100, 150), dim=None, **kw):
    dim = tuple(dim) if dim is not None else (16,) * (len(cut) - 1)
    return dict(name=name, n=n, d=d, cut=tuple(cut), dim=dim, **kw)


CUTS = {1: (90,), 2: (40, 100), 3: (40, 100, 150), 8: (40, 100, 150, 151, 200, 330, 331, 400)}
NS = (1, 63, 64, 65, 1023, 1024, 1025, 2085, 3073)
BIG = (2050, 1990)                                                # 17 x 16 tiles of 128 (gemm_ref.BIG)


def _build():
    c = []
    # compaction: every n at three bands; the other band counts at the sizes around a wave, a chunk and two chunks
    for n in NS:
        c.append(_spec(f"cmp-n{n}-b3-uniform", n))
    for nb in (1, 2, 8):
        for n in (1, 65, 1025, 2085):
            c.append(_spec(f"cmp-n{n}-b{nb}-uniform", n, cut=CUTS[nb]))
    for nb in (3, 8):
        pats = [f"all{b}" for b in range(nb)] + ["row0", "rowlast", "mod", "late", "wave", "chunk", "edges"]
        for p in pats:
            c.append(_spec(f"cmp-n2085-b{nb}-{p}", 2085, cut=CUTS[nb], pattern=p))
    c.append(_spec("cmp-n3073-b2-late", 3073, cut=CUTS[2], pattern="late"))
    c.append(_spec("cmp-n1-b3-all2", 1, pattern="all2"))
    # shapes of a band
    c.append(_spec("shape-one-word-band", 70, cut=(40, 41, 100), pattern="mod"))
    c.append(_spec("shape-head-below-64", 70, cut=(20, 50, 90), pattern="mod"))                   # 22 head logits: part 1 is (-inf, 0)
    c.append(_spec("shape-last-part-empty", 70, cut=(156, 286, 320), pattern="mod"))              # 158 head logits, a band of 130
    c.append(_spec("shape-band-65409", 40, cut=(40, 100, 100 + 65409), pattern="mod", expect=dict(reduce=[1, 1, 4])))
    c.append(_spec("shape-band-65409-p3", 40, cut=(40, 100 + 65409), pattern="mod", precision=3, expect=dict(reduce=[1, 4])))
    c.append(_spec("shape-band-65408", 40, cut=(40, 40 + 65408), pattern="mod", expect=dict(reduce=[1, 1])))
    c.append(_spec("shape-dim64", 300, cut=(40, 100, 800), dim=(16, 64), pattern="mod", expect=dict(band=["reg128", "astat128"])))
    c.append(_spec("shape-dims-differ", 130, cut=(40, 100, 150, 230), dim=(8, 32, 16), pattern="mod"))
    # routes of the head (no m_dev): reg128 is every small case above
    c.append(_spec("head-astat128", 129, d=64, cut=(298, 360, 420), pattern="mod", expect=dict(head="astat128")))
    c.append(_spec("head-dma128", 130, d=128, cut=(298, 360, 420), pattern="mod", expect=dict(head="dma128")))
    c.append(_spec("head-sched128", BIG[0], d=256, cut=(BIG[1] - 2, 2050, 2100), pattern="mod", expect=dict(head="sched128")))
    c.append(_spec("head-dma256", 2049, d=128, cut=(58198, 58260, 58300), pattern="mod", push=False, expect=dict(head="dma256")))
    for p in (1, 2, 3):
        c.append(_spec(f"head-split128-p{p}", BIG[0], d=256, cut=(BIG[1] - 2, 2050, 2100), pattern="mod", precision=p,
                       expect=dict(head="split128")))
        c.append(_spec(f"head-split256-p{p}", 5900, d=256, cut=(5899, 5960), pattern="mod", precision=p, push=False,
                       expect=dict(head="split256")))
        c.append(_spec(f"head-reg128-p{p}", 130, d=100, cut=(298, 360, 420), pattern="mod", precision=p, expect=dict(head="reg128")))
    # routes of a band (m_dev) and of the gathered projection
    c.append(_spec("band-dma128", 130, cut=(40, 340), dim=(128,), pattern="mod", expect=dict(band=["dma128"], proj=["reg64"])))
    c.append(_spec("band-sched128", BIG[0], d=32, cut=(40, 40 + BIG[1]), dim=(256,), pattern="mod",
                   expect=dict(band=["sched128"], proj=["reg64"])))
    for p in (1, 2, 3):
        c.append(_spec(f"band-split128-p{p}", BIG[0], d=32, cut=(40, 40 + BIG[1]), dim=(256,), pattern="mod", precision=p,
                       expect=dict(band=["split128"], proj=["reg64"])))
        c.append(_spec(f"band-reg128-p{p}", 130, cut=(40, 100, 400), dim=(16, 36), pattern="mod", precision=p,
                       expect=dict(band=["reg128", "reg128"])))
    c.append(_spec("proj-skinny32", 70, d=512, cut=(40, 100, 150), dim=(256, 64), pattern="mod",
                   expect=dict(proj=["skinny32", "skinny32"], band=["dma128", "astat128"])))
    c.append(_spec("proj-reg128", BIG[0], cut=(40, 80), dim=(1924,), pattern="mod", expect=dict(proj=["reg128"], band=["reg128"])))
    # numerics and the edges of the contract, at every precision
    for p in (0, 1, 2, 3):
        c.append(_spec(f"num-p{p}", 130, cut=(40, 100, 290), dim=(16, 32), pattern="mod", precision=p, special=True))
        c.append(_spec(f"oor-p{p}", 70, pattern="uniform", precision=p, oor=True))
    c.append(_spec("oor-n1100", 1100, pattern="uniform", oor=True))
    c.append(_spec("oor-n70-b1", 70, cut=CUTS[1], oor=True))
    assert len({s["name"] for s in c}) == len(c)
    return c


SPECS = _build()
SPEC_BY_NAME = {s["name"]: s for s in SPECS}
CASES = [s["name"] for s in SPECS]

# Routes gemm_ref.route() can return for a GEMM of this call that no case reaches, and why:
LEFT_OUT = {
    ("band", "split256"): "under m_dev the plane kernel takes 256 x 256 tiles only from M >= 2^17 rows on (SPLIT_MDEV_BIG_M): 131072 "
                          "rows against a band of 1024 or more words at dim 256 is no few-second case",
    ("band", "dma256"): "the dispatcher gives 256 x 256 LDS-DMA tiles only to a problem without m_dev: no band GEMM can reach it",
    ("proj", "split128"): "a projection at precisions 1..3 with d >= 256 and 256 or more 128 x 128 tiles needs n x dim >= 4M outputs "
                          "and a band GEMM over that dim behind it; the route itself is held by test_gemm_abi_gpu.py with m_dev and a_rows",
}


def case_by_name(name):
    return make_case(SPEC_BY_NAME[name])
