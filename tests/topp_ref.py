"""gnnlm_sample_topp restated in float64 numpy (tests only; imports neither the package under test nor the reference), and the
generators of every input row the GPU tests use, so that tests/test_topp_ref_cpu.py can check them without a GPU.

  is_bad(lp)          a NaN, a +inf or no finite entry
  order(lp)           larger value first, then smaller id
  nucleus(lp, p)      -> (member ids ascending, n, S, margin)
  pick(lp, p, u)      -> the id drawn
  sample_ref(...)     whole calls: done, bad rows, eos
  member_mid(...)     the u at the middle of a member's CDF interval, and that interval's relative width

``margin``: how far p is, relatively, from the two prefix sums on either side of the nucleus boundary -- min |p - c| / c over c =
c_{n-2} (the last sum below p) and c_{n-1} (the first one not below it, where there is one).  The kernel's sums are within a
relative ``E`` of the exact ones (include/gnnlm.h, csrc/sample_topp.hip), so a row with margin > E has the same n on the device.
"""
import functools

import numpy as np

PAD, EOS = 1, 2
E = 2.0 ** -21 + 2.0 ** -22          # the kernel's bound E(V) = 2^-21 + 2^(2 ceil(log2 V) - 62) at V = 2^20; smaller below
MIN_WIDTH = 1e-3                     # tests/test_sample_abi_gpu.py's, and its reasoning
CHUNK = 256                          # the kernel's chunks of consecutive ids start at multiples of 256 counted from the 16-byte
EDGE_IDS = (252, 253, 254, 255, 256)  # aligned address at or below the row: 256 - off, off in 0 .. 3.  These ids straddle it


def E_of(V):
    return 2.0 ** -21 + 2.0 ** (2 * int(np.ceil(np.log2(max(V, 1)))) - 62)


def is_bad(lp):
    lp = np.asarray(lp)
    return bool(np.isnan(lp).any() or np.isposinf(lp).any() or not np.isfinite(lp).any())


def masses(lp):
    lp = np.asarray(lp, np.float64)
    with np.errstate(over="ignore"):
        return np.where(np.isfinite(lp), np.exp(np.where(np.isfinite(lp), lp, 0.0)), 0.0)


def order(lp):
    lp = np.asarray(lp, np.float64)
    return np.lexsort((np.arange(lp.size), -(lp + 0.0)))


def nucleus(lp, p):
    """-> (member ids ascending int64, n, S, margin) of a row that is not bad."""
    lp = np.asarray(lp)
    o = order(lp)
    m = masses(lp)[o]
    c = np.cumsum(m)
    n_pos = int(np.isfinite(lp).sum())
    below = int((c[:n_pos] < p).sum())
    n = min(n_pos, 1 + below)
    near = []
    if below >= 1:
        near.append(c[below - 1])            # the last sum below p
    if below < n_pos:
        near.append(c[below])                # the first sum not below p
    margin = min(abs(p - x) / x for x in near) if np.isfinite(p) else np.inf
    return np.sort(o[:n]).astype(np.int64), n, float(c[n - 1]), float(margin)


def pick(lp, p, u):
    ids, n, S, _ = nucleus(lp, p)
    m = masses(lp)[ids]
    c = np.cumsum(m)
    hit = np.nonzero(c > np.float64(u) * c[-1])[0]
    return int(ids[hit[0]]) if hit.size else int(ids[np.nonzero(m > 0)[0][-1]])


def member_mid(lp, p, member):
    """-> (u at the midpoint of ``member``'s CDF interval in the ascending-id walk of the nucleus, the interval's relative width)."""
    ids, _, _, _ = nucleus(lp, p)
    m = masses(lp)[ids]
    c = np.cumsum(m)
    i = int(np.nonzero(ids == member)[0][0])
    lo = c[i - 1] if i else 0.0
    return float((lo + c[i]) / (2 * c[-1])), float((c[i] - lo) / c[-1])


def chosen_members(lp, p, edges=None):
    """The members the GPU tests draw: the smallest id, the largest, one in the middle (the member nearest to the middle id), and those
    on either side of every place the first chunk edge can be (the largest member below and the smallest member at or above each of
    253 .. 256)."""
    ids, n, _, _ = nucleus(lp, p)
    want = {int(ids[0]), int(ids[-1]), int(ids[np.abs(ids - np.asarray(lp).size // 2).argmin()])}
    for edge in (EDGE_IDS[1:] if edges is None else edges):
        lo, hi = ids[ids < edge], ids[ids >= edge]
        if lo.size and hi.size:
            want |= {int(lo[-1]), int(hi[0])}
    return sorted(want)


def sample_ref(L, p, u, pad=PAD, eos=EOS, done=None):
    """Whole calls.  L [B, V], u [B] -> (next int64 [B], picked column or -1 [B], done int32 [B], n_bad, n_keep [B], keep_mass [B]);
    -1 / 0 / 0 where the kernel leaves its outputs alone."""
    B = L.shape[0]
    done = np.zeros(B, np.int32) if done is None else np.asarray(done, np.int32).copy()
    nxt, col = np.full(B, pad, np.int64), np.full(B, -1, np.int64)
    n_keep, mass, n_bad = np.zeros(B, np.int64), np.zeros(B), 0
    for b in range(B):
        if done[b]:
            continue
        if is_bad(L[b]):
            done[b], n_bad = 1, n_bad + 1
            continue
        _, n_keep[b], mass[b], _ = nucleus(L[b], p)
        col[b] = nxt[b] = pick(L[b], p, u[b])
        if nxt[b] == eos:
            done[b] = 1
    return nxt, col, done, n_bad, n_keep, mass


# ------------------------------------------------------------------------------------------------ the rows of the GPU tests
SIZES = (1, 2, 63, 64, 65, 257, 4097, 70001)
PS = (0.3, 0.5, 0.79)


def _log(m):
    with np.errstate(divide="ignore"):
        return np.log(m).astype(np.float32)


def heavy_row(V, seed, n_heavy=40, heavy_mass=0.8, holes=False, shift=0.0, edge_ids=EDGE_IDS):
    """``n_heavy`` heavy ids scattered over a light tail.  The heaviest sit at 0, V - 1, V // 2 and on the chunk-edge ids, so that they
    are members at every p >= 0.3 and each holds >= 1e-3 of any nucleus; all heavy masses differ.  ``holes``: every tenth tail id is
    -inf.  ``shift`` is subtracted from every log-prob: the row then sums to exp(-shift)."""
    rs = np.random.RandomState(seed)
    need = [i for i in dict.fromkeys((0, V - 1, V // 2) + tuple(edge_ids)) if 0 <= i < V]
    rest = np.setdiff1d(np.arange(V), need)
    heavy = np.concatenate([need, rs.choice(rest, n_heavy - len(need), replace=False)]).astype(np.int64)
    w = 1.6 - 0.02 * np.arange(n_heavy) + 0.015 * rs.rand(n_heavy)
    m = np.zeros(V)
    m[heavy] = heavy_mass * w / w.sum()
    tail = np.setdiff1d(np.arange(V), heavy)
    t = np.exp(0.5 * rs.randn(tail.size))
    if holes:
        t[::10] = 0.0
    m[tail] = (1.0 - heavy_mass) * t / t.sum()
    return (_log(m) - np.float32(shift)).astype(np.float32)


def zipf_row(V, seed, s=1.3, edge_ids=EDGE_IDS):
    """Softmax of Zipf-like logits: mass of rank r proportional to r^-s, the first ranks on the ids heavy_row puts its heaviest on."""
    rs = np.random.RandomState(seed)
    need = [i for i in dict.fromkeys((0, V - 1, V // 2) + tuple(edge_ids)) if 0 <= i < V]
    rest = np.setdiff1d(np.arange(V), need)
    ids = np.concatenate([need, rs.permutation(rest)]).astype(np.int64)
    m = np.zeros(V)
    m[ids] = np.arange(1, V + 1, dtype=np.float64) ** -s
    return _log(m / m.sum())


def small_row(V, seed, holes=False, shift=0.0):
    """Uniform logits in [-1, 1): every entry of a row of <= 65 holds well over 1e-3 of it."""
    rs = np.random.RandomState(seed)
    z = rs.rand(V) * 2.0 - 1.0
    lp = z - np.log(np.exp(z).sum())
    if holes and V > 2:
        lp[rs.choice(V, max(1, V // 8), replace=False)] = -np.inf
    return (lp - shift).astype(np.float32)


def rows_for(V):
    """The four or five rows of size V, [R, V] float32, with different profiles."""
    if V <= 65:
        rows = [small_row(V, 100 + V), small_row(V, 200 + V, shift=0.25), small_row(V, 300 + V, holes=True), small_row(V, 400 + V)]
    else:
        rows = [heavy_row(V, 500 + V), heavy_row(V, 600 + V, shift=0.25), heavy_row(V, 700 + V, holes=True), zipf_row(V, 800 + V),
                heavy_row(V, 900 + V, n_heavy=24, heavy_mass=0.85)]
    return np.stack(rows)


BIG_V = 600001                       # more than 2048 chunks of 256: the kernel's chunks are 512 ids there, edges at 512 - off
BIG_EDGE_IDS = EDGE_IDS + (508, 509, 510, 511, 512)
BIG_P = 0.5


def big_rows():
    return np.stack([heavy_row(BIG_V, 31, edge_ids=BIG_EDGE_IDS), zipf_row(BIG_V, 32, edge_ids=BIG_EDGE_IDS)])


def _cases(R, ps, edges=None):
    out = []
    for r in range(R.shape[0]):
        for p in ps:
            ids, n, S, margin = nucleus(R[r], p)
            m = masses(R[r])[ids]
            c = np.cumsum(m)
            for member in chosen_members(R[r], p, edges):
                i = int(np.nonzero(ids == member)[0][0])
                lo = c[i - 1] if i else 0.0
                out.append(dict(row=r, p=p, member=member, u=float((lo + c[i]) / (2 * c[-1])), width=float((c[i] - lo) / c[-1]),
                                n=n, S=S, margin=margin))
    return out


@functools.lru_cache(maxsize=None)
def cases_for(V):
    """Every draw the size test makes at size V: dicts of row, p, member (the id that must come out), u, the CDF interval's relative
    width, and the row's n, S and margin at that p.  Computed once and shared."""
    if V == BIG_V:
        return tuple(_cases(big_rows(), (BIG_P,), BIG_EDGE_IDS[1:5] + BIG_EDGE_IDS[6:]))
    return tuple(_cases(rows_for(V), PS))


def last_digit_rows(V=300, seed=5):
    """[2, V] and the p of each.  Row 0: a head of 12 consecutive float32 numbers (they differ in the last mantissa bits only), each with
    about 0.06 of the mass, scattered; the boundary at p = 0.4 falls among them and is decided by the last radix digit.  Row 1: ten
    entries with EXACTLY the same value at the threshold, of which p admits fewer than are tied."""
    rs = np.random.RandomState(seed)
    tail = np.exp(0.3 * rs.randn(V))
    a = 0.25 * tail / tail.sum()
    head = rs.choice(V, 12, replace=False)
    base = np.float32(np.log(0.0625))
    vals = base + np.arange(12) * np.spacing(base)              # consecutive float32 numbers upward from log(0.0625)
    assert np.unique(vals.astype(np.float32)).size == 12
    lp0 = _log(a)
    lp0[head] = vals.astype(np.float32)[rs.permutation(12)]
    b = 0.3 * tail / tail.sum()
    lp1 = _log(b)
    tied = np.sort(rs.choice(np.arange(3, V), 10, replace=False))
    lp1[tied] = np.float32(np.log(0.05))
    lp1[1] = np.float32(np.log(0.2))
    return np.stack([lp0, lp1]), (0.4, 0.43), tied


def flat_row(V=70001, seed=11):
    """Softmax of twice-unit-normal logits: the nucleus at 0.9 is tens of thousands of entries and its boundary margin below any bound."""
    z = 2.0 * np.random.RandomState(seed).randn(V)
    return (z - np.log(np.exp(z).sum())).astype(np.float32)
