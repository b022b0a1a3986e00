"""gnnlm_sample_topp at the descriptor level, against the float64 restatement of tests/topp_ref.py: the nucleus size exact, its mass
within the kernel's documented bound E, the id and next_logp exact.  Every row and p used here has a boundary margin >= 8 E and every
u sits at the midpoint of a CDF interval whose relative width is >= 1e-3 (tests/test_topp_ref_cpu.py checks both without a GPU), so no
case sits on a boundary and none is left out.  ld = V + 3 with the padding filled with NaN: a read beyond V shows up as a bad row.
GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import topp_ref as tp

pytestmark = pytest.mark.gpu

PAD, EOS = tp.PAD, tp.EOS
F32 = 2.0 ** -24                       # keep_mass is rounded to float32 once


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class Call:
    """One descriptor filled by hand over sentinel-filled outputs."""

    def __init__(self, dev, L, p, u, done=None, ld_pad=3, optional=True):
        from gnnlm_amd import _lib
        B, V = L.shape
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.lp = torch.full((B, V + ld_pad), float("nan"), device=dev)
        self.lp[:, :V] = t(np.asarray(L, np.float32))
        self.u = t(np.asarray(u, np.float32))
        self.nxt = torch.full((B,), -99, dtype=torch.int64, device=dev)
        self.nlp = torch.full((B,), 777.0, device=dev)
        self.n_keep = torch.full((B,), -5, dtype=torch.int32, device=dev)
        self.mass = torch.full((B,), -1.0, device=dev)
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        self.done = None if done is None else t(np.asarray(done, np.int32))
        s = self.s = _lib.gnnlm_sample_topp_t()
        s.logp, s.ld, s.B, s.V, s.topp, s.u = self.lp.data_ptr(), V + ld_pad, B, V, p, self.u.data_ptr()
        s.pad, s.eos, s.next = PAD, EOS, self.nxt.data_ptr()
        if optional:
            s.next_logp, s.n_keep, s.keep_mass, s.n_bad = self.nlp.data_ptr(), self.n_keep.data_ptr(), self.mass.data_ptr(), self.n_bad.data_ptr()
        if self.done is not None:
            s.done = self.done.data_ptr()

    def launch(self):
        from gnnlm_amd import _lib
        return _lib.lib().gnnlm_sample_topp(ctypes.byref(self.s), _lib.stream())

    def read(self):
        torch.cuda.synchronize()
        return dict(next=self.nxt.cpu().numpy(), logp=self.nlp.cpu().numpy(), n_keep=self.n_keep.cpu().numpy(), mass=self.mass.cpu().numpy(),
                    n_bad=int(self.n_bad.item()), done=None if self.done is None else self.done.cpu().numpy())

    def run(self):
        assert self.launch() == 0
        return self.read()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]) if a[k].dtype == np.float32 else a[k], bits(b[k]) if b[k].dtype == np.float32 else b[k])
               for k in ("next", "logp", "n_keep", "mass"))


def check_cases(dev, R, cases, E):
    """One call per p with every (row, u) of ``cases``; then every row again alone with another ld: the same bits."""
    for p in sorted({c["p"] for c in cases}):
        mine = [c for c in cases if c["p"] == p]
        rows = [c["row"] for c in mine]
        L = R[rows]
        got = Call(dev, L, p, [c["u"] for c in mine], done=np.zeros(len(mine))).run()
        assert got["n_bad"] == 0 and got["done"].tolist() == [int(c["member"] == EOS) for c in mine]
        assert got["n_keep"].tolist() == [c["n"] for c in mine]
        want_S = np.asarray([c["S"] for c in mine])
        assert (np.abs(got["mass"] - want_S) <= (E + F32) * want_S).all(), np.abs(got["mass"] / want_S - 1).max()
        assert got["next"].tolist() == [c["member"] for c in mine]
        assert np.array_equal(bits(got["logp"]), bits(L[np.arange(len(mine)), got["next"]]))
        for i, c in enumerate(mine):
            alone = Call(dev, L[i:i + 1], p, [c["u"]], ld_pad=i % 3).run()
            assert same_bits({k: v[i:i + 1] for k, v in got.items() if k in ("next", "logp", "n_keep", "mass")}, alone), (p, i)


@pytest.mark.parametrize("V", tp.SIZES + (tp.BIG_V,))
def test_sizes_nucleus_and_pick(dev, V):
    R = tp.big_rows() if V == tp.BIG_V else tp.rows_for(V)
    check_cases(dev, R, tp.cases_for(V), tp.E_of(V))


def test_the_last_digits_and_ties_at_the_threshold(dev):
    R, ps, tied = tp.last_digit_rows()
    for r in range(2):
        ids, n, S, margin = tp.nucleus(R[r], ps[r])
        assert margin >= 8 * tp.E
        members = ids.tolist()                           # every member is drawn: each holds >= 4 % of the nucleus
        us = [tp.member_mid(R[r], ps[r], m) for m in members]
        assert min(w for _, w in us) >= tp.MIN_WIDTH
        got = Call(dev, np.repeat(R[r:r + 1], n, 0), ps[r], [u for u, _ in us]).run()
        assert got["n_keep"].tolist() == [n] * n and got["next"].tolist() == members
        assert (np.abs(got["mass"] - S) <= (tp.E + F32) * S).all()
    assert n == 6 and members[1:] == tied[:5].tolist() and members[0] == 1      # five of the ten tied: the smallest ids


def test_the_ends_of_p(dev):
    for V in (65, 4097):
        R = tp.rows_for(V)
        n_pos = np.isfinite(R).sum(1)
        last = [int(np.nonzero(np.isfinite(r))[0][-1]) for r in R]
        for p in (1.5, float("inf")):
            got = Call(dev, R, p, np.full(len(R), 1.0 - 2.0 ** -24)).run()       # u next to 1: the last entry with mass, never a -inf
            assert got["n_keep"].tolist() == n_pos.tolist() and got["next"].tolist() == last
            want = np.asarray([tp.nucleus(r, p)[2] for r in R])
            assert (np.abs(got["mass"] - want) <= (tp.E + F32) * want).all()
        R2 = R.copy()
        R2[0, [V - 2, 5]] = R2[0].max()                  # equal maxima: the smallest id
        for u in (0.0, 0.5, 1.0 - 2.0 ** -24):
            got = Call(dev, R2, 1e-9, np.full(len(R), u)).run()
            assert got["n_keep"].tolist() == [1] * len(R)
            assert got["next"].tolist() == [int(tp.order(r)[0]) for r in R2] and got["next"][0] == min(5, int(R[0].argmax()))
            assert np.array_equal(bits(got["logp"]), bits(R2.max(1)))


def test_done_eos_and_bad_rows(dev):
    V = 65
    R = np.stack([tp.small_row(V, 900 + i) for i in range(7)])
    R[2, :] = -np.inf
    R[3, 17] = np.nan
    R[5, 64] = np.inf
    done = np.array([0, 1, 0, 0, 0, 0, 0], np.int32)
    u = np.full(7, 0.5, np.float32)
    u[0], w = tp.member_mid(R[0], 1.5, EOS)              # row 0 draws eos
    assert w >= tp.MIN_WIDTH
    col = {b: tp.pick(R[b], 1.5, 0.5) for b in (1, 4, 6)}
    for b in col:                                       # the neighbours' u are mid-interval too
        u[b], w = tp.member_mid(R[b], 1.5, col[b])
        assert w >= tp.MIN_WIDTH
    want, wcol, wdone, wbad, wn, _ = tp.sample_ref(R, 1.5, u, done=done)
    assert want[0] == EOS and wdone.tolist() == [1, 1, 1, 1, 0, 1, 0] and wbad == 3 and wcol[4] == col[4] and wcol[6] == col[6]
    got = Call(dev, R, 1.5, u, done=done).run()
    assert got["next"].tolist() == want.tolist() == [EOS, PAD, PAD, PAD, int(col[4]), PAD, int(col[6])]
    assert got["done"].tolist() == wdone.tolist() and got["n_bad"] == 3
    assert got["n_keep"][[0, 4, 6]].tolist() == [V, V, V] and (got["n_keep"][[1, 2, 3, 5]] == -5).all()
    assert (got["logp"][[1, 2, 3, 5]] == 777.0).all() and (got["mass"][[1, 2, 3, 5]] == -1.0).all()     # untouched
    assert np.array_equal(bits(got["logp"][[0, 4, 6]]), bits(R[[0, 4, 6], [EOS, col[4], col[6]]]))
    # without done and without the optional outputs
    c = Call(dev, R, 1.5, u, optional=False)
    got = c.run()
    assert got["next"].tolist() == [EOS, col[1], PAD, PAD, col[4], PAD, col[6]]
    assert (got["logp"] == 777.0).all() and (got["n_keep"] == -5).all() and got["n_bad"] == 0


def test_two_calls_and_a_captured_call_give_the_same_bits(dev):
    V = 4097
    R = tp.rows_for(V)
    cases = [c for c in tp.cases_for(V) if c["p"] == 0.79]
    L, u = R[[c["row"] for c in cases]], [c["u"] for c in cases]
    first, second = Call(dev, L, 0.79, u).run(), Call(dev, L, 0.79, u).run()
    assert same_bits(first, second) and first["next"].tolist() == [c["member"] for c in cases]
    c = Call(dev, L, 0.79, u)
    side = torch.cuda.Stream(device=dev)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        assert c.launch() == 0
    g.replay()
    assert same_bits(first, c.read())
    c.u.copy_(torch.flip(c.u, [0]))                      # new random numbers in the captured buffer
    g.replay()
    assert same_bits(Call(dev, L, 0.79, u[::-1]).run(), c.read())


def test_a_realistic_flat_row(dev):
    """Softmax of twice-unit-normal logits at V = 70,001 and p = 0.9: tens of thousands of members and a boundary margin below any bound.
    So n_keep is held between the restatement's n at p (1 - E) and at p (1 + E), and the id drawn must be a member of the larger."""
    row, p = tp.flat_row(), 0.9
    _, n_lo, S_lo, _ = tp.nucleus(row, p * (1 - tp.E))
    ids_hi, n_hi, S_hi, _ = tp.nucleus(row, p * (1 + tp.E))
    assert 10000 < n_lo <= n_hi
    u = (np.arange(16) + 0.5) / 16
    got = Call(dev, np.repeat(row[None], 16, 0), p, u).run()
    assert got["n_bad"] == 0 and len(set(got["n_keep"].tolist())) == 1 and n_lo <= got["n_keep"][0] <= n_hi
    assert np.isin(got["next"], ids_hi).all() and (np.diff(got["next"]) >= 0).all()
    assert (got["mass"] >= S_lo * (1 - tp.E - F32)).all() and (got["mass"] <= S_hi * (1 + tp.E + F32)).all()
    assert np.array_equal(bits(got["logp"]), bits(row[got["next"]]))


def test_refusals_leave_the_outputs_alone(dev):
    from gnnlm_amd import _lib, ops
    V = 65
    R = tp.rows_for(V)
    c = Call(dev, R, 0.5, np.full(len(R), 0.5), done=np.zeros(len(R)), ld_pad=3)
    s, L = c.s, _lib.lib()
    refused = [("topp", 0.0), ("topp", -1.0), ("topp", float("nan")), ("V", 0), ("V", (1 << 24) + 1), ("B", -1), ("ld", V - 1), ("logp", None),
               ("u", None), ("next", None), ("logp", c.lp.data_ptr() + 2), ("u", c.u.data_ptr() + 1), ("next", c.nxt.data_ptr() + 4),
               ("next_logp", c.nlp.data_ptr() + 2), ("done", c.done.data_ptr() + 2), ("n_bad", c.n_bad.data_ptr() + 2),
               ("n_keep", c.n_keep.data_ptr() + 2), ("keep_mass", c.mass.data_ptr() + 2)]
    for field, value in refused:
        old = getattr(s, field)
        if field == "V" and value > V:
            s.ld = value + 3
        setattr(s, field, value)
        assert L.gnnlm_sample_topp(ctypes.byref(s), _lib.stream()) == -22, (field, value)
        setattr(s, field, old)
        s.ld = V + 3
    assert L.gnnlm_sample_topp(None, _lib.stream()) == -22
    got = c.read()
    assert (got["next"] == -99).all() and (got["logp"] == 777.0).all() and (got["n_keep"] == -5).all() and (got["mass"] == -1.0).all()
    assert got["n_bad"] == 0 and not got["done"].any()
    s.B = 0
    assert c.launch() == 0 and (c.read()["next"] == -99).all()
    s.B = len(R)
    want = c.run()
    # the wrapper: the row stride is taken from the tensor
    n_keep = torch.zeros(len(R), dtype=torch.int32, device=dev)
    mass = torch.zeros(len(R), device=dev)
    nxt, nlp = ops.sample_topp(c.lp[:, :V], 0.5, c.u, n_keep=n_keep, keep_mass=mass)
    torch.cuda.synchronize()
    assert np.array_equal(nxt.cpu().numpy(), want["next"]) and np.array_equal(bits(nlp.cpu().numpy()), bits(want["logp"]))
    assert np.array_equal(n_keep.cpu().numpy(), want["n_keep"]) and np.array_equal(bits(mass.cpu().numpy()), bits(want["mass"]))
    assert want["n_keep"].tolist() == [tp.nucleus(r, 0.5)[1] for r in R]
    with pytest.raises(TypeError):
        ops.sample_topp(c.lp[:, :V].double(), 0.5, c.u)
    with pytest.raises(ValueError):
        ops.sample_topp(c.lp[:, :V], 0.5, None)
    with pytest.raises(ValueError):
        ops.sample_topp(c.lp[:, :V], 0.5, c.u[:2])
