"""gnnlm_beam_select at the descriptor level (include/gnnlm.h) against select_ref (tests/beam_ref.py), bit for bit, over whole runs of
steps 0 .. max_new: beam 1, 2, 5 and 32, beam_in 1 (the first step) and beam, N = 2 * beam and larger.  The candidates carry
integer-valued scores, so the float32 add is exact and the ties -- across hypotheses and across tokens -- are real; eos sits among the
first beam candidates and beyond them; one sentence is fed eos until its finalized slots fill, one so few candidates that hypotheses
die, and at the last step only eos is present.  After every step the whole state and the table of cache slots are compared, so a
finished sentence is seen to stay untouched.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import beam_ref as br

pytestmark = pytest.mark.gpu

V, B, MAX_NEW = 90, 3, 6
LENS = [3, 0, 5]
CAP = 5 + MAX_NEW                                    # sentence 2 reaches len == cap at the last step: its own entry is not written
LD_SRC = CAP + 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def candidates(rs, st, beam, beam_in, N, t, pad_cols=2):
    """Sorted rows as gnnlm_topk_merge leaves them (value descending, token ascending; absent entries last: -inf, id -1), with pad
    columns of NaN / garbage behind them.  Sentence 0: ordinary; sentence 1: eos-heavy; sentence 2: mostly absent."""
    val = np.full((B * beam_in, N + pad_cols), np.nan, np.float32)
    idx = np.full((B * beam_in, N + pad_cols), -99, np.int64)
    for b in range(B):
        for j in range(beam_in):
            pos = -1
            if t == MAX_NEW:
                present, toks = 1, np.asarray([br.EOS])
            else:
                present = N if b < 2 else int(rs.randint(0, 3))
                toks = rs.permutation(np.arange(4, V))[:present]
                p_eos = [0.15, 0.8, 0.0][b]
                if present and rs.rand() < p_eos:
                    pos = rs.randint(present)
                    toks[pos] = br.EOS
            vals = -rs.randint(0, 4, size=present).astype(np.float32)
            if b == 1 and pos >= 0:
                vals[pos] = 0.0                                                  # (among the best: the finalized slots fill)
            order = np.lexsort((toks, -vals))
            r = b * beam_in + j
            val[r, :N], idx[r, :N] = -np.inf, -1
            val[r, :present], idx[r, :present] = vals[order], toks[order]
            if present and b == 0 and rs.rand() < 0.2:
                val[r, present - 1] = np.nan                                     # NaN: absent as well
    return val, idx


class Device:
    """The state of tests/beam_ref.new_state on the device and a hand-filled descriptor over it."""

    def __init__(self, st, src, beam, dev):
        from gnnlm_amd import _lib
        self.dev, self.beam = dev, beam
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st.items()}
        self.src = torch.from_numpy(src.copy()).to(dev)
        d = _lib.gnnlm_beam_select_t()
        d.B, d.beam, d.eos, d.pad, d.max_new, d.cap = B, beam, br.EOS, br.PAD, MAX_NEW, CAP
        g = lambda k: self.t[k].data_ptr()
        d.score_in = d.score_out = g("score")
        d.t, d.finished, d.fin_n, d.len, d.done, d.next, d.parent = g("t"), g("finished"), g("fin_n"), g("len"), g("done"), g("next"), g("parent")
        d.hist_tok, d.hist_par, d.hist_score = g("hist_tok"), g("hist_par"), g("hist_score")
        d.fin_tok, d.fin_cum, d.fin_len, d.fin_score = g("fin_tok"), g("fin_cum"), g("fin_len"), g("fin_score")
        d.src_in = d.src_out = self.src.data_ptr()
        d.ld_src = LD_SRC
        self.desc = d

    def run(self, val, idx, beam_in, N=None):
        from gnnlm_amd import _lib
        self.val, self.idx = torch.from_numpy(val).to(self.dev), torch.from_numpy(idx).to(self.dev)
        d = self.desc
        d.cand_val, d.ld_val, d.cand_id, d.ld_id = self.val.data_ptr(), val.shape[1], self.idx.data_ptr(), idx.shape[1]
        d.beam_in, d.N = beam_in, val.shape[1] if N is None else N
        rc = _lib.lib().gnnlm_beam_select(ctypes.byref(d), _lib.stream())
        torch.cuda.synchronize()
        return rc

    def state(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}, self.src.cpu().numpy()


def same(got, want, what):
    for k in br.STATE_KEYS:
        assert np.array_equal(bits(got[0][k]), bits(want[0][k])), (what, k, got[0][k], want[0][k])
    assert np.array_equal(got[1], want[1]), (what, "table")


@pytest.mark.parametrize("extra", [0, 3], ids=["N=2beam", "N=2beam+3"])
@pytest.mark.parametrize("beam", [1, 2, 5, 32])
def test_runs_of_steps_against_select_ref(dev, beam, extra):
    rs = np.random.RandomState(7 * beam + extra)
    N = 2 * beam + extra
    st = br.new_state(B, beam, MAX_NEW, LENS, score0=[0.0, -2.0, 1.0])
    src = np.full((B * beam, LD_SRC), -5, np.int32)                             # the first step builds the table from nothing
    gpu = Device(st, src, beam, dev)
    seen = dict(fin_first=0, fin_late=0, dead=0, early=0, ties=0)
    for t in range(MAX_NEW + 1):
        beam_in = 1 if t == 0 else beam
        val, idx = candidates(rs, st, beam, beam_in, N, t)
        assert gpu.run(val, idx, beam_in, N) == 0
        before = st
        st, src = br.select_ref(val[:, :N], idx[:, :N], st, beam, beam_in, src=src[:, :CAP])
        src = np.concatenate([src, np.full((B * beam, LD_SRC - CAP), -5, np.int32)], 1)
        same(gpu.state(), (st, src), f"beam {beam} N {N} step {t}")
        live = (before["finished"] == 0)
        seen["fin_first"] += int((st["fin_n"] - before["fin_n"])[live].sum())
        seen["dead"] += int((~np.isfinite(st["score"][live & (st["finished"] == 0)])).sum()) if t < MAX_NEW else 0
        seen["early"] += int(((st["finished"] == 1) & live).sum()) if t < MAX_NEW else 0
        # what lm.step does between two selections: len += 1 for the slots that are not done
        adv = (st["done"] == 0).astype(np.int32)
        st["len"] = st["len"] + adv
        gpu.t["len"] += torch.from_numpy(adv).to(dev)
    assert st["finished"].all() and (st["t"] <= MAX_NEW + 1).all() and (st["fin_n"] >= 1).sum() >= 2
    print(f"beam {beam} N {N}: finalized {st['fin_n'].tolist()}, steps taken {st['t'].tolist()}, seen {seen}")
    assert seen["fin_first"] >= 2
    if beam >= 2:
        assert seen["dead"] > 0
    if beam <= 5:
        assert seen["early"] >= 1                                               # a sentence filled its finalized slots before the last step


def test_eos_beyond_the_first_beam_and_separate_outputs(dev):
    """One step at beam 2 with hand-made candidates: eos as the third candidate is not finalized and does not survive; the outputs may be
    buffers of their own (score_out, src_out)."""
    beam, N = 2, 4
    st = br.new_state(B, beam, MAX_NEW, LENS)
    st["t"][:], st["score"][:] = 1, [[-1.0, -1.0]] * B
    src = np.tile(((np.arange(B * beam, dtype=np.int32) + 1) % (B * beam))[:, None], (1, LD_SRC))      # (row s names slot s + 1)
    val = np.tile(np.asarray([[-1, -2, -3, -4], [-1, -3, -4, -5]], np.float32), (B, 1))
    idx = np.tile(np.asarray([[10, br.EOS, 12, 13], [9, 14, 15, 16]], np.int64), (B, 1))
    # order: (-2, j 0, 10), (-2, j 1, 9), (-3, j 0, eos), (-4, ..): eos is third -> ignored
    gpu = Device(st, src, beam, dev)
    score_out, src_out = torch.full((B, beam), 7.0, device=dev), gpu.src.clone()
    gpu.desc.score_out, gpu.desc.src_out = score_out.data_ptr(), src_out.data_ptr()
    assert gpu.run(val, idx, beam) == 0
    want, tab = br.select_ref(val, idx, st, beam, beam, src=src[:, :CAP])
    got, src_after = gpu.state()
    assert np.array_equal(src_after, src) and np.array_equal(got["score"], st["score"])          # the inputs are left alone
    assert want["fin_n"].tolist() == [0] * B and want["next"].tolist() == [10, 9] * B
    for k in br.STATE_KEYS:
        if k != "score":
            assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(bits(score_out.cpu().numpy()), bits(want["score"]))
    assert np.array_equal(src_out.cpu().numpy()[:, :CAP], tab) and np.array_equal(src_out.cpu().numpy()[:, CAP:], src[:, CAP:])
    assert not np.array_equal(tab, src[:, :CAP])


def test_refusals(dev):
    from gnnlm_amd import _lib
    beam, N = 5, 10
    st = br.new_state(B, beam, MAX_NEW, LENS)
    src = np.full((B * beam, LD_SRC), -5, np.int32)
    rs = np.random.RandomState(3)
    val, idx = candidates(rs, st, beam, beam, N, 1, pad_cols=0)

    def check(edit, match, beam_in=beam):
        gpu = Device(st, src, beam, dev)
        gpu.val, gpu.idx = torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev)
        d = gpu.desc
        d.cand_val, d.ld_val, d.cand_id, d.ld_id, d.beam_in, d.N = gpu.val.data_ptr(), N, gpu.idx.data_ptr(), N, beam_in, N
        edit(d)
        assert _lib.lib().gnnlm_beam_select(ctypes.byref(d), _lib.stream()) == -22, match
        assert match in _lib.lib().gnnlm_last_error().decode(), (match, _lib.lib().gnnlm_last_error().decode())
        torch.cuda.synchronize()
        same(gpu.state(), (st, src), match)                                       # nothing was touched

    set_ = lambda **kw: (lambda d: [setattr(d, k, v) for k, v in kw.items()])
    check(set_(beam=0), "beam outside")
    check(set_(beam=33), "beam outside")
    check(set_(N=9), "N < 2 * beam")
    check(set_(beam_in=2), "beam_in")
    check(set_(beam=32, beam_in=32, N=257), "8192")
    check(set_(ld_val=N - 1), "ld_val")
    check(set_(ld_id=N - 1), "ld_val")
    check(set_(max_new=-1), "max_new")
    check(set_(ld_src=CAP - 1), "ld_src")
    check(set_(cap=-1), "cap")
    check(set_(src_in=None), "src_in")
    for field in ("cand_val", "cand_id", "score_in", "score_out", "t", "finished", "len", "done", "next", "parent"):
        check(set_(**{field: None}), "missing")
    for field in ("hist_tok", "hist_par", "hist_score", "fin_n", "fin_tok", "fin_cum", "fin_len", "fin_score"):
        check(set_(**{field: None}), "hist_* / fin_* missing")
    check(lambda d: setattr(d, "next", d.next + 4), "misaligned")
    check(lambda d: setattr(d, "t", d.t + 2), "misaligned")
    assert _lib.lib().gnnlm_beam_select(None, _lib.stream()) == -22
    # without a table, and B = 0
    gpu = Device(st, src, beam, dev)
    gpu.desc.src_in = gpu.desc.src_out = None
    assert gpu.run(val, idx, beam) == 0
    want, _ = br.select_ref(val, idx, st, beam, beam)
    same(gpu.state(), (want, src), "no table")
    gpu = Device(st, src, beam, dev)
    gpu.desc.B = 0
    assert gpu.run(val, idx, beam) == 0
    same(gpu.state(), (st, src), "B = 0")


def test_ops_wrapper(dev):
    """ops.beam_select over a BeamState gives what the hand-filled descriptor gives."""
    from gnnlm_amd import ops
    from gnnlm_amd.beam_search import BeamState
    beam, N = 5, 13
    rs = np.random.RandomState(11)
    st = br.new_state(B, beam, MAX_NEW, LENS, score0=[0.5, 0.0, -1.0])
    val, idx = candidates(rs, st, beam, 1, N, 0, pad_cols=0)
    lens, done = torch.from_numpy(st["len"]).to(dev), torch.zeros(B * beam, dtype=torch.int32, device=dev)
    state = BeamState(B, beam, MAX_NEW, lens, done, dev, score0=[0.5, 0.0, -1.0])
    table = torch.full((B * beam, CAP), -5, dtype=torch.int32, device=dev)
    nxt, parent = ops.beam_select(torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev), state, src=table, eos=br.EOS, pad=br.PAD)
    want, tab = br.select_ref(val, idx, st, beam, 1, src=np.full((B * beam, CAP), -5, np.int32))
    got = {k: getattr(state, k).cpu().numpy() for k in br.STATE_KEYS}
    same((got, table.cpu().numpy()), (want, tab), "ops.beam_select")
    assert nxt is state.next and parent is state.parent
    with pytest.raises(TypeError):
        ops.beam_select(torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev).int(), state, src=table)
    with pytest.raises(ValueError):
        ops.beam_select(torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev), state, src=table[:B])
