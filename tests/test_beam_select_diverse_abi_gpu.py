"""gnnlm_beam_select_diverse at the descriptor level (include/gnnlm.h) against select_diverse_ref (tests/diverse_beam_ref.py), bit for
bit: every state buffer and the table of cache slots after every step.  The candidates are small integers / 8 and the penalties
multiples of 1 / 8, so every float32 operation is exact and the ties -- inside a group after the penalty, across hypotheses, across
tokens -- are real.  Groups 1 / rate 0 is compared with gnnlm_beam_select itself on copies of the same buffers.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

import beam_ref as br
import diverse_beam_ref as db

pytestmark = pytest.mark.gpu

MAX_NEW = 5
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


class Device:
    """The state of tests/beam_ref.new_state on the device and a hand-filled gnnlm_beam_select_diverse_t over it."""

    def __init__(self, st, src, beam, dev, max_new=MAX_NEW, cap=None):
        from gnnlm_amd import _lib
        self.dev, self.beam = dev, beam
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in st.items()}
        self.src = torch.from_numpy(src.copy()).to(dev)
        self.dd = _lib.gnnlm_beam_select_diverse_t()
        d = self.dd.sel
        d.B, d.beam, d.eos, d.pad, d.max_new = len(st["t"]), beam, br.EOS, br.PAD, max_new
        d.cap = src.shape[1] if cap is None else cap
        g = lambda k: self.t[k].data_ptr()
        d.score_in = d.score_out = g("score")
        d.t, d.finished, d.fin_n, d.len, d.done, d.next, d.parent = g("t"), g("finished"), g("fin_n"), g("len"), g("done"), g("next"), g("parent")
        d.hist_tok, d.hist_par, d.hist_score = g("hist_tok"), g("hist_par"), g("hist_score")
        d.fin_tok, d.fin_cum, d.fin_len, d.fin_score = g("fin_tok"), g("fin_cum"), g("fin_len"), g("fin_score")
        d.src_in = d.src_out = self.src.data_ptr()
        d.ld_src = src.shape[1]

    def feed(self, val, idx, beam_in, N=None):
        self.val, self.idx = torch.from_numpy(np.ascontiguousarray(val)).to(self.dev), torch.from_numpy(np.ascontiguousarray(idx)).to(self.dev)
        d = self.dd.sel
        d.cand_val, d.ld_val, d.cand_id, d.ld_id = self.val.data_ptr(), val.shape[1], self.idx.data_ptr(), idx.shape[1]
        d.beam_in, d.N = beam_in, val.shape[1] if N is None else N

    def run(self, val, idx, beam_in, N=None, groups=1, strength=0.0, rate=0.0, plain=False):
        from gnnlm_amd import _lib
        self.feed(val, idx, beam_in, N)
        self.dd.groups, self.dd.strength, self.dd.rate = groups, strength, rate
        if plain:
            rc = _lib.lib().gnnlm_beam_select(ctypes.byref(self.dd.sel), _lib.stream())
        else:
            rc = _lib.lib().gnnlm_beam_select_diverse(ctypes.byref(self.dd), _lib.stream())
        torch.cuda.synchronize()
        return rc

    def state(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}, self.src.cpu().numpy()


def same(got, want, what):
    for k in br.STATE_KEYS:
        assert np.array_equal(bits(got[0][k]), bits(want[0][k])), (what, k, got[0][k], want[0][k])
    assert np.array_equal(got[1], want[1]), (what, "table")


def candidates(rs, B, beam_in, N, t, max_new=MAX_NEW, vocab=None, pad_cols=2, sparse=None, p_eos=(0.2, 0.7, 0.0)):
    """Sorted rows as gnnlm_topk_merge leaves them (value descending, token ascending; absent entries last: -inf, id -1) with pad
    columns of NaN / garbage behind them.  Values are -k / 8; the tokens come from a vocabulary barely larger than a row, so the rows
    of a sentence share most of theirs.  Sentence ``sparse`` has 0 .. 2 candidates per row; at the last step only eos is present."""
    vocab = N + 6 if vocab is None else vocab
    val = np.full((B * beam_in, N + pad_cols), np.nan, np.float32)
    idx = np.full((B * beam_in, N + pad_cols), -99, np.int64)
    for b in range(B):
        for j in range(beam_in):
            if t == max_new:
                present, toks = 1, np.asarray([br.EOS])
            else:
                present = int(rs.randint(0, 3)) if b == sparse else N
                toks = rs.permutation(np.arange(4, 4 + vocab))[:present]
                if present and rs.rand() < p_eos[b % len(p_eos)]:
                    toks[rs.randint(min(present, 3))] = br.EOS
            vals = -rs.randint(0, 12, size=present).astype(np.float32) / 8
            order = np.lexsort((toks, -vals))
            r = b * beam_in + j
            val[r, :N], idx[r, :N] = -np.inf, -1
            val[r, :present], idx[r, :present] = vals[order], toks[order]
    return val, idx


def run_steps(dev, B, beam, N, lens, seed, groups=1, strength=0.0, rate=0.0, sparse=None, against_plain=False, steps=MAX_NEW + 1):
    """Steps 0 .. of one run, the whole state compared after each -> what was seen on the way."""
    rs = np.random.RandomState(seed)
    cap = max(lens) + MAX_NEW
    ld = cap + 3
    st = br.new_state(B, beam, MAX_NEW, lens, score0=[0.0, -2.0, 1.0][:B])
    src = np.full((B * beam, ld), -5, np.int32)
    gpu = Device(st, src, beam, dev, cap=cap)
    twin = Device(st, src, beam, dev, cap=cap) if against_plain else None
    seen = dict(fin=0, dead=0, early=0, penalised=0)
    for t in range(steps):
        beam_in = 1 if t == 0 else beam
        val, idx = candidates(rs, B, beam_in, N, t, sparse=sparse)
        assert gpu.run(val, idx, beam_in, N, groups, strength, rate) == 0
        before = st
        st, tab = db.select_diverse_ref(val[:, :N], idx[:, :N], st, beam, beam_in, groups, strength, rate, src=src[:, :cap])
        src = np.concatenate([tab, np.full((B * beam, ld - cap), -5, np.int32)], 1)
        same(gpu.state(), (st, src), f"beam {beam} groups {groups} N {N} step {t}")
        if twin is not None:
            assert twin.run(val, idx, beam_in, N, plain=True) == 0
            same(gpu.state(), twin.state(), f"beam {beam} step {t}: gnnlm_beam_select")
        live = before["finished"] == 0
        plain, _ = br.select_ref(val[:, :N], idx[:, :N], before, beam, beam_in)
        seen["penalised"] += int(not np.array_equal(plain["next"], st["next"]))
        seen["fin"] += int((st["fin_n"] - before["fin_n"])[live].sum())
        seen["dead"] += int((~np.isfinite(st["score"][live & (st["finished"] == 0)])).sum()) if t < MAX_NEW else 0
        seen["early"] += int(((st["finished"] == 1) & live).sum()) if t < MAX_NEW else 0
        adv = (st["done"] == 0).astype(np.int32)             # what lm.step does between two selections
        st["len"] = st["len"] + adv
        gpu.t["len"] += torch.from_numpy(adv).to(dev)
        if twin is not None:
            twin.t["len"] += torch.from_numpy(adv).to(dev)
    return st, seen


# ---------------------------------------------------------------------------------------------------- 1. groups 1 / rate 0 is the plain entry
@pytest.mark.parametrize("beam,extra", [(1, 0), (5, 3), (32, 0)])
def test_one_group_without_a_rate_is_gnnlm_beam_select(dev, beam, extra):
    """beam_in = 1 at step 0, beam_in = beam afterwards; every buffer equal to gnnlm_beam_select's on copies, and to the restatement."""
    st, seen = run_steps(dev, 3, beam, 2 * beam + extra, [3, 0, 5], 11 * beam + extra, sparse=2, against_plain=True)
    assert st["finished"].all() and seen["fin"] >= 2 and seen["penalised"] == 0


# ---------------------------------------------------------------------------------------------------- 2. runs of steps under groups
@pytest.mark.parametrize("beam,groups,strength", [(4, 2, 0.5), (6, 3, 1.0), (4, 4, 0.5), (4, 2, 0.0), (6, 2, 0.375)])
def test_runs_of_steps_against_the_restatement(dev, beam, groups, strength):
    st, seen = run_steps(dev, 3, beam, 2 * beam, [3, 0, 5], 100 * beam + groups, groups=groups, strength=strength, sparse=2)
    print(f"beam {beam} groups {groups} strength {strength}: finalized {st['fin_n'].tolist()}, steps {st['t'].tolist()}, seen {seen}")
    assert st["finished"].all() and seen["fin"] >= 2 and seen["dead"] > 0
    assert seen["penalised"] >= 3                            # the groups' steps differ from plain beam search's


def test_the_largest_shape(dev):
    """beam 32 / groups 4, N = 64: beam_in * N = 2048 candidates, 64 places, 64 chosen tokens -- the bounds of the LDS layout."""
    st, seen = run_steps(dev, 2, 32, 64, [4, 1], 5, groups=4, strength=0.25, steps=3)
    assert seen["penalised"] >= 2 and (st["t"] == 3).all()
    st, seen = run_steps(dev, 2, 32, 64, [4, 1], 6, rate=0.125, steps=3)
    assert seen["penalised"] >= 1


# ---------------------------------------------------------------------------------------------------- 3. by hand
def one_step(dev, val, idx, st, beam, beam_in, max_new=3, **kw):
    """One launch on hand-made arrays -> the device's state, checked against the restatement's."""
    B = len(st["t"])
    src = np.tile(((np.arange(B * beam, dtype=np.int32) + 1) % (B * beam))[:, None], (1, 8))
    gpu = Device(st, src, beam, dev, max_new=max_new)
    assert gpu.run(val, idx, beam_in, **kw) == 0
    want = db.select_diverse_ref(val, idx, st, beam, beam_in, kw.get("groups", 1), kw.get("strength", 0.0), kw.get("rate", 0.0), src=src)
    got = gpu.state()
    same(got, want, str(kw))
    return got[0]


def hand_state(beam, score, B=1, t=1, max_new=3):
    st = br.new_state(B, beam, max_new, [5] * B)
    st["t"][:], st["score"][:] = t, score
    return st


HAND_VAL = np.tile(-np.arange(8, dtype=np.float32) / 8, (4, 1))
HAND_IDX = np.asarray([[7, 10, 11, 12, 13, 14, 15, 16], [7, 20, 21, 22, 23, 24, 25, 26], [7, 30, 31, 32, 33, 34, 35, 36],
                       [40, 41, 42, 43, 44, 45, 46, 47]], np.int64)


def test_penalty_interleave_and_a_token_chosen_twice(dev):
    beam = 4
    st = hand_state(beam, [-1.0, -1.0, -2.0, -2.0])
    # group 0 = hypotheses 0, 2 chooses (0, 7), (0, 10), (0, 11), (0, 12); group 1 = hypotheses 1, 3 pays 0.5 for token 7
    out = one_step(dev, HAND_VAL, HAND_IDX, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 20, 10, 21] and out["parent"].tolist() == [0, 1, 0, 1] and out["score"][0].tolist() == [-1.0, -1.125, -1.125, -1.25]
    out = one_step(dev, HAND_VAL, HAND_IDX, st, beam, beam, N=8, groups=2, strength=0.0, max_new=3)
    assert out["next"].tolist() == [7, 7, 10, 20] and out["score"][0].tolist() == [-1.0, -1.0, -1.125, -1.125]
    # group 0 chooses token 7 twice, (0, 7) and (2, 7): group 1's (1, 7) costs 2 * 0.5 and falls behind (1, 20) .. (1, 23)
    st2 = hand_state(beam, [-1.0, -1.0, -1.0, -2.0])
    out = one_step(dev, HAND_VAL, HAND_IDX, st2, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 20, 7, 21] and out["parent"].tolist() == [0, 1, 2, 1]
    # .. and with 2 * 0.0625 it stays in front, at -1.125, tied with (1, 20): the tie goes to the smaller token
    out = one_step(dev, HAND_VAL, HAND_IDX, st2, beam, beam, N=8, groups=2, strength=0.0625, max_new=3)
    assert out["next"].tolist() == [7, 7, 7, 20] and out["score"][0].tolist() == [-1.0, -1.125, -1.0, -1.125]


def test_a_tie_inside_a_group_after_the_penalty(dev):
    """Group 1 = hypotheses 1 and 3 hold the same token at the same value once hypothesis 1 has paid: hypothesis order, then token order."""
    beam = 4
    st = hand_state(beam, [0.0, -1.0, -9.0, -1.5])
    val = np.tile(-np.arange(8, dtype=np.float32) / 8, (beam, 1))
    idx = np.asarray([[7, 10, 11, 12, 13, 14, 15, 16], [7, 9, 21, 22, 23, 24, 25, 26], [50, 51, 52, 53, 54, 55, 56, 57],
                      [7, 8, 42, 43, 44, 45, 46, 47]], np.int64)
    # group 0 chooses token 7 once.  group 1: (1, 7) = -1 - 0.5 = -1.5 and (3, 7) = -1.5 - 0.5 = -2; (1, 9) = -1.125, (1, 21) = -1.25,
    # (1, 22) = -1.375, then (1, 7) = -1.5 = (1, 23): the same hypothesis, token 7 first; group 1 takes 4: 9, 21, 22, 7
    out = one_step(dev, val, idx, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 9, 10, 21]
    # the same token and value in two hypotheses of a group: (1, 7) and (3, 7) at -1.5 with hypothesis 3 at -1.0 -- hypothesis 1 first
    st["score"][0] = [0.0, -1.0, -9.0, -1.0]
    idx[1, 1:4], idx[3, 1:4] = [60, 61, 62], [70, 71, 72]
    val2 = val.copy()
    val2[1, 1:], val2[3, 1:] = -2.0 - np.arange(7) / 8, -2.0 - np.arange(7) / 8
    out = one_step(dev, val2, idx, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 7, 10, 7] and out["parent"].tolist() == [0, 1, 0, 3] and out["score"][0].tolist() == [0.0, -1.5, -0.125, -1.5]


def test_an_eos_first_in_group_0_shifts_the_survivors(dev):
    beam = 4
    st = hand_state(beam, [-1.0, -1.0, -2.0, -2.0])
    st["hist_tok"][0, 0], st["hist_par"][0, 0], st["hist_score"][0, 0] = [15, 16, 17, 18], [0, 0, 0, 0], [-1.0, -1.0, -2.0, -2.0]
    idx = HAND_IDX.copy()
    idx[0, 0] = br.EOS
    out = one_step(dev, HAND_VAL, idx, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["fin_n"][0] == 1 and out["fin_tok"][0, 0, :2].tolist() == [15, br.EOS] and out["fin_score"][0, 0] == -1.0
    # the list: eos, (1, 7), (0, 10), (1, 20), (0, 11), ..: hypothesis 0 of the next step continues group 1's candidate
    assert out["next"].tolist() == [7, 10, 20, 11] and out["parent"].tolist() == [1, 0, 1, 0]
    # an eos at a place >= beam is neither finalized nor a survivor
    idx = HAND_IDX.copy()
    idx[0, 2] = br.EOS                                       # group 0's third candidate: place 4
    out = one_step(dev, HAND_VAL, idx, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["fin_n"][0] == 0 and out["next"].tolist() == [7, 20, 10, 21]


def test_a_finished_sentence_and_one_at_the_last_step_among_live_ones(dev):
    beam, B, max_new = 4, 3, 3
    st = hand_state(beam, [[-1.0, -1.0, -2.0, -2.0]] * B, B=B)
    st["finished"][0] = 1                                    # untouched
    st["t"][2] = max_new                                     # forced to finish: the host has left only eos
    val, idx = np.tile(HAND_VAL, (B, 1)), np.tile(HAND_IDX, (B, 1))
    val[2 * beam:, 1:], idx[2 * beam:, 0], idx[2 * beam:, 1:] = -np.inf, br.EOS, -1
    out = one_step(dev, val, idx, st, beam, beam, N=8, groups=2, strength=0.5, max_new=max_new)
    assert out["t"].tolist() == [1, 2, max_new + 1] and out["finished"].tolist() == [1, 0, 1]
    assert out["fin_n"].tolist() == [0, 0, 4] and out["done"].reshape(B, beam).all(1).tolist() == [False, False, True]
    assert out["next"][beam:2 * beam].tolist() == [7, 20, 10, 21] and (out["next"][:beam] == br.PAD).all()


def test_absent_candidates_and_dead_slots(dev):
    beam = 4
    st = hand_state(beam, [-1.0, -np.inf, -2.0, -2.0])       # hypothesis 1 is dead: group 1 has hypothesis 3 only
    val = HAND_VAL.copy()
    val[:, 1] = -np.inf                                      # a column absent in every row
    val[3, 3:] = -np.inf                                     # hypothesis 3: two candidates in all -> group 1 chooses 2 of its 4
    out = one_step(dev, val, HAND_IDX, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    # group 0: (0, 7) -1, (0, 11) -1.25, (0, 12) -1.375, (0, 13) -1.5; group 1: (3, 40) -2, (3, 42) -2.25, then nothing: places 5, 7 empty
    assert out["next"].tolist() == [7, 40, 11, 42] and out["parent"].tolist() == [0, 3, 0, 3]
    val[3] = -np.inf                                         # group 1 has nothing: places 1, 3, 5, 7 are empty, group 0's four survive
    out = one_step(dev, val, HAND_IDX, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 11, 12, 13] and out["parent"].tolist() == [0, 0, 0, 0]
    val[0, 4:] = -np.inf                                     # and group 0 only three (hypothesis 2 adds its own): a dead slot comes out
    val[2] = -np.inf
    out = one_step(dev, val, HAND_IDX, st, beam, beam, N=8, groups=2, strength=0.5, max_new=3)
    assert out["next"].tolist() == [7, 11, 12, br.PAD] and out["parent"].tolist() == [0, 0, 0, 3] and out["score"][0, 3] == -np.inf


# ---------------------------------------------------------------------------------------------------- 4. siblings
def test_siblings_by_hand_and_where_the_rate_does_not_act(dev):
    st = hand_state(3, [0.0, -0.25, -3.0])
    val = np.tile(-np.arange(6, dtype=np.float32) / 8, (3, 1))
    idx = np.asarray([[10, 11, 12, 13, 14, 15], [20, 21, 22, 23, 24, 25], [30, 31, 32, 33, 34, 35]], np.int64)
    # hypothesis 0: 0 - 0.25, -0.125 - 0.5, -0.25 - 0.75, ..; hypothesis 1: -0.25 - 0.25, -0.375 - 0.5, ..
    out = one_step(dev, val, idx, st, 3, 3, N=6, rate=0.25, max_new=3)
    assert out["next"].tolist() == [10, 20, 11] and out["parent"].tolist() == [0, 1, 0] and out["score"][0].tolist() == [-0.25, -0.5, -0.625]
    # unsorted rows and equal values in a row: the rank is the row's own order (value, then token), wherever the candidates stand
    val2, idx2 = val.copy(), idx.copy()
    val2[0, :3], idx2[0, :3] = [-0.125, 0.0, 0.0], [12, 11, 10]                    # ranks: (0, 10) 1, (0, 11) 2, (0, 12) 3
    out = one_step(dev, val2, idx2, st, 3, 3, N=6, rate=0.25, max_new=3)
    assert out["next"].tolist() == [10, 11, 20] and out["score"][0].tolist() == [-0.25, -0.5, -0.5]
    # the first selection is the plain one; rate 0 is the plain one bit for bit
    st0 = hand_state(3, [0.5, 0.0, 0.0], t=0)
    a = one_step(dev, val[:1], idx[:1], st0, 3, 1, N=6, rate=0.25, max_new=3)
    b, _ = br.select_ref(val[:1], idx[:1], st0, 3, 1)
    assert all(np.array_equal(bits(a[k]), bits(b[k])) for k in br.STATE_KEYS)
    rs = np.random.RandomState(4)
    st5 = hand_state(5, -rs.randint(0, 9, size=(2, 5)).astype(np.float32) / 8, B=2)
    val5, idx5 = candidates(rs, 2, 5, 12, 1, pad_cols=0)
    src = np.zeros((10, 8), np.int32)
    gpu, twin = Device(st5, src, 5, dev), Device(st5, src, 5, dev)
    assert gpu.run(val5, idx5, 5, rate=0.0) == 0 and twin.run(val5, idx5, 5, plain=True) == 0
    same(gpu.state(), twin.state(), "rate 0")


@pytest.mark.parametrize("beam,rate", [(3, 0.25), (5, 0.125)])
def test_runs_of_steps_under_a_rate(dev, beam, rate):
    st, seen = run_steps(dev, 3, beam, 2 * beam + 2, [3, 0, 5], 40 + beam, rate=rate, sparse=2)
    print(f"beam {beam} rate {rate}: finalized {st['fin_n'].tolist()}, steps {st['t'].tolist()}, seen {seen}")
    assert st["finished"].all() and seen["fin"] >= 2 and seen["penalised"] >= 2


# ---------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_touch_nothing(dev):
    from gnnlm_amd import _lib
    beam, N, B = 4, 8, 2
    st = hand_state(beam, [[-1.0, -1.0, -2.0, -2.0]] * B, B=B, max_new=MAX_NEW)
    for k in ("next", "parent", "hist_tok", "hist_par", "fin_tok", "fin_len", "done"):
        st[k][...] = SENTINEL
    for k in ("hist_score", "fin_cum", "fin_score"):
        st[k][...] = float(SENTINEL)
    src = np.full((B * beam, 9), SENTINEL, np.int32)
    val, idx = np.tile(HAND_VAL, (B, 1)), np.tile(HAND_IDX, (B, 1))

    def check(match, groups=2, strength=0.5, rate=0.0, **edit):
        gpu = Device(st, src, beam, dev)
        gpu.feed(val, idx, beam, N)
        gpu.dd.groups, gpu.dd.strength, gpu.dd.rate = groups, strength, rate
        for k, v in edit.items():
            setattr(gpu.dd.sel, k, v(gpu.dd.sel) if callable(v) else v)
        assert _lib.lib().gnnlm_beam_select_diverse(ctypes.byref(gpu.dd), _lib.stream()) == -22, match
        assert match in _lib.lib().gnnlm_last_error().decode(), (match, _lib.lib().gnnlm_last_error().decode())
        torch.cuda.synchronize()
        same(gpu.state(), (st, src), match)                  # the sentinels stand

    check("groups < 1", groups=0)
    check("groups < 1", groups=-2)
    check("beam % groups", groups=3)
    check("beam % groups", groups=8)
    check("strength", strength=-0.5)
    check("strength", strength=float("nan"))
    check("strength", strength=float("inf"))
    check("rate", groups=1, rate=-0.25)
    check("rate", groups=1, rate=float("nan"))
    check("rate", groups=1, rate=float("inf"))
    check("together with rate", groups=2, rate=0.5)
    # everything gnnlm_beam_select refuses
    check("beam outside", beam=0)
    check("beam outside", beam=33)
    check("N < 2 * beam", N=7)
    check("beam_in", beam_in=2)
    check("8192", beam=32, beam_in=32, N=257, groups=4)
    check("ld_val", ld_val=N - 1)
    check("ld_val", ld_id=N - 1)
    check("max_new", max_new=-1)
    check("max_new", B=-1)
    check("ld_src", ld_src=8)
    check("cap", cap=-1)
    check("src_in", src_in=None)
    for field in ("cand_val", "cand_id", "score_in", "score_out", "t", "finished", "len", "done", "next", "parent"):
        check("missing", **{field: None})
    for field in ("hist_tok", "hist_par", "hist_score", "fin_n", "fin_tok", "fin_cum", "fin_len", "fin_score"):
        check("hist_* / fin_* missing", **{field: None})
    check("misaligned", next=lambda d: d.next + 4)
    check("misaligned", t=lambda d: d.t + 2)
    assert _lib.lib().gnnlm_beam_select_diverse(None, _lib.stream()) == -22
    # B = 0 is accepted and touches nothing; without a table the rest is as with one
    gpu = Device(st, src, beam, dev)
    gpu.dd.sel.B = 0
    assert gpu.run(val, idx, beam, N, groups=2, strength=0.5) == 0
    same(gpu.state(), (st, src), "B = 0")
    gpu = Device(st, src, beam, dev)
    gpu.dd.sel.src_in = gpu.dd.sel.src_out = None
    assert gpu.run(val, idx, beam, N, groups=2, strength=0.5) == 0
    want, _ = db.select_diverse_ref(val, idx, st, beam, beam, 2, 0.5)
    same(gpu.state(), (want, src), "no table")


def test_ops_wrapper(dev):
    """ops.beam_select_diverse over a BeamState gives what the hand-filled descriptor gives."""
    from gnnlm_amd import ops
    from gnnlm_amd.beam_search import BeamState
    beam, N, B = 4, 8, 2
    st = br.new_state(B, beam, MAX_NEW, [3, 5])
    st["t"][:], st["score"][:] = 1, [-1.0, -1.0, -2.0, -2.0]
    val, idx = np.tile(HAND_VAL, (B, 1)), np.tile(HAND_IDX, (B, 1))
    state = BeamState(B, beam, MAX_NEW, torch.from_numpy(st["len"]).to(dev), torch.zeros(B * beam, dtype=torch.int32, device=dev), dev)
    state.t += 1
    state.score.copy_(torch.from_numpy(st["score"]))
    src = np.tile(np.arange(B * beam, dtype=np.int32)[::-1, None], (1, 9))
    table = torch.from_numpy(src.copy()).to(dev)
    nxt, parent = ops.beam_select_diverse(torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev), state, src=table, eos=br.EOS, pad=br.PAD,
                                          groups=2, strength=0.5)
    want, tab = db.select_diverse_ref(val, idx, st, beam, beam, 2, 0.5, src=src)
    same(({k: getattr(state, k).cpu().numpy() for k in br.STATE_KEYS}, table.cpu().numpy()), (want, tab), "ops.beam_select_diverse")
    assert nxt is state.next and parent is state.parent and want["next"][:beam].tolist() == [7, 20, 10, 21]
    with pytest.raises(Exception, match="beam % groups"):
        ops.beam_select_diverse(torch.from_numpy(val).to(dev), torch.from_numpy(idx).to(dev), state, src=table, groups=3)


# ---------------------------------------------------------------------------------------------------- 6. a captured select + step
def test_captured_diverse_select_and_step_replay_the_eager_pair(dev):
    import decode_ref as dr
    import test_beam_search_gpu as e2e
    from gnnlm_amd import ops
    from gnnlm_amd.beam_search import BeamGenerator
    seed, beam, max_new = 301, 4, 8
    lm = e2e.gen_lm(seed, "dense", dev)
    g = BeamGenerator(lm)
    prompts = dr.gen_prompts(seed)[1:]
    bound = max(len(p) for p in prompts) + max_new

    def pair(run, xbuf):
        ops.beam_select_diverse(run["cand"][0], run["cand"][1], run["state"], src=run["table"], eos=dr.EOS, pad=dr.PAD, groups=2, strength=0.5)
        x, _ = lm.step(run["state"].next, run["cache"], want_inner=False, want_ffn_input=False, max_len=bound, src=run["table"])
        xbuf.copy_(x)

    def start():
        run = g.start(prompts, max_new, beam)
        val, idx = g.candidates(run, run["x"], {}, 0, min_len=max_new)
        ops.beam_select_diverse(val, idx, run["state"], src=run["table"], eos=dr.EOS, pad=dr.PAD, groups=2, strength=0.5)
        x, _ = lm.step(run["state"].next, run["cache"], want_inner=False, want_ffn_input=False, max_len=bound, src=run["table"])
        xbuf = x.clone()
        g.candidates(run, xbuf, {}, 1, min_len=max_new)
        pair(run, xbuf)                                      # the warm-up of the pair itself (step 1)
        g.candidates(run, xbuf, {}, 2, min_len=max_new)
        return run, xbuf

    def snap(run, xbuf):
        s = run["state"]
        return [v.clone() for v in (s.next, s.parent, s.score, s.t, s.hist_tok, s.hist_par, s.hist_score, xbuf, run["table"], run["cache"].len)]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run, xbuf = start()
        pair(run, xbuf)
        eager = snap(run, xbuf)
        run2, xbuf2 = start()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pair(run2, xbuf2)
        replayed_once = snap(run2, xbuf2)                    # (capture runs nothing)
        graph.replay()
        replayed = snap(run2, xbuf2)
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    as_bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x
    for a, b in zip(eager, replayed):
        assert torch.equal(as_bits(a), as_bits(b))
    assert replayed[3].tolist() == [3] * len(prompts) and replayed_once[3].tolist() == [2] * len(prompts)
    assert int(run2["cache"].n_bad.item()) == 0 and (replayed[0] != dr.PAD).all()
