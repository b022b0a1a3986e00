"""gnnlm_topk_merge at the descriptor level (include/gnnlm.h: gnnlm_topk_t): every route of the dispatcher -- select<KP, EPT> for
KP in {64, 256, 1024, 2048} and EPT in {16, 20}, merge<KP> for KP in {512, 1024, 2048} with and without the counting pre-pass --
against the numpy restatement of tests/topk_ref.py, and gnnlm_ivfpq_split_payload against two lines of numpy.  Descriptors are
filled by hand and passed to ``_lib.call_desc``.

The contract is exact, so every comparison is: ids equal the reference's, values compare equal to it (``np.array_equal``; the sign
of a zero is unspecified, -0 == +0), the padding is -1 with -inf / +inf, guards are compared as bits.  No tolerance anywhere.

What EVERY call of this file carries (``lay_out`` / ``run``), so the field rules are checked by every case and not by one:
  * ld = ncols + 3 and ld_ids = ncols + 1, the scores pointer one float into its allocation; the pad columns hold the WINNING
    infinity (and valid ids): a kernel that strides by ncols, or reads a pad column, selects it;
  * in the ragged cases the columns beyond row_ncols[r] hold the winning infinity with valid ids; row_ncols holds values above
    ncols (clamped), 0 and negative ones (empty rows);
  * ids, col_ids and col0 are set together where ids or col_ids are: the sources that must be ignored are poisoned (col0 so
    negative that every column would be skipped, col_ids other ids with every second one -1);
  * the state buffers lie between guard regions; before an init = 1 call they hold a NaN-payload sentinel and a sentinel id, so
    every one of the n * k slots must be overwritten; a second identical call gives identical bits.
The rows of a case are described in topk_ref.py (ties by the thousand at the cut, ascending rows, an invalid or constant sample,
NaN / infinities / zeros of both signs / denormals, tied runs whose ids differ in one 11-bit digit of the select kernel's id
radix); test_topk_ref_cpu.py checks without a GPU that they are what they say and that every case notices every field it sets.
Denormals are ordered as numbers (gfx9 keeps float32 denormals): the 'specials' row of every case expects it of both kernels.

Out of scope: the GNNLM_TOPK_MERGE_ONLY switch.  It is read once per process and only reaches a path production never takes
(init = 1 in the merge kernel without the pre-pass on narrow rows)."""
import numpy as np
import pytest
import torch

import topk_ref as ref

pytestmark = pytest.mark.gpu

SENT_F_BITS = 0x7FC0BEEF                                                      # a NaN with a payload of its own: compared as bits
SENT_I = -0x0123456789ABCDEF
GUARD = 64
PAD_ID = 1                                                                    # a valid id in the pad column of ids


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def lay_out(call, dev):
    """-> (descriptor without state, tensors to keep alive)"""
    from gnnlm_amd import _lib
    n, nc = call["scores"].shape
    assert nc == call["ncols"]
    win = np.float32(np.inf if call["largest"] else -np.inf)
    d, keep = _lib.gnnlm_topk_t(), []
    d.n, d.ncols, d.k, d.largest, d.init = n, nc, call["k"], call["largest"], call["init"]
    d.alpha, d.col0 = call["alpha"], call["col0"]
    if nc > 0:                                                                # (ncols = 0: null scores are accepted)
        ld = nc + 3
        host = np.full(1 + n * ld, win, dtype=np.float32)
        host[1:].reshape(n, ld)[:, :nc] = call["scores"]
        t = to_dev(host, dev)
        d.scores, d.ld = t.data_ptr() + 4, ld
        keep.append(t)
        if call["ids"] is not None:
            ids = np.full((n, nc + 1), PAD_ID, dtype=np.int64)
            ids[:, :nc] = call["ids"]
            t = to_dev(ids, dev)
            d.ids, d.ld_ids = t.data_ptr(), nc + 1
            keep.append(t)
        for f in ("col_ids", "col_scale", "col_bias"):
            if call[f] is not None:
                t = to_dev(call[f], dev)
                assert t.numel() == nc and t.dtype == (torch.int64 if f == "col_ids" else torch.float32)
                setattr(d, f, t.data_ptr())
                keep.append(t)
    if call["row_ncols"] is not None:
        t = to_dev(call["row_ncols"].astype(np.int32), dev)
        d.row_ncols = t.data_ptr()
        keep.append(t)
    return d, keep


def state_buffers(n, k, dev, state=None):
    """best_val / best_id between guards: the sentinel everywhere, the incoming state inside if there is one"""
    v = np.full(2 * GUARD + n * k, SENT_F_BITS, dtype=np.uint32).view(np.float32)
    i = np.full(2 * GUARD + n * k, SENT_I, dtype=np.int64)
    if state is not None:
        v[GUARD:GUARD + n * k], i[GUARD:GUARD + n * k] = state[0].reshape(-1), state[1].reshape(-1)
    return to_dev(v, dev), to_dev(i, dev)


def read_state(vt, it, n, k, touched=True):
    """(val [n, k], id [n, k]) of the buffers; the guards still hold the sentinel; ``touched``: no slot inside does"""
    v, i = vt.cpu().numpy(), it.cpu().numpy()
    inner = slice(GUARD, GUARD + n * k)
    assert (bits(v[:GUARD]) == SENT_F_BITS).all() and (bits(v[GUARD + n * k:]) == SENT_F_BITS).all()
    assert (i[:GUARD] == SENT_I).all() and (i[GUARD + n * k:] == SENT_I).all()
    if touched:
        assert not (bits(v[inner]) == SENT_F_BITS).any() and not (i[inner] == SENT_I).any()
    return v[inner].reshape(n, k), i[inner].reshape(n, k)


def launch(d, vt, it):
    from gnnlm_amd import _lib
    d.best_val, d.best_id = vt.data_ptr() + 4 * GUARD, it.data_ptr() + 8 * GUARD
    _lib.call_desc("gnnlm_topk_merge", d)
    torch.cuda.synchronize()


def run(call, dev, state=None):
    """The call on the device, twice from the same incoming state: identical bits; -> (val, id)."""
    n, k = call["scores"].shape[0], call["k"]
    d, keep = lay_out(call, dev)
    outs = []
    for _ in range(2):
        vt, it = state_buffers(n, k, dev, None if call["init"] else state)
        launch(d, vt, it)
        outs.append(read_state(vt, it, n, k))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def check(got, want):
    """ids exactly, values equal, the padding exactly -1 with the worst infinity (array_equal tells the infinities apart)"""
    (gv, gi), (wv, wi) = got, want
    assert gv.shape == wv.shape
    for r in range(len(wi)):
        assert np.array_equal(gi[r], wi[r]), (r, int((gi[r] != wi[r]).argmax()), int((wi[r] >= 0).sum()))
        assert np.array_equal(gv[r], wv[r]), (r, int((gv[r] != wv[r]).argmax()))
    pad = wi < 0
    assert (gi[pad] == -1).all() and np.array_equal(bits(gv[pad]), bits(wv[pad]))


def device_empty_state(n, k, largest, dev):
    """the empty state as the entry point writes it: init = 1 over 0 columns, null scores"""
    empty = dict(scores=np.zeros((n, 0), dtype=np.float32), ncols=0, k=k, largest=largest, init=1, alpha=1.0, col0=0, col_ids=None,
                 col_scale=None, col_bias=None, ids=None, row_ncols=None)
    got = run(empty, dev)
    check(got, ref.empty_state(n, k, largest))
    return got


# ----------------------------------------------------------------------------------------------------- 1. the select kernel
@pytest.mark.parametrize("spec", ref.SELECT_CASES, ids=ref.select_case_id)
def test_select(dev, spec):
    call = ref.make_case(spec)
    assert ref.route(call).startswith("select<")
    print(ref.route(call), len(call["patterns"]), "rows")
    check(run(call, dev), ref.fold(call))


# ----------------------------------------------------------------------------------------------------- 2. the merge kernel
@pytest.mark.parametrize("spec", ref.MERGE_CASES, ids=ref.merge_case_id)
def test_merge(dev, spec):
    """init = 0 over every chunk width and incoming state (an 'empty' one is written by the device: init = 1 over 0 columns); init = 1
    with 16385 columns: the pre-pass; per-row ids with row_ncols in {0, 1, cap}: the round-2 fold of the IVF-PQ search."""
    call, state = ref.make_merge_case(spec)
    assert ref.route(call) == f"merge<{ref.merge_kp(spec['k'])}>" + ("+prepass" if spec["init"] else "")
    print(ref.route(call), len(call["patterns"]), "rows")
    if spec["state"] == "empty":
        dv, di = device_empty_state(len(call["patterns"]), spec["k"], spec["largest"], dev)
        assert np.array_equal(bits(dv), bits(state[0])) and np.array_equal(di, state[1])
    got = run(call, dev, state)
    check(got, ref.fold(call, state))
    if call["ncols"] == 0:                                                    # an empty chunk leaves the state's content as it is
        check(got, state)


# ----------------------------------------------------------------------------------------------------- 3. chunking
def widen(call, width, largest):
    """The call behind a descriptor of ``width`` columns: row_ncols = its own width, the columns beyond hold the winning infinity, valid
    ids, scale 1 and bias 0."""
    n, nc = call["scores"].shape
    a = np.float32(1.0 if call["alpha"] == 0 else call["alpha"])
    win = np.float32(np.inf if largest else -np.inf) * np.sign(a)
    w = dict(call, ncols=width, row_ncols=np.full(n, nc, dtype=np.int32))
    w["scores"] = np.concatenate([call["scores"], np.full((n, width - nc), win, dtype=np.float32)], axis=1)
    if call["col_scale"] is not None:
        w["col_scale"] = np.concatenate([call["col_scale"], np.ones(width - nc, dtype=np.float32)])
    if call["col_bias"] is not None:
        w["col_bias"] = np.concatenate([call["col_bias"], np.zeros(width - nc, dtype=np.float32)])
    extra = (1 << 58) + np.arange(width - nc, dtype=np.int64)
    if call["col_ids"] is not None:
        w["col_ids"] = np.concatenate([call["col_ids"], extra])
    if call["ids"] is not None:
        w["ids"] = np.concatenate([call["ids"], np.broadcast_to(extra, (n, width - nc))], axis=1)
    return w


@pytest.mark.parametrize("spec", ref.CHUNK_CASES, ids=ref.chunk_case_id)
def test_chunking(dev, spec):
    """The same rows in one select call, as {1 column, the rest}, in ragged chunks (an empty one among them) and as {a 16385 wide first
    chunk: the merge kernel with its pre-pass, the rest}: identical ids, equal values (a zero may differ in sign), all equal to the
    reference."""
    call = ref.make_case(spec)
    want = ref.fold(call)
    results = {}
    for name, cuts in spec["cuts"].items():
        state = None
        for j, (c0, c1) in enumerate(cuts):
            sub = ref.split(call, c0, c1, init=int(j == 0))
            if name == "wide+rest" and j == 0:
                sub = widen(sub, spec["wide"], spec["largest"])
                assert ref.route(sub) == f"merge<{ref.merge_kp(spec['k'])}>+prepass"
            elif j == 0:
                assert ref.route(sub).startswith("select<")
            expect = ref.fold(sub, state)
            state = run(sub, dev, state)
            check(state, expect)                                              # every step, from the device's own state
        results[name] = state
        check(state, want)
    for name, (v, i) in results.items():
        assert np.array_equal(i, results["one"][1]) and np.array_equal(v, results["one"][0]), name


# ----------------------------------------------------------------------------------------------------- 4. accepted and refused
def small_call(init=1, n=3, nc=40, k=8):
    rs = np.random.RandomState(1)
    return dict(scores=rs.randn(n, nc).astype(np.float32), ncols=nc, k=k, largest=1, init=init, alpha=1.0, col0=100, col_ids=None,
                col_scale=None, col_bias=None, ids=None, row_ncols=None)


def test_refused(dev):
    """Descriptors the entry point must refuse, each one field away from a valid one: GnnlmError, nothing written."""
    from gnnlm_amd._lib import GnnlmError

    def refused(change, k=8, null=None):
        call = small_call()
        d, keep = lay_out(call, dev)
        vt, it = state_buffers(3, k, dev)
        change(d)
        d.best_val, d.best_id = vt.data_ptr() + 4 * GUARD, it.data_ptr() + 8 * GUARD
        if null:
            setattr(d, null, None)
        with pytest.raises(GnnlmError):
            from gnnlm_amd import _lib
            _lib.call_desc("gnnlm_topk_merge", d)
        torch.cuda.synchronize()
        assert (bits(vt.cpu().numpy()) == SENT_F_BITS).all() and (it.cpu().numpy() == SENT_I).all()

    def setter(**kw):
        def f(d):
            for a, b in kw.items():
                setattr(d, a, b)
        return f

    d, keep = lay_out(small_call(), dev)                                      # the valid one is accepted
    vt, it = state_buffers(3, 8, dev)
    launch(d, vt, it)
    check(read_state(vt, it, 3, 8), ref.fold(small_call()))
    refused(setter(k=0))
    refused(setter(k=2049), k=2049)
    refused(setter(), null="best_val")
    refused(setter(), null="best_id")
    refused(setter(n=-1))
    refused(setter(ncols=-1))
    refused(setter(), null="scores")
    refused(setter(init=0), null="scores")


def test_accepted_empty_shapes(dev):
    """n = 0 touches nothing (whatever else the descriptor holds); ncols = 0 with null scores: init = 1 writes the padding, init = 0
    leaves the state's content as it is, in both directions."""
    d, keep = lay_out(small_call(), dev)
    vt, it = state_buffers(3, 8, dev)
    d.n, d.scores = 0, None
    launch(d, vt, it)
    assert (bits(vt.cpu().numpy()) == SENT_F_BITS).all() and (it.cpu().numpy() == SENT_I).all()
    for largest in (1, 0):
        for k in (1, 8, 300, 2048):
            device_empty_state(3, k, largest, dev)
        src = small_call()
        src["largest"] = largest
        for nc in (40, 5):                                                    # a full state, one with unfilled slots
            state = ref.fold(ref.split(src, 0, nc, init=1))
            none = dict(ref.split(src, 0, 0, init=0), row_ncols=np.array([0, 5, -1], dtype=np.int32))
            check(run(none, dev, state), state)


# ----------------------------------------------------------------------------------------------------- 5. gnnlm_ivfpq_split_payload
def split_payload(idx_t, n, label_bits, val_last, vals_t):
    from gnnlm_amd import _lib
    _lib.call("gnnlm_ivfpq_split_payload", _lib.ptr(idx_t), n, label_bits, val_last, _lib.ptr(vals_t), _lib.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("with_vals", [False, True])
@pytest.mark.parametrize("label_bits", [1, 24, 31])
def test_split_payload(dev, label_bits, with_vals):
    """payload = id << label_bits | label, negative = none: the id in place (a negative payload stays), the label to out_vals (none:
    val_last); out_vals = NULL: ids only.  n in {0, 1, 255, 256, 257} (blocks of 256), guard words behind both arrays."""
    rs = np.random.RandomState(label_bits)
    val_last, guard = -12345, 16
    for n in (0, 1, 255, 256, 257):
        p = (rs.randint(0, 1 << 31, 300).astype(np.int64) << 31 | rs.randint(0, 1 << 31, 300)).astype(np.int64)
        p[:6] = [((1 << 31) - 1) << 24 | 0xFFFFFF, -1, 0, -5, -(1 << 62), (1 << 62) + 12345]
        p = rs.permutation(p[:n])
        idx = np.concatenate([p, np.full(guard, SENT_I, dtype=np.int64)])
        idx_t = to_dev(idx, dev)
        vals_t = torch.full((n + guard,), 0x5EADBEEF, dtype=torch.int32, device=dev) if with_vals else None
        split_payload(idx_t, n, label_bits, val_last, vals_t)
        got = idx_t.cpu().numpy()
        assert np.array_equal(got[:n], np.where(p < 0, p, p >> label_bits)) and (got[n:] == SENT_I).all(), n
        if with_vals:
            got = vals_t.cpu().numpy()
            assert np.array_equal(got[:n], np.where(p < 0, val_last, p & ((1 << label_bits) - 1)).astype(np.int32)), n
            assert (got[n:] == 0x5EADBEEF).all(), n


def test_split_payload_refused(dev):
    from gnnlm_amd._lib import GnnlmError
    idx_t = torch.full((8,), 77, dtype=torch.int64, device=dev)
    vals_t = torch.full((8,), 5, dtype=torch.int32, device=dev)
    for bad in (0, 32):
        with pytest.raises(GnnlmError):
            split_payload(idx_t, 8, bad, -1, vals_t)
    with pytest.raises(GnnlmError):
        split_payload(None, 8, 24, -1, vals_t)
    with pytest.raises(GnnlmError):
        split_payload(idx_t, -1, 24, -1, vals_t)
    assert (idx_t.cpu().numpy() == 77).all() and (vals_t.cpu().numpy() == 5).all()
