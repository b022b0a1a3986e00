"""``gnnlm_pack_rows`` at the descriptor level: ``gnnlm_pack_rows_t`` filled by hand and called through ``_lib`` -- every layout of the
tables, both outputs, both code paths (16-byte and scalar), the refusals.  GPU only.

Bars: the copy bit for bit; the unit rows within ``pack_rows_ref.unit_tolerance`` (derived there: a float32 sum of d squares in any
order, one square root, one division) of the float64 restatement; pad columns and rows that are not described keep a sentinel.
"""
import ctypes

import numpy as np
import pytest
import torch

import pack_rows_ref as pr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0

LAYOUTS = {
    # name: (block lengths, skips or None)
    "rows_of_1": ([1] * 9, [0] * 9),
    "skip_null": ([5, 1, 33, 7], None),
    "some_skipped": ([4, 6, 1, 9, 3], [4, 2, 1, 0, 3]),
    "all_skipped": ([3, 5, 2], [3, 5, 2]),
    "one_block": ([37], [29]),
    "70_blocks": ([1 + (7 * i) % 5 for i in range(70)], [(3 * i) % (1 + (7 * i) % 5 + 1) if i % 9 else 0 for i in range(70)]),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Call:
    """One hand-filled descriptor with its device buffers."""

    def __init__(self, dev, src_np, lengths, skips, d, ld_src=None, base=0, src_offset=0, want=("dst", "unit"), pad=4):
        from gnnlm_amd import _lib
        self._lib = _lib
        self.d, self.want = d, want
        self.block_off, self.skip, self.out_off = pr.tables(lengths, skips, base)
        if skips is None:
            self.skip = None
        n_tok, self.n_out = int(sum(lengths)), int(self.out_off[-1])
        ld_src = d if ld_src is None else ld_src
        # the source rows live in a flat buffer, `src_offset` floats in: an offset of 1 leaves the rows 4-byte aligned only
        flat = np.full(src_offset + n_tok * ld_src + 4, SENTINEL, np.float32)
        view = flat[src_offset:src_offset + n_tok * ld_src].reshape(n_tok, ld_src)
        view[:, :d] = src_np[:n_tok, :d]
        self.src_host = view.copy()
        self.flat = t(flat, dev)
        self.tabs = {k: (None if v is None else t(v, dev)) for k, v in (("block_off", self.block_off), ("skip", self.skip), ("out_off", self.out_off))}
        self.ld_out = d + pad
        self.out = {k: torch.full((max(self.n_out, 1) + 1, self.ld_out), SENTINEL, device=dev) for k in ("dst", "unit")}
        self.n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
        q = _lib.gnnlm_pack_rows_t()
        q.src, q.ld_src = self.flat.data_ptr() + 4 * src_offset, ld_src
        q.block_off, q.out_off = self.tabs["block_off"].data_ptr(), self.tabs["out_off"].data_ptr()
        q.skip = None if self.skip is None else self.tabs["skip"].data_ptr()
        if "dst" in want:
            q.dst, q.ld_dst = self.out["dst"].data_ptr(), self.ld_out
        if "unit" in want:
            q.dst_unit, q.ld_unit = self.out["unit"].data_ptr(), self.ld_out
        q.n_blocks, q.d, q.n_tok, q.n_out = len(lengths), d, n_tok, self.n_out
        q.n_bad, q.wait = self.n_bad.data_ptr(), 1
        self.q = q

    def run(self):
        L = self._lib.lib()
        rc = L.gnnlm_pack_rows(ctypes.byref(self.q), self._lib.stream())
        torch.cuda.synchronize()
        return rc

    def check(self):
        rows, unit = pr.pack(self.src_host, self.block_off, self.skip, self.out_off, self.d)
        n, d = self.n_out, self.d
        for key in ("dst", "unit"):
            got = self.out[key].cpu().numpy()
            assert (got[n:] == SENTINEL).all() and (got[:, d:] == SENTINEL).all(), key          # the spare row and the pad columns
            if key not in self.want:
                assert (got == SENTINEL).all(), key
        if "dst" in self.want:
            assert np.array_equal(self.out["dst"].cpu().numpy()[:n, :d].view(np.uint32), rows.view(np.uint32))
        if "unit" in self.want and n:
            got = self.out["unit"].cpu().numpy()[:n, :d].astype(np.float64)
            zero = ~np.isfinite(unit).all(-1)
            assert np.isnan(got[zero]).all()                                                    # 0 / 0, as the reference's expression
            err, tol = np.abs(got[~zero] - unit[~zero]), pr.unit_tolerance(unit[~zero], d)
            if err.size:
                print(f"d = {d}: unit rows worst error / bound = {(err / tol).max():.3f}")
            assert (err <= tol).all()


def source(n, d, seed):
    rs = np.random.RandomState(seed)
    return (rs.randn(n, d) * rs.choice([1e-2, 1.0, 50.0], size=(n, 1))).astype(np.float32)


@pytest.mark.parametrize("d", [4, 6, 32, 100, 1024])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts(dev, d, layout):
    lengths, skips = LAYOUTS[layout]
    src = source(sum(lengths), d, 11 + d)
    if sum(lengths) > 2:
        src[2] = 0                                               # a zero row (taken in some layouts, context in others)
    for ld_src in (d, 3 * d + 4):
        c = Call(dev, src, lengths, skips, d, ld_src=ld_src, base=5 if layout != "skip_null" else 0)
        assert c.run() == 0
        if layout == "all_skipped":
            assert c.n_out == 0
        c.check()


@pytest.mark.parametrize("d", [4, 32, 100, 1024])
def test_scalar_path_and_single_outputs(dev, d):
    """A source 4 bytes off a 16-byte boundary, or an output stride that is no multiple of 4 floats, takes the scalar path; each
    output alone and both together."""
    lengths, skips = LAYOUTS["some_skipped"]
    src = source(sum(lengths), d, 5)
    for off, pad in ((0, 4), (1, 4), (0, 3)):
        for want in (("dst",), ("unit",), ("dst", "unit")):
            c = Call(dev, src, lengths, skips, d, src_offset=off, want=want, base=3, pad=pad)
            assert c.run() == 0
            c.check()


def test_block_outside_the_rows_is_skipped(dev):
    """A block described beyond n_tok is never read: its output rows keep the sentinel, the others are written."""
    lengths, d = [3, 4, 5], 8
    src = source(12, d, 9)
    c = Call(dev, src, lengths, [1, 1, 1], d)
    c.q.n_tok = 7                                                 # the third block now ends at row 12 > n_tok
    c.q.n_bad, c.q.wait = None, 0                                 # (the tables themselves are consistent; nothing to count)
    assert c.run() == 0
    rows, _ = pr.pack(c.src_host, c.block_off, c.skip, c.out_off, d)
    got = c.out["dst"].cpu().numpy()
    assert np.array_equal(got[:5, :d], rows[:5]) and (got[5:] == SENTINEL).all()


def test_refusals_touch_nothing(dev):
    from gnnlm_amd import _lib
    lengths, skips, d = [4, 6, 3], [1, 0, 3], 8
    src = source(sum(lengths), d, 2)

    def refused(mutate, tables=None):
        c = Call(dev, src, lengths, skips, d)
        for name, values in (tables or {}).items():
            c.tabs[name].copy_(t(np.asarray(values, np.int32), dev))
        mutate(c.q)
        assert c.run() == -22
        assert _lib.lib().gnnlm_last_error()
        for o in c.out.values():
            assert (o == SENTINEL).all()
        return c

    refused(lambda q: setattr(q, "ld_src", d - 1))
    refused(lambda q: setattr(q, "ld_dst", d - 1))
    refused(lambda q: setattr(q, "ld_unit", d - 1))
    refused(lambda q: setattr(q, "d", 0))
    refused(lambda q: setattr(q, "d", -4))
    refused(lambda q: (setattr(q, "dst", None), setattr(q, "dst_unit", None)))
    refused(lambda q: setattr(q, "out_off", None))
    refused(lambda q: setattr(q, "n_out", -1))
    refused(lambda q: setattr(q, "n_bad", None))                  # wait without a counter
    # the tables, counted on the device: a negative skip, a skip longer than its block, an out_off that does not match the lengths
    same = lambda q: None
    for tables in ({"skip": [-1, 0, 3]}, {"skip": [1, 7, 3]}, {"out_off": [0, 3, 9, 10]}, {"out_off": [1, 4, 10, 10]}, {"out_off": [0, 3, 8, 9]}):
        c = refused(same, tables)
        assert int(c.n_bad.item()) >= 1
    # ... and with wait = 0 they are counted, not read back: the call returns 0 and follows nothing it cannot verify
    c = Call(dev, src, lengths, skips, d)
    c.tabs["skip"].copy_(t(np.asarray([-1, 0, 3], np.int32), dev))
    c.q.wait = 0
    assert c.run() == 0 and int(c.n_bad.item()) == 2              # (the skip itself, and the out_off entry it no longer matches)
    rows, _ = pr.pack(c.src_host, c.block_off, c.skip, c.out_off, d)
    got = c.out["dst"].cpu().numpy()
    assert (got[:3] == SENTINEL).all() and np.array_equal(got[3:9, :d], rows[3:9])      # the block with the bad skip is left alone
    # the unmodified call is accepted
    c = Call(dev, src, lengths, skips, d)
    assert c.run() == 0 and int(c.n_bad.item()) == 0
    c.check()


def test_ops_wrapper(dev):
    """``ops.pack_rows``: strided views in and out, what is not wanted is None, a bad table raises before anything is written."""
    from gnnlm_amd import ops
    from gnnlm_amd._lib import GnnlmError
    lengths, skips, d = [5, 8, 2], [2, 0, 1], 32
    block_off, skip, out_off = pr.tables(lengths, skips)
    wide = t(source(sum(lengths), 3 * d, 4), dev)
    src = wide[:, d:2 * d]                                       # a column block of a wider buffer (ld = 3 d)
    rows, unit = ops.pack_rows(src, t(block_off, dev), t(skip, dev), t(out_off, dev), d, want_rows=True, want_unit=True)
    want_rows, want_unit = pr.pack(src.cpu().numpy(), block_off, skip, out_off, d)
    assert np.array_equal(rows.cpu().numpy(), want_rows)
    assert (np.abs(unit.cpu().numpy().astype(np.float64) - want_unit) <= pr.unit_tolerance(want_unit, d)).all()
    only_rows = ops.pack_rows(src, t(block_off, dev), t(skip, dev), t(out_off, dev), d)
    assert only_rows[1] is None and torch.equal(only_rows[0], rows)
    out = torch.full((int(out_off[-1]), d), SENTINEL, device=dev)
    with pytest.raises(GnnlmError, match="tables"):
        ops.pack_rows(src, t(block_off, dev), t(np.asarray([2, 9, 1], np.int32), dev), t(out_off, dev), d, out=(out, None))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
