"""``gnnlm_pack_rows`` without a GPU: the restatement's row map, the derived bound on the unit rows (tests/pack_rows_ref.py) against
float32 evaluations of the kernel's expression in three summation orders, and the ABI additions (header, struct, symbol)."""
import ctypes
import re

import numpy as np

import pack_rows_ref as pr


def test_row_map_and_tables():
    block_off, skip, out_off = pr.tables([3, 1, 4, 2], [1, 1, 0, 2], base=7)
    assert block_off.tolist() == [7, 10, 11, 15, 17] and out_off.tolist() == [0, 2, 2, 6, 6]
    assert pr.source_rows(block_off, skip, out_off).tolist() == [1, 2, 4, 5, 6, 7]
    assert pr.source_rows(block_off, None, np.array([0, 3, 4, 8, 10])).tolist() == list(range(10))
    src = np.arange(10 * 5, dtype=np.float32).reshape(10, 5)
    rows, unit = pr.pack(src, block_off, skip, out_off, 4)
    assert np.array_equal(rows, src[[1, 2, 4, 5, 6, 7], :4])
    assert np.allclose((unit ** 2).sum(-1), 1.0, atol=1e-12)


def test_bound_covers_float32_in_any_order_and_has_teeth():
    rs = np.random.RandomState(3)
    for d in (4, 6, 32, 100, 1024):
        x = (rs.randn(24, d) * rs.choice([1e-3, 1.0, 300.0], size=(24, 1))).astype(np.float32)
        x[5] = np.abs(x[5])                                     # all one sign: the sum's rounding errors cannot cancel
        _, unit = pr.pack(x, *pr.tables([24]), d)
        tol = pr.unit_tolerance(unit, d)
        worst = 0.0
        for order in ("forward", "reverse", "lanes"):
            y = pr.unit_f32(x, order)
            err = np.abs(y.astype(np.float64) - unit)
            assert (err <= tol).all(), (d, order)
            worst = max(worst, float((err / tol).max()))
        print(f"d = {d}: worst error / bound = {worst:.3f}")
        assert tol.max() <= 3.2e-5 * d / 1024 + 2.5e-7          # (|unit| <= 1: about d / 2 float32 ulps of 1, 3.1e-5 at d = 1024)
        # teeth: a float16 sum, or a row scaled by a norm that is one part in 10^3 off, is outside
        bad = (x / (np.sqrt((x.astype(np.float64) ** 2).sum(-1, keepdims=True)) * 1.001)).astype(np.float32)
        assert not (np.abs(bad.astype(np.float64) - unit) <= tol).all()


def test_zero_row_is_what_the_division_gives():
    x = np.zeros((2, 8), np.float32)
    x[1, 3] = 2.0
    _, unit = pr.pack(x, *pr.tables([2]), 8)
    assert np.isnan(unit[0]).all() and unit[1, 3] == 1.0
    assert np.isnan(pr.unit_f32(x)[0]).all()


def test_abi_additions():
    from gnnlm_amd import _lib
    text = open(_lib.HEADER).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", text)                                   # additions only
    assert "gnnlm_pack_rows" in _lib.exported_symbols()
    st = _lib.STRUCTS["gnnlm_pack_rows_t"]
    names = [f[0] for f in st._fields_]
    assert names == ["src", "ld_src", "block_off", "skip", "out_off", "dst", "ld_dst", "dst_unit", "ld_unit", "n_blocks", "d", "n_tok", "n_out",
                     "n_bad", "wait"]
    L = _lib.lib()
    assert L.gnnlm_abi_version() == 12
    assert L.gnnlm_sizeof(b"gnnlm_pack_rows_t") == ctypes.sizeof(st)
    assert hasattr(L, "gnnlm_pack_rows")
