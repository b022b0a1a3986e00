"""The host side of the fused coarse step: the descriptor in header, binding and library; ``run_index_build.parse_opq_block``;
``ivfpq.choose_coarse`` and the threshold it reads; the slab rule.  No GPU."""
import ctypes
import inspect

import pytest


def test_descriptor_agrees_across_header_binding_and_library():
    from gnnlm_amd import _lib
    st = _lib.STRUCTS["gnnlm_ivfpq_coarse_t"]
    assert [f[0] for f in st._fields_] == ["x", "ldx", "n", "coarse", "nlist", "d", "col_bias", "k", "slabs", "part_val", "part_id",
                                           "out_val", "out_id"]
    types = dict(st._fields_)
    assert types["ldx"] is ctypes.c_int64 and types["n"] is ctypes.c_int64 and types["nlist"] is ctypes.c_int32
    assert all(types[f] is ctypes.c_void_p for f in ("x", "coarse", "col_bias", "part_val", "part_id", "out_val", "out_id"))
    L = _lib.lib()
    assert L.gnnlm_sizeof(b"gnnlm_ivfpq_coarse_t") == ctypes.sizeof(st) > 0
    assert "gnnlm_ivfpq_coarse_probes" in _lib.exported_symbols() and hasattr(L, "gnnlm_ivfpq_coarse_probes")
    assert _lib.ABI_VERSION == 12 and L.gnnlm_abi_version() == 12       # additive: the version stays


def test_parse_opq_block():
    from gnnlm_amd.run_index_build import parse_index_type, parse_opq_block
    assert parse_opq_block("OPQ16_64,IVF1048576,PQ16", 1024) == 64
    assert parse_opq_block("OPQ64_1024,IVF4096,PQ64", 1024) == 1024
    assert parse_opq_block("IVF4096,PQ64", 1024) is None
    assert parse_opq_block("OPQ64,IVF4096,PQ64", 1024) is None
    with pytest.raises(ValueError):
        parse_opq_block("OPQ16_60,IVF4096,PQ16", 1024)
    with pytest.raises(ValueError):
        parse_opq_block("OPQ16_2048,IVF4096,PQ16", 1024)
    assert parse_index_type("OPQ16_64,IVF1048576,PQ16") == (1048576, 16)  # (unchanged: still two numbers)


def test_choose_coarse(monkeypatch):
    from gnnlm_amd import ivfpq, ivfpq_train
    monkeypatch.delenv("GNNLM_IVF_COARSE", raising=False)
    assert ivfpq_train.COARSE_FUSED_MIN_LISTS >= 16384
    for nlist in (1, 4096, 8192, 1 << 18, 1 << 20):
        assert ivfpq.choose_coarse("int8", nlist) == "dense"
    for route in ("packed", "rowmajor"):
        assert ivfpq.choose_coarse(route, 4096) == "dense" and ivfpq.choose_coarse(route, 8192) == "dense"
        assert ivfpq.choose_coarse(route, 1 << 20) == "fused"
        assert ivfpq.choose_coarse(route, ivfpq_train.COARSE_FUSED_MIN_LISTS) == "fused"
        assert ivfpq.choose_coarse(route, ivfpq_train.COARSE_FUSED_MIN_LISTS - 1) == "dense"
        assert ivfpq.choose_coarse(route, 4096, "fused") == "fused" and ivfpq.choose_coarse(route, 1 << 20, "dense") == "dense"
    with pytest.raises(ValueError):
        ivfpq.choose_coarse("packed", 4096, "sparse")
    monkeypatch.setenv("GNNLM_IVF_COARSE", "fused")
    assert ivfpq.choose_coarse("rowmajor", 4096) == "fused" and ivfpq.choose_coarse("packed", 4096, "dense") == "dense"
    assert ivfpq.choose_coarse("int8", 4096) == "dense"                   # its scan reads the score matrix
    monkeypatch.setenv("GNNLM_IVF_COARSE", "dense")
    assert ivfpq.choose_coarse("packed", 1 << 20) == "dense" and ivfpq.choose_coarse("packed", 1 << 20, "fused") == "fused"
    assert not ivfpq_train.coarse_fused(1 << 20, 64) and ivfpq_train.coarse_fused(1 << 20, 64, "fused")
    monkeypatch.delenv("GNNLM_IVF_COARSE")
    assert ivfpq_train.coarse_fused(1 << 20, 64) and not ivfpq_train.coarse_fused(8192, 64) and not ivfpq_train.coarse_fused(1 << 20, 6)
    # the threshold is read when the decision is taken
    monkeypatch.setattr(ivfpq_train, "COARSE_FUSED_MIN_LISTS", 100)
    assert ivfpq.choose_coarse("packed", 128) == "fused" and ivfpq_train.coarse_fused(128, 64)


def test_plan_tuples_and_signatures_are_as_they_were():
    from gnnlm_amd import ivfpq, ivfpq_train, quantize_features
    assert ivfpq._Block._fields == ("qr", "cs", "pv", "pi", "lut", "tables", "cv", "ci", "cc")
    assert list(inspect.signature(ivfpq.choose_route).parameters) == ["M", "ntotal", "max_list", "nlist", "scan", "metric", "list_term_bytes"]
    assert inspect.signature(ivfpq.IVFPQIndex.__init__).parameters["coarse_route"].default is None
    for fn in (ivfpq.IVFPQIndex.train, ivfpq.IVFPQIndex.build, ivfpq_train.train, ivfpq_train.build_arrays):
        assert inspect.signature(fn).parameters["d_out"].default is None
    assert quantize_features._initial_rotation is ivfpq_train._initial_rotation          # one copy


def test_slab_rule():
    from gnnlm_amd.ops import ivfpq_coarse_slabs
    assert ivfpq_coarse_slabs(8192, 1 << 20, 32) == 8                       # 128 row tiles x 8 slabs = 1024 workgroups
    assert ivfpq_coarse_slabs(8192, 16384, 32) == 4                         # slabs no narrower than 4096 lists
    assert ivfpq_coarse_slabs(1 << 18, 1 << 20, 1) == 1
    assert ivfpq_coarse_slabs(1, 1 << 20, 64) == 64 and ivfpq_coarse_slabs(1, 1 << 20, 32) == 64
    assert ivfpq_coarse_slabs(5, 100, 4) == 1 and ivfpq_coarse_slabs(0, 0, 1) == 1
    for n, nlist, k in ((1, 1 << 20, 64), (300, 70001, 32), (8192, 1 << 20, 1)):
        assert ivfpq_coarse_slabs(n, nlist, k) * k <= 4096
