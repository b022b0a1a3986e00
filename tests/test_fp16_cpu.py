"""`--fp16` without a GPU: the ABI documents precision 3 and keeps its version, the Python table and the parser know the mode, the
"ignored" warning is gone, and the fixture's inputs are the ones tests/fp16_inputs.py regenerates."""
import os
import re

import numpy as np

import fp16_inputs as fi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "gnnlm.h")).read()


def test_header_documents_fp16_at_the_three_precision_fields():
    h = _header()
    fields = [m.start() for m in re.finditer(r"int32_t (gemm_)?precision;", h)]
    assert len(fields) == 3
    for at in fields:
        comment = h[at:h.index("*/", at)]
        assert "3" in comment and "fp16" in comment, comment


def test_abi_version_is_unchanged():
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", _header())


def test_precisions_table():
    from gnnlm_amd import ops
    assert ops.PRECISIONS["fp16"] == 3
    assert ops.PRECISIONS == {"f32": 0, "bf16x3": 1, "bf16x6": 2, "fp16": 3}
    assert ops.precision_value("fp16") == 3 and ops.precision_value(3) == 3 and ops.precision_name(3, 3) == "fp16"
    for bad in ("fp8", 4, -1):
        try:
            ops.precision_value(bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_parser_accepts_fp16_and_nothing_is_ignored():
    from gnnlm_amd import eval_lm
    assert eval_lm.get_parser().parse_args(["data", "--path", "ckpt.pt", "--fp16"]).fp16 is True
    assert eval_lm.get_parser().parse_args(["data", "--path", "ckpt.pt"]).fp16 is False
    src = open(os.path.join(ROOT, "gnn-lm_amd", "eval_lm.py")).read()
    assert "ignored" not in src


def test_engine_and_model_take_a_precision():
    import torch
    from gnnlm_amd.engine import GnnLmEngine
    from gnnlm_amd.hgt import HGT
    from gnnlm_amd.model import GnnLmModel

    class Asm:
        gemm_precision = 0
    hgt, asm = HGT(in_dim=32, hidden_dim=32, out_dim=32, n_layers=1, n_heads=2), Asm()
    eng = GnnLmEngine(hgt, asm, None, 2, 2, precision="fp16")
    assert (hgt.gemm_precision, asm.gemm_precision, eng.precision) == (3, 3, "fp16")
    eng.precision = "f32"
    assert (hgt.gemm_precision, asm.gemm_precision, eng.precision) == (0, 0, "f32")
    m = GnnLmModel(hgt, asm, precision="fp16")
    assert (hgt.gemm_precision, asm.gemm_precision, m.precision) == (3, 3, "fp16")
    assert GnnLmModel(hgt, asm).precision == "fp16"            # None leaves what the modules carry
    assert isinstance(m, torch.nn.Module)


def test_fixture_checksums_match_the_generator():
    g = np.load(os.path.join(ROOT, "tests", "golden", "hgt_fp16.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hgt_fp16.npz")) < 900 * 1024
    for name, c in fi.HGT_CASES.items():
        assert np.array_equal(g[name + ".checksum"], fi.checksum(fi.hgt_inputs(name))), name
        assert g[name + ".ref_f64"].dtype == np.float64 and g[name + ".ref_half"].dtype == np.float16
        assert g[name + ".ref_f64"].shape == g[name + ".ref_half"].shape == (c["T"], c["d"])
    assert np.array_equal(g["asm.checksum"], fi.checksum(fi.asm_inputs()))
    assert g["asm.ref_f64"].shape == g["asm.ref_half"].shape == (fi.ASM_CASE["n"],)
    # the yardstick exists: the reference's half run is measurably away from its float64 run, and finite
    for key in list(fi.HGT_CASES) + ["asm"]:
        d = g[key + ".ref_half"].astype(np.float64) - g[key + ".ref_f64"]
        assert np.isfinite(d).all() and 1e-5 < np.sqrt(np.mean(d * d)) < 1e-1, key
