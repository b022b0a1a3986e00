"""Host side of the plain (non-adaptive) output layer (transformer.py:843-852,1081-1085: a ``--arch transformer_lm`` checkpoint,
enwik8): the C ABI's new struct and entries, the descriptor checks, the state-dict reader, and the fixture against the float64
restatement.  No GPU."""
import ctypes
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import dense_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_head.npz")


def test_header_and_library_export_the_new_entries():
    from gnnlm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gnnlm.h")).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", hdr) and _lib.ABI_VERSION == 12        # additions only
    syms = _lib.exported_symbols()
    L = _lib.lib()
    assert L.gnnlm_abi_version() == 12
    for name in ("gnnlm_dense_workspace_bytes", "gnnlm_dense_target_logp"):
        assert name in syms and hasattr(L, name), name
    # the declarations cite the reference lines they replace
    comment = hdr[:hdr.index("typedef struct gnnlm_dense_softmax")].rsplit("/*", 1)[1]
    for cite in ("Replaces", "fairseq/models/transformer.py:843-852", ":1081-1085", "fairseq/sequence_scorer.py:48-53,89"):
        assert cite in comment, cite
    after = hdr[hdr.index("typedef struct gnnlm_dense_softmax"):]
    assert after.index("gnnlm_dense_workspace_bytes(") < after.index("gnnlm_dense_target_logp(") < after.index("kNN-LM distance-softmax")


def test_struct_mirror_matches_the_c_size():
    from gnnlm_amd import _lib
    L = _lib.lib()
    st = _lib.STRUCTS["gnnlm_dense_softmax_t"]
    assert [f[0] for f in st._fields_] == ["d", "vocab", "gemm_precision", "route", "w", "ldw", "bias"]
    assert L.gnnlm_sizeof(b"gnnlm_dense_softmax_t") == ctypes.sizeof(st) == 40


def _desc(**kw):
    from gnnlm_amd import _lib
    w = _lib.gnnlm_dense_softmax_t()
    w.d, w.vocab, w.gemm_precision, w.route, w.w, w.ldw, w.bias = 64, 205, 0, 0, 16, 64, None
    for k_, v in kw.items():
        setattr(w, k_, v)
    return w


@pytest.mark.parametrize("kw, msg", [
    (dict(d=6, ldw=8), "d must be"),
    (dict(vocab=0), "vocab"),
    (dict(gemm_precision=4), "gemm_precision"),
    (dict(route=3), "route"),
    (dict(route=1, vocab=513), "vocab <= 512"),
    (dict(route=1, gemm_precision=1), "precision 0 or 3"),
    (dict(w=None), "null weight"),
])
def test_invalid_descriptors_are_refused_before_any_pointer_is_touched(kw, msg):
    from gnnlm_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)                                        # (never dereferenced)
    w = _desc(**kw)
    rc = L.gnnlm_dense_target_logp(ctypes.byref(w), one, 64, one, 4, one, one, 1 << 30, None)
    assert rc != 0 and msg in L.gnnlm_last_error().decode(), (kw, L.gnnlm_last_error())


@pytest.mark.parametrize("bias", [None, 16])
def test_a_workspace_that_is_too_small_is_refused(bias):
    from gnnlm_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    w = _desc(route=2, vocab=1000, bias=bias)
    n = 300
    need, least = L.gnnlm_dense_workspace_bytes(ctypes.byref(w), n), L.gnnlm_dense_workspace_bytes_min(ctypes.byref(w), n)
    assert 0 < least <= need and (least < need) == (bias is not None)            # only the logits of the bias path can be cut
    for ws, size in ((one, least - 1), (one, 0), (None, need)):
        rc = L.gnnlm_dense_target_logp(ctypes.byref(w), one, 64, one, n, one, ws, size, None)
        assert rc != 0 and "workspace too small" in L.gnnlm_last_error().decode(), (size, L.gnnlm_last_error())
    # the one-launch route needs none
    assert L.gnnlm_dense_workspace_bytes(ctypes.byref(_desc(route=1)), n) == 0
    assert L.gnnlm_dense_workspace_bytes(ctypes.byref(_desc(gemm_precision=3)), n) == 0    # auto at V = 205 under fp16: one launch
    assert L.gnnlm_dense_workspace_bytes(ctypes.byref(_desc()), n) > 0                     # auto at f32: the general route
    assert L.gnnlm_dense_workspace_bytes(ctypes.byref(_desc(gemm_precision=1)), n) > 0     # split-bf16: the general route


def test_weights_from_state_dict():
    from gnnlm_amd.dense_softmax import weights_from_state_dict
    emb, out, bias = torch.randn(7, 8), torch.randn(7, 8), torch.randn(7)
    sd = {"decoder.embed_tokens.weight": emb, "decoder.embed_out": out}
    w, b = weights_from_state_dict(sd, Namespace(share_decoder_input_output_embed=True))
    assert w is emb and b is None
    w, b = weights_from_state_dict(sd, Namespace(share_decoder_input_output_embed=False))
    assert w is out and b is None
    w, b = weights_from_state_dict(sd, Namespace())                                # the flag's default is unshared
    assert w is out
    w, b = weights_from_state_dict(dict(sd, **{"decoder.xl_bias": bias}), Namespace(share_decoder_input_output_embed=True))
    assert w is emb and b is bias
    w, b = weights_from_state_dict({"m.embed_out": out, "m.xl_bias": bias}, Namespace(), prefix="m.")
    assert w is out and b is bias
    for args in (Namespace(share_decoder_input_output_embed=True), Namespace()):
        with pytest.raises(ValueError) as err:
            weights_from_state_dict({"decoder.hgt_decoder.x": emb}, args)
        assert "decoder.embed_tokens.weight" in str(err.value) and "decoder.embed_out" in str(err.value)


def test_package_exports_the_class():
    import gnnlm_amd
    from gnnlm_amd.dense_softmax import DenseSoftmax
    assert gnnlm_amd.DenseSoftmax is DenseSoftmax
    for attr in ("target_log_prob", "release_stream_state", "from_state_dict"):
        assert hasattr(DenseSoftmax, attr)


def test_fixture_equals_the_float64_restatement():
    """Every target column the reference returned == the float64 restatement of output_layer + log_softmax, mixed in probability
    space at the ratio, within the project's 2e-5 for log-probabilities against float64: yardstick and fixture agree."""
    g = np.load(GOLDEN)
    V, d = g["embed_tokens"].shape
    tgt = g["target"].reshape(-1)
    assert (V, d) == (205, 64) and g["target"].shape == (2, 40) and 0 in tgt and V - 1 in tgt
    assert [float(a) for a in g["ratios"]] == [0.0, 0.1, 0.5, 0.9] and np.abs(g["xl_bias"]).min() > 0
    x, h = g["x"].reshape(-1, d), g["h"].reshape(-1, d)
    for kind, with_bias in ref.CASES:
        w, b = ref.case_weights(g, kind, with_bias)
        gnn, base = ref.dense_logp64(x, w, b, tgt), ref.dense_logp64(h, w, b, tgt)
        assert np.abs(gnn - base).max() > 1.0 and gnn.std() > 1.0                  # the branches differ, the logits are not flat
        name = ref.case_name(kind, with_bias)
        for a in list(g["ratios"]) + [1.0]:
            err = np.abs(g[f"logp.{name}.{float(a)}"].reshape(-1) - ref.mix64(base, gnn, float(a))).max()
            print(f"{name} ratio {a}: max |fixture - float64| = {err:.2e}")
            assert err < 2e-5
        # on this branch the reference's ratio 1 does not raise (no math.log(1 - ratio)): it scores the base LM alone
        assert str(g[f"alpha_1_raises.{name}"]) == ""
    assert np.abs(g["logp.shared.bias.0.0"] - g["logp.shared.nobias.0.0"]).max() > 0.1            # the bias is felt
    assert np.abs(g["logp.shared.nobias.0.0"] - g["logp.unshared.nobias.0.0"]).max() > 0.1        # and so is the weight's choice
