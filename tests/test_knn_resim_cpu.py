"""What the similarity recompute (`gnnlm_knn_recompute_sims`, `--knn-sim-func ip | l2`) promises without a device."""
import ctypes
import inspect

import pytest
import torch


def test_host_tensors_are_refused():
    """No CPU fallback: host tensors raise GnnlmError, in indexed and in direct mode."""
    from gnnlm_amd import ops
    from gnnlm_amd._lib import GnnlmError
    q, ids, keys = torch.zeros(3, 16), torch.zeros(3, 4, dtype=torch.int64), torch.zeros(12, 16, dtype=torch.float16)
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.knn_recompute_sims(q, ids, keys, "ip")
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.knn_recompute_sims(q, None, keys, "l2")
    with pytest.raises(GnnlmError, match="no CPU fallback"):
        ops.knn_recompute_sims(q, ids, keys, "ip", normalize_keys=True, out=torch.zeros(3, 4))


def test_parser_keeps_its_defaults():
    from gnnlm_amd import eval_lm
    parser = eval_lm.get_parser
    args = parser().parse_args(["data", "--path", "x.pt"])
    assert args.knn_sim_func == "do_not_recomp_ip" and not args.knnlm
    for fn in ("ip", "l2"):
        assert parser().parse_args(["data", "--path", "x.pt", "--knnlm", "--knn-sim-func", fn]).knn_sim_func == fn


def test_descriptor_agrees_across_header_binding_and_library():
    from gnnlm_amd import _lib
    st = _lib.STRUCTS["gnnlm_knn_resim_t"]
    assert [f[0] for f in st._fields_] == ["queries", "ldq", "ids", "ld_ids", "keys", "keys_itemsize", "ld_keys", "n_rows", "d", "n", "k",
                                           "metric", "normalize_keys", "out", "ld_out"]
    L = _lib.lib()
    assert L.gnnlm_sizeof(b"gnnlm_knn_resim_t") == ctypes.sizeof(st) > 0
    assert "gnnlm_knn_recompute_sims" in _lib.exported_symbols() and hasattr(L, "gnnlm_knn_recompute_sims")
    assert _lib.ABI_VERSION == 12 and L.gnnlm_abi_version() == 12
    names = []
    while L.gnnlm_kernel_name(len(names)) is not None:
        names.append(L.gnnlm_kernel_name(len(names)).decode())
    assert names[-1] == "knn_resim_kernel" and names[16] == "knn_interp_grid_kernel"


def test_engine_and_model_arguments():
    """The new arguments default to what every current call does."""
    from gnnlm_amd.engine import GnnLmEngine
    from gnnlm_amd.knn_model import KNNModel
    for fn in (GnnLmEngine.score, GnnLmEngine.score_begin):
        sig = inspect.signature(fn)
        assert sig.parameters["knn_keys"].default is None and sig.parameters["knn_sim_func"].default == "do_not_recomp_ip"
    assert callable(KNNModel.keys_home)
