"""gnnlm_amd -- MI355X-native implementation of the GNN+kNN eval hot path of ShannonAI/GNN-LM.

Host-side mirror of the reference's Python operator surface (DataStore, TorchPQCodec, HGT,
KNNModel, SequenceScorer, eval_lm) over the C ABI of libgnnlm_hip.so (include/gnnlm.h).
"""
__version__ = "0.1.0"

__all__ = ["DenseSoftmax"]


def __getattr__(name):
    # (lazy: importing the package must not load torch or the shared library)
    if name == "DenseSoftmax":
        from .dense_softmax import DenseSoftmax
        return DenseSoftmax
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
