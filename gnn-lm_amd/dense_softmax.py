"""Plain (non-adaptive) output layer, target log-probability only -- mirror of ``TransformerDecoder.output_layer`` with
``adaptive_softmax is None`` (fairseq/models/transformer.py:843-852: ``F.linear(features, embed_tokens.weight | embed_out)
[+ xl_bias]``), the ``log_softmax`` of ``get_normalized_probs`` (:1081-1085) and ``gather_target_probs``
(fairseq/sequence_scorer.py:48-53,89).

This is the head of a ``--arch transformer_lm`` checkpoint: the enwik8 recipe (gnnlm_scripts/enwik8/prepare_enwik8.sh:34-42,
Transformer-XL's last layer with its ``xl_bias``) and any model trained with ``--share-decoder-input-output-embed``.  The
reference materialises the dense ``[B, T, V]`` logits and gathers one column; here the target's log-probability leaves the GEMM
directly (csrc/dense_logp.hip).  ``DenseSoftmax`` has the surface of ``AdaptiveSoftmax`` that the model, the engine and the
scorer use, so it goes into the same slot.
"""
import ctypes
from typing import Optional

import torch

from . import _lib

ROUTES = {0: "auto", 1: "one-launch", 2: "general"}


def weights_from_state_dict(sd, args, prefix="decoder."):
    """-> (weight [V, d], bias [V] or None) of a reference state dict, on the host: ``embed_tokens.weight`` when the checkpoint
    shares input and output embeddings (``share_decoder_input_output_embed``), else ``embed_out`` (transformer.py:847-850); the
    bias is ``xl_bias`` when the key is present (:665-668)."""
    shared = bool(getattr(args, "share_decoder_input_output_embed", False))
    k_shared, k_out = f"{prefix}embed_tokens.weight", f"{prefix}embed_out"
    key = k_shared if shared else k_out
    if key not in sd:
        raise ValueError(f"no dense output layer in the checkpoint: share_decoder_input_output_embed = {shared} needs {key!r}; the "
                         f"state dict must hold {k_shared!r} (shared) or {k_out!r} (unshared)")
    bias = sd.get(f"{prefix}xl_bias")
    return sd[key], bias


class DenseSoftmax:
    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, device=None):
        """weight [V, d] (d % 4 == 0), bias [V] or None (``xl_bias``: added in f32 under every precision)."""
        assert weight.dim() == 2 and weight.shape[1] % 4 == 0, "weight must be [V, d] with d % 4 == 0"
        device = weight.device if device is None else device
        f = lambda t: t.detach().to(device, torch.float32).contiguous()
        self.weight = f(weight)
        self.bias = None if bias is None else f(bias.reshape(-1))
        assert self.bias is None or self.bias.shape[0] == self.weight.shape[0]
        self.vocab, self.d = self.weight.shape
        w = _lib.gnnlm_dense_softmax_t()
        w.d, w.vocab = self.d, self.vocab
        w.w, w.ldw = self.weight.data_ptr(), self.weight.stride(0)
        w.bias = self.bias.data_ptr() if self.bias is not None else None
        self._w = w
        self._ws = None
        self.gemm_precision = 0     # 0 exact f32 MFMA | 1 bf16x3 | 2 bf16x6 | 3 fp16 operands, f32 accumulate (--fp16)
        self.route = 0              # 0 auto (one launch for V <= 384 under fp16, else general) | 1 the one-launch kernel (V <= 512, precision 0 or 3) | 2 the general route
        self.small_workspace = False   # the least workspace the library accepts: 128-row logit chunks for the bias (tests, A/B)

    @classmethod
    def from_state_dict(cls, sd, args, device, prefix="decoder."):
        weight, bias = weights_from_state_dict(sd, args, prefix)
        return cls(weight, bias, device)

    def route_name(self) -> str:
        """The route a call takes now (what ``auto`` resolves to)."""
        r = self.route
        if r == 0:
            r = 1 if self.vocab <= 384 and self.gemm_precision == 3 else 2          # (csrc/dense_logp.hip::dense_route)
        return ROUTES[r]

    def release_stream_state(self, keep=()):
        """Free the scratch arenas of every stream but `keep` (raw handles): see HGT.release_stream_state."""
        if self._ws:
            for k_ in [k_ for k_ in self._ws if k_ not in set(keep)]:
                del self._ws[k_]

    def log_probs(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [n, d] f32 -> log_softmax(x . w^T + bias) [n, V] f32 (transformer.py:843-852,1081-1085): the logits are written into
        the result by the GEMM and finished in place (csrc/dense_dist.hip); ``route`` plays no part."""
        from . import ops
        self._w.gemm_precision = self.gemm_precision
        key = (_lib.raw_stream(), "dense")                      # one arena per stream, beside target_log_prob's
        if self._ws is None:
            self._ws = {}
        need = _lib.lib().gnnlm_dense_log_probs_workspace_bytes(ctypes.byref(self._w), x.shape[0])
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, device=x.device, dtype=torch.uint8)
        return ops.dense_log_probs(self._w, x, out=out, workspace=ws)

    def target_log_prob(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """x [n, d] f32 (row stride % 4 == 0), target [n] int64 -> log p(target | x) [n]; -inf for a target outside [0, V)."""
        n = x.shape[0]
        if x.stride(-1) != 1 or x.stride(0) % 4 or x.stride(0) < self.d:
            x = x.contiguous()
        target = target.contiguous()
        assert x.dtype == torch.float32 and target.dtype == torch.int64 and x.shape[1] == self.d
        if not x.is_cuda:
            raise _lib.GnnlmError("gnnlm_amd kernels need device (HIP) tensors; there is no CPU fallback")
        out = torch.empty(n, device=x.device, dtype=torch.float32)
        if n == 0:
            return out
        self._w.gemm_precision, self._w.route = self.gemm_precision, self.route
        L = _lib.lib()
        size = L.gnnlm_dense_workspace_bytes_min if self.small_workspace else L.gnnlm_dense_workspace_bytes
        need = size(ctypes.byref(self._w), n)
        ws = None
        if need:
            key = _lib.raw_stream()                             # one arena per stream
            if self._ws is None:
                self._ws = {}
            ws = self._ws.get(key)
            if ws is None or ws.numel() < need or (self.small_workspace and ws.numel() != need):
                ws = self._ws[key] = torch.empty(need, device=x.device, dtype=torch.uint8)
        _lib.check(L.gnnlm_dense_target_logp(ctypes.byref(self._w), ctypes.c_void_p(x.data_ptr()), x.stride(0), _lib.ptr(target), n,
                                             _lib.ptr(out), _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream()),
                   "gnnlm_dense_target_logp")
        return out
