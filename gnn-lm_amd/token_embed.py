"""The token-embedding table of ``--reinit-nfeat`` -- mirror of ``self.embed_tokens(labels)`` as the graph decoder calls it
(fairseq/models/transformer.py:1046-1048: ``embed_tokens`` directly, no ``embed_scale``, no positions, no ``project_in_dim``).

The reference evaluates the embedding module per batch of labels.  A neighbour node's feature is a function of its label
alone, so the whole module is materialised ONCE at load as ``E [V, d]`` float32 and every consumer is a row gather
(``ops.token_gather``, the star edges of layer 0 through ``ops.neighbor_labels``):

  * adaptive input (fairseq/modules/adaptive_input.py:63-74; wiki103, One Billion Word): for band ``i`` with
    ``cutoff[i-1] <= y < cutoff[i]`` the row is ``embeddings.i.0.weight[y - cutoff[i-1]] @ embeddings.i.1.weight.T`` -- band 0
    included, which has a projection of its own (``embeddings.0.1.weight [d, d]``) that the tied adaptive softmax never reads.
    One ``ops.gemm_nt`` per band under the model's GEMM precision (``--fp16``: both operands rounded to float16, f32
    accumulation; the table stays float32);
  * plain embedding (``--arch transformer_lm``: enwik8): the row is ``decoder.embed_tokens.weight[y]``, the weight itself.
"""
import logging
from typing import List, Optional

import torch

logger = logging.getLogger(__name__)


def band_weights(sd, prefix="decoder."):
    """-> ("adaptive", [(emb_i [size_i, dim_i], proj_i [d, dim_i]), ...]) or ("plain", weight [V, d]) from a reference state dict
    (host tensors are fine: nothing here needs a device)."""
    k_plain = f"{prefix}embed_tokens.weight"
    k_band = f"{prefix}embed_tokens.embeddings.{{}}.{{}}.weight"
    if k_band.format(0, 0) in sd:
        bands, i = [], 0
        while k_band.format(i, 0) in sd:
            if k_band.format(i, 1) not in sd:
                raise ValueError(f"--reinit-nfeat: the checkpoint has {k_band.format(i, 0)!r} but not its projection "
                                 f"{k_band.format(i, 1)!r} (adaptive_input.py:41-44: every band, band 0 included, is Embedding + Linear)")
            emb, proj = sd[k_band.format(i, 0)], sd[k_band.format(i, 1)]
            if emb.dim() != 2 or proj.dim() != 2 or proj.shape[1] != emb.shape[1]:
                raise ValueError(f"--reinit-nfeat: band {i} has embedding {tuple(emb.shape)} and projection {tuple(proj.shape)}; "
                                 "expected [size, dim] and [d, dim]")
            if bands and proj.shape[0] != bands[0][1].shape[0]:
                raise ValueError(f"--reinit-nfeat: band {i} projects to {proj.shape[0]} dimensions, band 0 to {bands[0][1].shape[0]}")
            bands.append((emb, proj))
            i += 1
        return "adaptive", bands
    if k_plain in sd:
        w = sd[k_plain]
        if w.dim() != 2:
            raise ValueError(f"--reinit-nfeat: {k_plain!r} is {tuple(w.shape)}, expected [V, d]")
        return "plain", w
    raise ValueError(f"--reinit-nfeat needs the input embedding: the checkpoint holds neither {k_band.format(0, 0)!r} (adaptive input) "
                     f"nor {k_plain!r} (plain embedding)")


def check_bands(bands, cutoff: Optional[List[int]]):
    """The band sizes against ``--adaptive-input-cutoff`` (adaptive_input.py:26-39), when the checkpoint's args carry it."""
    if not cutoff:
        return
    sizes = [e.shape[0] for e, _ in bands]
    bounds = [0] + [int(c) for c in cutoff]
    for i, size in enumerate(sizes[:-1]):
        if i + 1 >= len(bounds) or bounds[i + 1] - bounds[i] != size:
            raise ValueError(f"--reinit-nfeat: band {i} of embed_tokens holds {size} rows, adaptive_input_cutoff {cutoff} says "
                             f"{bounds[i + 1] - bounds[i] if i + 1 < len(bounds) else 'no such band'}")


class TokenEmbedding:
    """``E [V, d]`` float32 on the device; ``kind`` is "adaptive" or "plain"; ``precision`` the GEMM precision (a value of
    ``ops.PRECISIONS``) the adaptive table was built under -- None for the plain table, which is a copy under every precision."""

    def __init__(self, table: torch.Tensor, kind: str, precision=None):
        assert table.dim() == 2 and table.dtype == torch.float32 and table.is_contiguous() and table.shape[1] % 4 == 0
        self.table, self.kind, self.precision = table, kind, precision

    @property
    def vocab(self):
        return self.table.shape[0]

    @property
    def d(self):
        return self.table.shape[1]

    @classmethod
    def from_state_dict(cls, sd, args=None, device=None, precision=0, prefix="decoder."):
        kind, w = band_weights(sd, prefix)
        if device is None or torch.device(device).type != "cuda":
            from ._lib import GnnlmError
            raise GnnlmError("TokenEmbedding needs a device: the table is built by the HIP GEMM, gnnlm_amd has no CPU fallback")
        if kind == "plain":
            table = w.detach().to(device, torch.float32).contiguous()
        else:
            from . import ops
            cut = getattr(args, "adaptive_input_cutoff", None) if args is not None else None
            check_bands(w, [int(c) for c in str(cut).split(",")] if cut else None)
            d, V = w[0][1].shape[0], sum(e.shape[0] for e, _ in w)
            table = torch.empty(V, d, device=device, dtype=torch.float32)
            row = 0
            f = lambda t: torch.nn.functional.pad(t.detach().float(), (0, (-t.shape[1]) % 4)).to(device).contiguous()   # K % 4: zero columns, exact
            for emb, proj in w:
                ops.gemm_nt(f(emb), f(proj), out=table[row:row + emb.shape[0]], precision=precision)
                row += emb.shape[0]
        if table.shape[1] % 4:
            raise ValueError(f"--reinit-nfeat: the embedding dimension {table.shape[1]} must be a multiple of 4")
        logger.info("--reinit-nfeat: token-embedding table %s (%s), %d x %d float32 = %.1f MB", kind,
                    "emb_i @ proj_i^T per band" if kind == "adaptive" else "embed_tokens.weight", table.shape[0], table.shape[1],
                    table.numel() * 4 / 1e6)
        return cls(table, kind, None if kind == "plain" else int(precision))
