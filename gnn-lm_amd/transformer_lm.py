"""``TransformerLM`` -- the base transformer language model on the device: mirror of ``TransformerDecoder.extract_features``
(fairseq/models/transformer.py:700-841) over ``TransformerDecoderLayer.forward`` (fairseq/modules/transformer_layer.py:223-331)
for a ``--arch transformer_lm*`` checkpoint in eval mode (decoder only, ``decoder_normalize_before`` forced by
transformer_lm.py:225, dropout and layer-drop the identity).

It is the front of the pipeline: its features are ``{split}_dstore/keys.npy`` (``--use-precompute-feat``), the keys the kNN
index is built over and the queries of the kNN command.  Samples are PACKED blocks (``ragged.RaggedBatch``): no padding, no
padding mask -- the token stream is assumed to hold no ``<pad>``, as a binarised corpus does.

The forward is ONE call of the C ABI (``gnnlm_transformer_lm_forward``, include/gnnlm.h), which enqueues the embed kernel, the
library's GEMMs, ``gnnlm_causal_attn_varlen``, LayerNorm and the activation on the current stream.  Weights are prepared once at
load: q | k | v concatenated into ``Wqkv [3d, d]`` with the ``d_k^-0.5`` of ``q *= self.scaling`` folded into the q rows (exact
when d_k is a power of 4, one more float32 rounding of those weights otherwise), the adaptive-input table materialised by
``TokenEmbedding``, the sinusoidal positions built on the host exactly as ``SinusoidalPositionalEmbedding.get_embedding`` does.
There is no CPU fallback.
"""
import ctypes
import math
from argparse import Namespace

import torch

from . import _lib, ops
from .adaptive_softmax import AdaptiveSoftmax
from .dense_softmax import DenseSoftmax
from .token_embed import TokenEmbedding

ACTS = {"relu": 0, "gelu": 1}
PAD_IDX = 1                     # fairseq Dictionary: bos 0, pad 1, eos 2, unk 3


def sinusoidal_table(rows, d, pad_idx=PAD_IDX):
    """``SinusoidalPositionalEmbedding.get_embedding(rows, d, pad_idx)`` (sinusoidal_positional_embedding.py:36-60) in float32 on
    the host, operation for operation; row ``pad_idx`` is zero.  A row does not depend on ``rows``: a longer table extends a shorter."""
    half = d // 2
    emb = math.log(10000) / (half - 1)
    emb = torch.exp(torch.arange(half, dtype=torch.float) * -emb)
    emb = torch.arange(rows, dtype=torch.float).unsqueeze(1) * emb.unsqueeze(0)
    emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1).view(rows, -1)
    if d % 2 == 1:
        emb = torch.cat([emb, torch.zeros(rows, 1)], dim=1)
    if pad_idx is not None and pad_idx < rows:
        emb[pad_idx, :] = 0
    return emb


def _get(args, name, default=None):
    v = getattr(args, name, default)
    return default if v is None else v


def check_args(args):
    """The settings this build does not compute are refused by name (``ValueError``), never approximated."""
    d = int(args.decoder_embed_dim)
    for name in ("decoder_input_dim", "decoder_output_dim"):
        v = int(_get(args, name, d))
        if v != d:
            raise ValueError(f"{name} = {v} != decoder_embed_dim = {d}: project_in_dim / project_out_dim are not built")
    if _get(args, "character_embeddings", False):
        raise ValueError("character_embeddings (CharacterTokenEmbedder) is not built")
    act = _get(args, "activation_fn", "relu")
    if act not in ACTS:
        raise ValueError(f"activation_fn = {act!r}: only relu and gelu are built")
    return d, act                                             # (decoder_layerdrop: eval mode keeps every layer, transformer.py:799)


def fused_qkv(sd, prefix, d):
    """-> (Wqkv [3d, d], bqkv [3d]) of one layer from either attention layout: the old fused ``in_proj_weight`` / ``in_proj_bias``
    or the split ``q_proj`` / ``k_proj`` / ``v_proj`` (upgrade_state_dict_named, multihead_attention.py: q rows first, then k, then v)."""
    if prefix + "in_proj_weight" in sd:
        w = sd[prefix + "in_proj_weight"].detach().float()
        b = sd[prefix + "in_proj_bias"].detach().float() if prefix + "in_proj_bias" in sd else torch.zeros(3 * d)
    elif prefix + "q_proj.weight" in sd:
        w = torch.cat([sd[prefix + f"{n}_proj.weight"].detach().float() for n in "qkv"], 0)
        b = torch.cat([sd[prefix + f"{n}_proj.bias"].detach().float() if prefix + f"{n}_proj.bias" in sd else torch.zeros(d) for n in "qkv"], 0)
    else:
        raise ValueError(f"no self-attention weights under {prefix!r}: neither in_proj_weight nor q_proj / k_proj / v_proj")
    if tuple(w.shape) != (3 * d, d) or tuple(b.shape) != (3 * d,):
        raise ValueError(f"{prefix}: q | k | v weights are {tuple(w.shape)} / {tuple(b.shape)}, expected {(3 * d, d)} / {(3 * d,)}")
    return w.clone(), b.clone()


class KVCache:
    """The K/V cache of :meth:`TransformerLM.prefill` / :meth:`TransformerLM.step` (``gnnlm_kv_cache_t``): ``k`` / ``v`` f32
    [L, B, cap, d], ``len`` int32 [B] (keys held per sequence), ``done`` int32 [B], ``n_bad`` int32 [1] -- all on the device -- and
    ``steps``, the HOST's upper bound on ``len.max()`` (the prompts' longest block plus the steps taken since): what ``max_len`` of the
    C entries is computed from, so that no step has to read ``len`` back."""

    def __init__(self, L, B, cap, d, device):
        self.k = torch.empty(L, B, cap, d, device=device, dtype=torch.float32)
        self.v = torch.empty(L, B, cap, d, device=device, dtype=torch.float32)
        self.len = torch.zeros(B, device=device, dtype=torch.int32)
        self.done = torch.zeros(B, device=device, dtype=torch.int32)
        self.n_bad = torch.zeros(1, device=device, dtype=torch.int32)
        self.L, self.B, self.cap, self.d, self.steps = L, B, cap, d, 0

    def desc(self):
        return ops.kv_cache_desc(self.k, self.v, self.len, self.done, self.n_bad)

    def reset(self):
        self.len.zero_(), self.done.zero_(), self.n_bad.zero_()
        self.steps = 0

    def prompt_view(self, beam):
        """Beam search: the ``B / beam`` sequences ``0, beam, 2 * beam, ..`` of this cache as a cache of their own (the same memory,
        ``ld_seq`` multiplied by ``beam``) -- what the prompts of ``B / beam`` sentences are prefilled into, once per sentence.  Its
        ``len`` is a tensor of its own: :meth:`spread` copies it to the ``beam`` slots of every sentence."""
        if beam < 1 or self.B % beam:
            raise ValueError(f"prompt_view: the cache's {self.B} sequences are no multiple of beam {beam}")
        view = object.__new__(KVCache)
        view.k, view.v = self.k[:, ::beam], self.v[:, ::beam]
        view.len = torch.zeros(self.B // beam, device=self.k.device, dtype=torch.int32)
        view.done, view.n_bad = None, self.n_bad
        view.L, view.B, view.cap, view.d, view.steps = self.L, self.B // beam, self.cap, self.d, 0
        return view

    def spread(self, view):
        """After a prefill into :meth:`prompt_view`: every slot of a sentence holds the sentence's ``len``."""
        beam = self.B // view.B
        self.len.view(view.B, beam).copy_(view.len.unsqueeze(1).expand(view.B, beam))
        self.steps = view.steps


class TransformerLM:
    def __init__(self, embed, layers, H, act="relu", scale=None, pos=None, learned_pos=False, ln_emb=None, ln_out=None, head=None,
                 device=None, precision=None, pad_idx=PAD_IDX, ln_eps=1e-5):
        """embed: ``TokenEmbedding`` (E [V, d] on the device).  layers: list of dicts of HOST or device float32 tensors with the
        keys ln1_g ln1_b wqkv bqkv wo bo ln2_g ln2_b w1 b1 w2 b2 -- UNSCALED (the fold of d_k^-0.5 happens here).  pos: the position
        table [rows, d] (host or device) or None; ``learned_pos`` False lets it grow on demand (sinusoidal).  ln_emb / ln_out:
        (weight, bias) or None.  head: ``AdaptiveSoftmax`` / ``DenseSoftmax`` or None."""
        device = embed.table.device if device is None else torch.device(device)
        if device.type != "cuda":
            raise _lib.GnnlmError("TransformerLM needs a device: gnnlm_amd has no CPU fallback")
        self.device, self.embed, self.head = device, embed, head
        self.d, self.H, self.L = embed.d, int(H), len(layers)
        if self.L < 1 or self.d % self.H or self.d // self.H not in (16, 32, 64, 128):
            raise ValueError(f"TransformerLM: d / H = {self.d} / {self.H} must be one of 16, 32, 64, 128 (gnnlm_causal_attn_varlen)")
        if act not in ACTS:
            raise ValueError(f"activation_fn = {act!r}: only relu and gelu are built")
        self.act, self.pad_idx, self.ln_eps = act, int(pad_idx), float(ln_eps)
        self.scale = math.sqrt(self.d) if scale is None else float(scale)
        f = lambda t: None if t is None else t.detach().to(device, torch.float32).contiguous()
        self.learned_pos = bool(learned_pos)
        self.pos = f(pos)
        self.ln_emb = None if ln_emb is None else (f(ln_emb[0]), f(ln_emb[1]))
        self.ln_out = None if ln_out is None else (f(ln_out[0]), f(ln_out[1]))
        scaling = (self.d // self.H) ** -0.5
        self.layers = []
        for w in layers:
            w = dict(w)
            wqkv, bqkv = w["wqkv"].detach().float().clone(), w["bqkv"].detach().float().clone()
            wqkv[:self.d] *= scaling                          # q = (x Wq^T + bq) * scaling (multihead_attention.py)
            bqkv[:self.d] *= scaling
            w["wqkv"], w["bqkv"] = wqkv, bqkv
            self.layers.append({k_: f(v) for k_, v in w.items()})
        self.ffn = int(self.layers[0]["w1"].shape[0])
        for w in self.layers:
            shapes = {"wqkv": (3 * self.d, self.d), "bqkv": (3 * self.d,), "wo": (self.d, self.d), "bo": (self.d,), "w1": (self.ffn, self.d),
                      "b1": (self.ffn,), "w2": (self.d, self.ffn), "b2": (self.d,), "ln1_g": (self.d,), "ln1_b": (self.d,),
                      "ln2_g": (self.d,), "ln2_b": (self.d,)}
            for k_, shp in shapes.items():
                if tuple(w[k_].shape) != shp:
                    raise ValueError(f"TransformerLM: layer tensor {k_} is {tuple(w[k_].shape)}, expected {shp}")
        self._c_layers = (_lib.gnnlm_tlm_layer_t * self.L)()
        for cl, w in zip(self._c_layers, self.layers):
            for k_ in w:
                setattr(cl, k_, w[k_].data_ptr())
        self.gemm_precision = 0
        if precision is not None:
            self.precision = precision
        self._ws = {}
        self.n_bad = torch.zeros(1, device=device, dtype=torch.int32)      # token ids outside [0, V), over every call so far

    # ---- precision: the orchestrator's GEMMs and the head's, one setting (`eval_lm --fp16`)
    @property
    def precision(self):
        mods = [self] + ([self.head] if self.head is not None else [])
        return ops.precision_name(*(m.gemm_precision for m in mods))

    @precision.setter
    def precision(self, value):
        v = ops.precision_value(value)
        self.gemm_precision = v
        if self.head is not None:
            self.head.gemm_precision = v

    def _positions(self, max_len):
        """The position table able to hold a block of ``max_len`` tokens.  Sinusoidal: grown as the reference grows it
        (sinusoidal_positional_embedding.py:70-75).  Learned: fixed -- a longer block is refused (C side, before any launch)."""
        if self.pos is None:
            return None
        need = self.pad_idx + 1 + int(max_len)
        if not self.learned_pos and need > self.pos.shape[0]:
            self.pos = sinusoidal_table(need, self.d, self.pad_idx).to(self.device).contiguous()
        return self.pos

    def _desc(self, P):
        m = _lib.gnnlm_tlm_t()
        m.L, m.d, m.H, m.ffn, m.act, m.precision = self.L, self.d, self.H, self.ffn, ACTS[self.act], self.gemm_precision
        m.ln_eps, m.scale = self.ln_eps, self.scale
        E = self.embed.table
        m.E, m.ld_e, m.n_vocab, m.pad_idx = E.data_ptr(), E.stride(0), E.shape[0], self.pad_idx
        if P is not None:
            m.P, m.ld_p, m.p_rows = P.data_ptr(), P.stride(0), P.shape[0]
        if self.ln_emb is not None:
            m.ln_emb_g, m.ln_emb_b = self.ln_emb[0].data_ptr(), self.ln_emb[1].data_ptr()
        if self.ln_out is not None:
            m.ln_out_g, m.ln_out_b = self.ln_out[0].data_ptr(), self.ln_out[1].data_ptr()
        m.layers = ctypes.addressof(self._c_layers)
        return m

    def extract_features(self, tokens, block_off, want_inner=True, want_ffn_input=True, check=True):
        """tokens int64 [n_tok] (device), ``block_off`` a ``ragged.RaggedBatch`` or offsets [n_blocks + 1] ->
        ``(x [n_tok, d], {"inner_states": [inner_states[-1]], "last_ffn_input": ...})`` -- x after the final layer_norm when the model
        has one, ``inner_states[-1]`` before it, ``last_ffn_input`` the last layer's ``final_layer_norm`` output.
        ``check``: read the count of token ids outside the vocabulary together with the results (one synchronisation) and raise;
        a driver passes False and calls :meth:`check_tokens` once at the end."""
        return self._forward(tokens, block_off, want_inner, want_ffn_input, check, None)

    def new_cache(self, B, cap):
        """An empty :class:`KVCache` for ``B`` sequences of up to ``cap`` tokens (prompt + continuation).  A sinusoidal position table
        is grown HERE, once, to the ``cap`` positions the cache can hold: no step builds or uploads a table.  (Growing replaces the
        table: a step captured in a graph before a LARGER cache was made must be captured again.)"""
        if B < 1 or cap < 1:
            raise ValueError("new_cache: B >= 1 and cap >= 1")
        self._positions(int(cap))
        return KVCache(self.L, int(B), int(cap), self.d, self.device)

    def prefill(self, tokens, block_off, cache, want_inner=True, want_ffn_input=True, check=True):
        """:meth:`extract_features` over packed prompts -- block b is sequence b of ``cache`` -- that also writes every layer's K' / V'
        rows into the cache and sets ``cache.len`` (``gnnlm_transformer_lm_prefill``).  Returns ``(x, extra)`` exactly as
        ``extract_features`` does, the same bits.  Refused before any launch: another number of blocks than ``cache.B``, a block longer
        than ``cache.cap``."""
        return self._forward(tokens, block_off, want_inner, want_ffn_input, check, cache)

    def step(self, tokens, cache, want_inner=True, want_ffn_input=True, max_len=None, src=None):
        """One decoding step (``gnnlm_transformer_lm_step``): ``tokens`` int64 [B] (device), token b is appended to sequence b ->
        ``(x [B, d], extra)`` as :meth:`extract_features` names them -- the mirror of ``extract_features(prev_output_tokens,
        incremental_state=...)``, which looks at the last token only (transformer.py:739-750).  Only enqueues: no host read, no
        synchronisation, no allocation beyond the outputs once the stream's workspace is large enough (the sinusoidal table was sized for
        ``cache.cap`` positions by :meth:`new_cache`, not here) -- a step can be captured in a graph.  ``max_len``: the host bound on ``len + 1`` (default ``cache.steps + 1``; for a captured step, the bound over every replay).
        A full cache and a position beyond a learned table are refused before any launch.
        ``src`` (beam search): the int32 [B, >= cap] table of cache slots -- key row u of sequence b is row u of sequence ``src[b, u]``
        (``gnnlm_transformer_lm_step_beam``, every layer through ``gnnlm_beam_attn``); without it the step is what it always was."""
        if tokens.dtype != torch.int64 or tokens.shape != (cache.B,):
            raise TypeError("step: tokens must be int64 [B]")
        ld_src = ops._src_table(src, cache.B, cache.cap, "step") if src is not None else 0
        self._need_device(tokens)
        bound = cache.steps + 1 if max_len is None else int(max_len)
        # the table of new_cache: cache.cap positions, whatever the bound (a cache made by hand is served here, once)
        m = self._desc(self._positions(cache.cap))
        c = cache.desc()
        io = _lib.gnnlm_tlm_step_io_t()
        io.tokens, io.max_len = tokens.data_ptr(), bound
        x, extra = self._outputs(io, cache.B, tokens.device, want_inner, want_ffn_input)
        L = _lib.lib()
        need = L.gnnlm_transformer_lm_step_workspace_bytes(ctypes.byref(m), ctypes.byref(c), ctypes.byref(io))
        ws = self._workspace(need, tokens.device)
        if src is None:
            _lib.check(L.gnnlm_transformer_lm_step(ctypes.byref(m), ctypes.byref(c), ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()),
                       "gnnlm_transformer_lm_step")
        else:
            _lib.check(L.gnnlm_transformer_lm_step_beam(ctypes.byref(m), ctypes.byref(c), ctypes.byref(io), ctypes.c_void_p(src.data_ptr()),
                                                        ld_src, _lib.ptr(ws), ws.numel(), _lib.stream()), "gnnlm_transformer_lm_step_beam")
        cache.steps += 1                                        # (replays of a captured step: the caller adds them)
        return x, extra

    @staticmethod
    def _need_device(tokens):
        if not tokens.is_cuda or not tokens.is_contiguous():
            raise _lib.GnnlmError("gnnlm_amd kernels need contiguous device (HIP) tensors; there is no CPU fallback")

    def _outputs(self, io, n, device, want_inner, want_ffn_input):
        """Allocate ``x`` [n, d] and the wanted ones of ``inner_states[-1]`` / ``last_ffn_input``, point ``io`` (either io descriptor) at
        them and at ``n_bad`` -> ``(x, extra)`` as :meth:`extract_features` returns them."""
        new = lambda: torch.empty(n, self.d, device=device, dtype=torch.float32)
        x = new()
        inner = new() if want_inner else None
        ffn_in = new() if want_ffn_input else None
        io.out = x.data_ptr()
        io.last_inner = inner.data_ptr() if inner is not None else None
        io.last_ffn_input = ffn_in.data_ptr() if ffn_in is not None else None
        io.n_bad = self.n_bad.data_ptr()
        extra = {"inner_states": [inner]}
        if ffn_in is not None:
            extra["last_ffn_input"] = ffn_in
        return x, extra

    def _workspace(self, need, device):
        key = _lib.raw_stream()                                 # one arena per stream
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, device=device, dtype=torch.uint8)
        return ws

    def _forward(self, tokens, block_off, want_inner, want_ffn_input, check, cache):
        from .ragged import as_ragged
        if tokens.dtype != torch.int64 or tokens.dim() != 1:
            raise TypeError("extract_features: tokens must be int64 [n_tok]")
        self._need_device(tokens)
        rg = as_ragged(block_off, tokens.device)
        n = rg.n_tok
        if n != tokens.shape[0]:
            raise ValueError(f"extract_features: {tokens.shape[0]} tokens, the blocks hold {n}")
        max_len = int(rg.lengths.max()) if rg.n_blocks else 0
        m = self._desc(self._positions(max_len))
        io = _lib.gnnlm_tlm_io_t()
        io.tokens, io.blocks, io.max_len = tokens.data_ptr(), rg.desc(), max_len
        x, extra = self._outputs(io, n, tokens.device, want_inner, want_ffn_input)
        L = _lib.lib()
        need = L.gnnlm_transformer_lm_workspace_bytes(ctypes.byref(m), ctypes.byref(io))
        ws = self._workspace(need, tokens.device)
        if cache is None:
            _lib.check(L.gnnlm_transformer_lm_forward(ctypes.byref(m), ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()),
                       "gnnlm_transformer_lm_forward")
        else:
            c = cache.desc()
            _lib.check(L.gnnlm_transformer_lm_prefill(ctypes.byref(m), ctypes.byref(io), ctypes.byref(c), _lib.ptr(ws), ws.numel(),
                                                      _lib.stream()), "gnnlm_transformer_lm_prefill")
            cache.steps = max_len
        if check:
            self.check_tokens()
        return x, extra

    def check_tokens(self):
        """Raise if any call so far met a token id outside [0, V) (such rows were computed from a zero embedding)."""
        bad = int(self.n_bad.item())
        if bad:
            self.n_bad.zero_()
            raise ValueError(f"{bad} token id(s) outside the vocabulary [0, {self.embed.vocab}) were fed to the base LM")

    def target_logp(self, x_rows, targets):
        """log p(targets | x_rows) [n] through the checkpoint's own head (tied adaptive softmax or the plain output layer)."""
        if self.head is None:
            raise ValueError("this TransformerLM was built without an output layer")
        return self.head.target_log_prob(x_rows, targets)

    def release_stream_state(self, keep=()):
        for k_ in [k_ for k_ in self._ws if k_ not in set(keep)]:
            del self._ws[k_]
        if self.head is not None and hasattr(self.head, "release_stream_state"):
            self.head.release_stream_state(keep=keep)

    # ---- loading
    @classmethod
    def from_state_dict(cls, sd, args, device, precision=None, prefix="decoder."):
        if not isinstance(args, Namespace):
            args = Namespace(**args)
        d, act = check_args(args)
        H, L = int(args.decoder_attention_heads), int(args.decoder_layers)
        pv = ops.precision_value(precision or "f32")
        embed = TokenEmbedding.from_state_dict(sd, args, device, pv, prefix)
        if embed.d != d:
            raise ValueError(f"embed_tokens has {embed.d} columns, decoder_embed_dim is {d} (project_in_dim is not built)")
        layers = []
        for i in range(L):
            p = f"{prefix}layers.{i}."
            if p + "encoder_attn.out_proj.weight" in sd:
                raise ValueError("the checkpoint has encoder attention: only decoder-only language models are built")
            wqkv, bqkv = fused_qkv(sd, p + "self_attn.", d)
            try:
                layers.append({"ln1_g": sd[p + "self_attn_layer_norm.weight"], "ln1_b": sd[p + "self_attn_layer_norm.bias"],
                               "wqkv": wqkv, "bqkv": bqkv, "wo": sd[p + "self_attn.out_proj.weight"], "bo": sd[p + "self_attn.out_proj.bias"],
                               "ln2_g": sd[p + "final_layer_norm.weight"], "ln2_b": sd[p + "final_layer_norm.bias"],
                               "w1": sd[p + "fc1.weight"], "b1": sd[p + "fc1.bias"], "w2": sd[p + "fc2.weight"], "b2": sd[p + "fc2.bias"]})
            except KeyError as e:
                raise ValueError(f"the checkpoint lacks {e.args[0]!r} (decoder_layers = {L})") from None
        if f"{prefix}layers.{L}.fc1.weight" in sd:
            raise ValueError(f"the checkpoint holds more than decoder_layers = {L} layers")
        pos, learned = None, bool(_get(args, "decoder_learned_pos", False))
        if not _get(args, "no_token_positional_embeddings", False):
            if learned:
                k_ = f"{prefix}embed_positions.weight"
                if k_ not in sd:
                    raise ValueError(f"decoder_learned_pos needs {k_!r}")
                pos = sd[k_]
            else:
                rows = int(_get(args, "max_target_positions", _get(args, "tokens_per_sample", 1024))) + PAD_IDX + 1
                pos = sinusoidal_table(rows, d, PAD_IDX)
        ln = lambda name: (sd[f"{prefix}{name}.weight"], sd[f"{prefix}{name}.bias"]) if f"{prefix}{name}.weight" in sd else None
        ln_out = None if _get(args, "no_decoder_final_norm", False) else ln("layer_norm")
        ln_emb = ln("layernorm_embedding") if _get(args, "layernorm_embedding", False) else None
        if _get(args, "layernorm_embedding", False) and ln_emb is None:
            raise ValueError(f"layernorm_embedding needs {prefix}layernorm_embedding.weight / .bias")
        # the head: the tied adaptive softmax, else the plain output layer (as GnnLmModel.from_checkpoint)
        if _get(args, "adaptive_softmax_cutoff") is not None and f"{prefix}adaptive_softmax.head.class_proj.weight" in sd:
            if embed.kind != "adaptive":
                raise ValueError("an adaptive softmax that is not tied to an adaptive input (tie_adaptive_weights) is not built")
            cut = [int(c) for c in str(args.adaptive_softmax_cutoff).split(",")]
            head = AdaptiveSoftmax.from_state_dict(sd, cut, embed.vocab, device, prefix)
        elif _get(args, "adaptive_softmax_cutoff") is not None:
            raise ValueError("adaptive_softmax_cutoff is set but the checkpoint has no adaptive_softmax.head.class_proj.weight")
        else:
            head = DenseSoftmax.from_state_dict(sd, args, device, prefix)
        scale = 1.0 if _get(args, "no_scale_embedding", False) else math.sqrt(d)
        return cls(embed, layers, H, act=act, scale=scale, pos=pos, learned_pos=learned, ln_emb=ln_emb, ln_out=ln_out, head=head,
                   device=device, precision=precision)

    @classmethod
    def from_checkpoint(cls, path, device, overrides=None, precision=None):
        """Load a reference ``.pt`` ({'args': Namespace, 'model': state_dict}) -> (model, args)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        args = ckpt["args"] if isinstance(ckpt["args"], Namespace) else Namespace(**ckpt["args"])
        for k_, v in (overrides or {}).items():
            setattr(args, k_, v)
        return cls.from_state_dict(ckpt["model"], args, device, precision=precision), args
