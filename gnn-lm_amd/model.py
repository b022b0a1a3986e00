"""``GnnLmModel`` -- the eval-path behaviour of ``TransformerLanguageModel`` with a
``TokenGraphTransformerDecoder`` (fairseq/models/transformer.py:910-1085) under
``--use-precompute-feat``: the base LM is bypassed (:974-976), the graph decoder (HGT) refines the
precomputed features, and the output layer scores the targets: the tied adaptive softmax, or -- for a checkpoint without one
(``--arch transformer_lm``: enwik8) -- the plain softmax over ``embed_tokens.weight | embed_out [+ xl_bias]`` (``DenseSoftmax``).

State-dict names follow the reference (prefix ``decoder.``): ``hgt_decoder.gcs.*``,
``tgt_quantizer.*`` (convert_ckpt.py:40-45), ``embed_tokens.embeddings.{i}.{0,1}.weight``,
``adaptive_softmax.head.class_proj.weight``; dense head: ``embed_tokens.weight`` / ``embed_out``,
``xl_bias``.
"""
import os
from argparse import Namespace
from typing import Union

import torch

from ._lib import raw_stream as _lib_raw_stream
from .adaptive_softmax import AdaptiveSoftmax
from .dense_softmax import DenseSoftmax
from .hgt import HGT, CodeStore, NeighborGraph, TokenStore, store_table
from .pq_wrapper import TorchPQCodec


class GnnLmModel(torch.nn.Module):
    graph_capture = False              # (class defaults: subclasses that script forward() need not call __init__)
    _graphs, _static_x = None, frozenset()
    orig_prob_ratio, keep_branches, short_cut = 0.0, False, False

    def __init__(self, hgt: HGT, asm: Union[AdaptiveSoftmax, DenseSoftmax], quantizer: TorchPQCodec = None, orig_prob_ratio: float = 0.0,
                 short_cut: bool = False, precision=None, token_embed=None):
        super().__init__()
        # `--reinit-nfeat` (language_modeling.py:151-153): the neighbour features are rows of this token_embed.TokenEmbedding
        # instead of decoded PQ codes; no quantizer is involved
        self.token_embed = token_embed
        # orig_prob_ratio = alpha > 0 (transformer.py:987-1005,1056-1062,1075-1077): every token is scored with
        #   logsumexp(log(alpha) + log p_asm(target | h), log(1 - alpha) + log p_asm(target | x))
        # h the base LM's feature, x the GNN output, both through the same head (`asm`: the tied adaptive softmax, or the dense
        # softmax, where the reference mixes the two softmaxes in probability space, :990-991,1002 -- the same target column).  Under --use-precompute-feat h is
        # graph.tgt_h, which the step already holds: no base LM is involved.  alpha <= 0 is off (the reference tests `> 0`);
        # alpha >= 1 is where the reference's math.log(1 - p1_coeff) raises ValueError("math domain error")
        if orig_prob_ratio >= 1:
            raise ValueError(f"math domain error: orig_prob_ratio = {orig_prob_ratio} needs log(1 - orig_prob_ratio) "
                             "(transformer.py:1060); use a ratio below 1 (eval_lm --sweep-orig-prob-ratio scores the base LM alone as its point 1)")
        self.orig_prob_ratio = float(orig_prob_ratio) if orig_prob_ratio > 0 else 0.0
        # a driver that sweeps the ratio wants the two unmixed branches of every batch whatever the model's own ratio is
        self.keep_branches = False
        self.hgt_decoder, self.adaptive_softmax, self.tgt_quantizer = hgt, asm, quantizer
        self.short_cut = short_cut
        # `eval_lm --graph-capture`: the launches of forward() and of target_log_probs() replayed from HIP graphs, one pair per
        # batch shape (the recipe's literal one-block batches are launch-bound: ~45 launches for 0.2 ms of GPU work)
        self.graph_capture = False
        if precision is not None:          # a name of ops.PRECISIONS ("fp16": what `eval_lm --fp16` sets); None: as hgt / asm carry
            self.precision = precision

    @property
    def precision(self) -> str:
        """Arithmetic of the GEMMs of the graph decoder and of the adaptive softmax (see ``GnnLmEngine.precision``)."""
        from . import ops
        mods = [m for m in (self.hgt_decoder, self.adaptive_softmax) if m is not None]
        return ops.precision_name(*(m.gemm_precision for m in mods))

    @precision.setter
    def precision(self, value):
        from . import ops
        v = ops.precision_value(value)
        for m in (self.hgt_decoder, self.adaptive_softmax):
            if m is not None:
                m.gemm_precision = v

    def eval(self):
        return self

    def forward(self, src_tokens, src_lengths=None, graph: NeighborGraph = None, **unused):
        """-> (x [bsz, tgt_len, d], extra) like TokenGraphTransformerDecoder.forward (:943-1009)."""
        if self.graph_capture and graph is not None and graph.block_off is not None:
            raise ValueError("--graph-capture replays one graph per batch SHAPE: a ragged batch (blocks of unequal length) has its own")
        if self.graph_capture and graph is not None and graph.tgt_h is not None and graph.fetcher is None \
                and graph.fetched_codes is None and not torch.cuda.is_current_stream_capturing():
            return self._forward_replayed(src_tokens, graph)
        return self._forward(src_tokens, graph)

    def _forward_replayed(self, src_tokens, graph):
        """The same call through a HIP graph captured once per batch shape: the batch's neighbour ids and features are copied into
        the graph's static input buffers (two small copies), one replay enqueues every launch of the step.  The outputs are the
        graph's static buffers -- valid until the next call of this shape (the scorer consumes them at once)."""
        import dataclasses
        key = ("fwd", tuple(src_tokens.shape), tuple(graph.ids.shape), graph.tgt_h.dtype, graph.left, graph.right, graph.max_intra_context,
               self.precision,                                                      # (a captured launch has its arithmetic baked in)
               id(graph.store), store_table(graph.store).data_ptr(), _lib_raw_stream())      # (one set of static buffers per stream)
        if self._graphs is None:
            self._graphs, self._static_x = {}, set()
        e = self._graphs.get(key)
        if e is None:
            ids, feats = graph.ids.clone(), graph.tgt_h.clone()
            static = dataclasses.replace(graph, ids=ids, tgt_h=feats)
            self._forward(src_tokens, static)                     # eager once: one-time allocations happen outside the capture
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            # captured ON THE LANE'S OWN STREAM: the workspaces of the HGT and of the softmax are keyed by the stream the kernels are
            # enqueued on (hgt.py, adaptive_softmax.py) -- torch's default capture stream is one stream for every capture, i.e. every
            # lane's graph would get the SAME scratch addresses and the graphs, replayed concurrently on different lanes, would race
            cap = self._capture_stream()
            with torch.cuda.graph(g, stream=cap):
                out = self._forward(src_tokens, static)
            e = self._graphs[key] = {"graph": g, "ids": ids, "feats": feats, "out": out, "static": static, "capture_stream": cap}
            self._static_x.add(out[0].data_ptr())
        e["ids"].copy_(graph.ids)
        e["feats"].copy_(graph.tgt_h)
        e["graph"].replay()
        return e["out"]

    def release_stream_state(self, keep=()):
        """Drop what is held per stream for every stream but `keep` (raw handles): the HIP graphs captured for those lanes FIRST (their
        launches have the lanes' workspace addresses baked in), then the workspaces and merge tables themselves
        (HGT.release_stream_state).  Called by a driver whose side lanes are gone (eval_lm.main); the caller has joined the lanes."""
        keep = set(keep)
        if self._graphs:
            torch.cuda.synchronize()
            gone = [k_ for k_ in self._graphs if k_[0] == "fwd" and k_[-1] not in keep]
            xs = {self._graphs[k_]["out"][0].data_ptr() for k_ in gone}
            gone += [k_ for k_ in self._graphs if k_[0] == "asm" and k_[1] in xs]
            for k_ in gone:
                del self._graphs[k_]
            self._static_x = set(self._static_x) - xs
        for mod in (self.hgt_decoder, self.adaptive_softmax):
            if hasattr(mod, "release_stream_state"):
                mod.release_stream_state(keep=keep)

    @staticmethod
    def _capture_stream():
        """The stream a lane's graphs are captured on: the lane's own stream -- or, for the lane that runs on the default stream
        (which cannot capture), a private stream of that lane: either way no two lanes' captures see the same stream handle."""
        cur = torch.cuda.current_stream()
        return torch.cuda.Stream(device=cur.device) if cur == torch.cuda.default_stream(cur.device) else cur

    def _forward(self, src_tokens, graph):
        bsz, tgt_len = src_tokens.shape
        if graph is None or graph.tgt_h is None:
            raise ValueError("graph.tgt_h (precomputed tgt features) is required: the base LM is not built "
                             "(--use-precompute-feat path, transformer.py:974-976)")
        if graph.block_off is not None:                    # a ragged batch: one run of packed tokens, cut into blocks by graph.block_off
            assert bsz == 1 and tgt_len == graph.ids.shape[0]
        else:
            assert graph.n_blocks == bsz and graph.T == tgt_len
        h = graph.tgt_h
        if h.dtype != torch.float32:
            from . import ops
            h = ops.half_to_float(h.contiguous()) if h.dtype == torch.float16 else h.float()
        extra = {"inner_states": [h.view(bsz, tgt_len, -1).transpose(0, 1)]}
        x = h if self.short_cut else self.hgt_decoder(graph, features={"tgt": h})["tgt"]
        x = x.view(bsz, tgt_len, -1)
        extra["gcn_feat"] = x.transpose(0, 1)                               # :997
        if self.orig_prob_ratio > 0 or self.keep_branches:
            extra["orig_x"] = h.view(bsz, tgt_len, -1)                      # :1004 (with an adaptive softmax output_layer is the identity)
            extra["orig_ratio"] = self.orig_prob_ratio                      # :1005
        return x, extra

    # ---- generation: the graph decoder one token at a time (generate_gnn.GnnGenerator)
    def _rows_graph(self, ids, store, left, right, n_blocks, T, block_off=None):
        if self.orig_prob_ratio > 0:
            raise NotImplementedError("orig_prob_ratio > 0 is not built for generation: the base-LM / GNN mixture is scored by eval_lm only")
        if store is None:
            raise ValueError("prefill_rows / step_rows need the model's store (make_store)")
        return NeighborGraph(ids=ids, n_blocks=n_blocks, T=T, left=left, right=right, store=store, block_off=block_off)

    def new_cache(self, B, cap, done=None, device=None):
        """The graph decoder's K' / V' cache (``HGT.new_cache``); ``done`` is shared with the base LM's cache."""
        return self.hgt_decoder.new_cache(B, cap, done=done, device=device)

    def prefill_rows(self, x, ids, cache, store, left, right, block_off):
        """Base-LM rows ``x`` [n_tok, d] of the packed prompts (``block_off``; block b is sequence b of ``cache``) and their neighbour
        ids [n_tok, kg] -> the GNN rows [n_tok, d] (``HGT.prefill``: the cache is filled).  ``short_cut``: the rows pass through."""
        G = self._rows_graph(ids, store, left, right, cache.B, 0, block_off)
        if self.short_cut:
            return x
        return self.hgt_decoder.prefill(G, {"tgt": x}, cache)["tgt"]

    def step_rows(self, x, ids, cache, store, left, right, max_len=None):
        """One new base-LM row per sequence ``x`` [B, d] and its neighbour ids [B, kg] -> the GNN rows [B, d] (``HGT.step``)."""
        G = self._rows_graph(ids, store, left, right, cache.B, 1)
        if self.short_cut:
            return x
        return self.hgt_decoder.step(G, {"tgt": x}, cache, max_len=max_len)["tgt"]

    def target_log_probs(self, net_output, target):
        """log p(target) [bsz, tgt_len]: get_normalized_probs(log_probs=True) + gather
        (transformer.py:1064-1079, sequence_scorer.py:48-53,89) without the dense [T, V] tensor."""
        x = net_output[0]
        bsz, T, d = x.shape
        extra = net_output[1] if len(net_output) > 1 and isinstance(net_output[1], dict) else {}
        if "orig_x" in extra:
            return self._target_log_probs_mixed(x, extra, target)
        if self.graph_capture and x.data_ptr() in self._static_x and not torch.cuda.is_current_stream_capturing():
            key = ("asm", x.data_ptr(), bsz, T, d)                # x is a replayed forward's static output: its address names the shape's graph
            e = self._graphs.get(key)
            if e is None:
                tgt = target.reshape(-1).clone()
                self.adaptive_softmax.target_log_prob(x.reshape(-1, d).contiguous(), tgt)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                cap = self._capture_stream()
                with torch.cuda.graph(g, stream=cap):                          # (the lane's own stream: see _forward_replayed)
                    out = self.adaptive_softmax.target_log_prob(x.reshape(-1, d).contiguous(), tgt).view(bsz, T)
                e = self._graphs[key] = {"graph": g, "target": tgt, "out": out, "x": x, "capture_stream": cap}
            e["target"].copy_(target.reshape(-1))
            e["graph"].replay()
            return e["out"]
        return self.adaptive_softmax.target_log_prob(x.reshape(-1, d).contiguous(), target.reshape(-1)).view(bsz, T)

    def _branches(self, x2, h2, tgt):
        """-> (gnn, base, mixed), each [n]: the softmax of the GNN output, of the base LM's feature, and their mixture at the model's
        own ratio (the GNN branch itself when that is 0).  The GNN branch is the same call as without a ratio.  With short_cut the
        GNN output IS the feature (both branches on h): one call serves both."""
        from . import ops
        asm = self.adaptive_softmax
        if self.short_cut:
            gnn = base = asm.target_log_prob(x2, tgt)
        else:                   # two n-row calls (one call over the stacked [2n, d] rows was measured and is no faster: DESIGN.md 7.9)
            gnn, base = asm.target_log_prob(x2, tgt), asm.target_log_prob(h2, tgt)
        mixed = ops.logp_mix(gnn, base, [self.orig_prob_ratio])[0] if self.orig_prob_ratio > 0 else gnn
        return gnn, base, mixed

    def _target_log_probs_mixed(self, x, extra, target):
        """target_log_probs with the base branch (get_normalized_probs, transformer.py:1075-1077): the mixture [bsz, tgt_len]; the
        two unmixed rows are left in ``extra["branch_logp"] = (gnn, base)`` for a sweep over the ratio."""
        bsz, T, d = x.shape
        h = extra["orig_x"]
        x2, h2 = x.reshape(-1, d).contiguous(), h.reshape(-1, h.shape[-1]).contiguous()
        if self.graph_capture and x.data_ptr() in self._static_x and not torch.cuda.is_current_stream_capturing():
            # both branches and the mix inside the shape's "asm" graph (x and orig_x are the replayed forward's static outputs)
            key = ("asm", x.data_ptr(), bsz, T, d)
            e = self._graphs.get(key)
            if e is None:
                tgt = target.reshape(-1).clone()
                self._branches(x2, h2, tgt)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                cap = self._capture_stream()
                with torch.cuda.graph(g, stream=cap):                          # (the lane's own stream: see _forward_replayed)
                    out = tuple(t.view(bsz, T) for t in self._branches(x2, h2, tgt))
                e = self._graphs[key] = {"graph": g, "target": tgt, "out": out, "x": x, "h": h2, "capture_stream": cap}
            e["target"].copy_(target.reshape(-1))
            e["graph"].replay()
            gnn, base, mixed = e["out"]
        else:
            gnn, base, mixed = (t.view(bsz, T) for t in self._branches(x2, h2, target.reshape(-1)))
        extra["branch_logp"] = (gnn, base)
        return mixed

    def dense_log_probs_rows(self, x2, h2=None):
        """Dense log-probs [rows, V] of flattened rows: the head over the GNN output ``x2`` [rows, d], mixed with the head over the
        base LM's features ``h2`` at the model's ``orig_prob_ratio`` when that is > 0 and ``h2`` is given (transformer.py:1075-1077)."""
        from .predict import lm_dense_rows
        if h2 is None or self.orig_prob_ratio <= 0 or self.short_cut:     # short_cut: both branches are the same rows (mixing x with x)
            return self.adaptive_softmax.log_probs(x2)
        return lm_dense_rows(self.adaptive_softmax, x2, h2, self.orig_prob_ratio)

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        """The dense [B, T, V] (log-)probabilities (transformer.py:1064-1085), on the device: 4 V bytes per token -- the eval path
        never asks for it (``target_log_probs``), and ``predict.predict_rows`` consumes it in row chunks instead."""
        x = net_output[0]
        bsz, T, d = x.shape
        extra = net_output[1] if len(net_output) > 1 and isinstance(net_output[1], dict) else {}
        h = extra.get("orig_x") if self.orig_prob_ratio > 0 else None         # :1075-1077 (a ratio of 0 is the GNN branch itself)
        lp = self.dense_log_probs_rows(x.reshape(-1, d).contiguous(), None if h is None else h.reshape(-1, h.shape[-1]).contiguous())
        lp = lp.view(bsz, T, -1)
        return lp if log_probs else lp.exp_()

    @classmethod
    def from_checkpoint(cls, path, device, overrides=None, vocab_size=None, quantizer=None, reinit_nfeat=False, precision=None):
        """Load a reference ``.pt`` ({'args': Namespace, 'model': state_dict}, checkpoint_utils.py:161-176).
        ``reinit_nfeat`` (the task flag ``--reinit-nfeat``): no quantizer is needed; the token-embedding table is built instead.
        ``precision`` (a name of ``ops.PRECISIONS``, e.g. "fp16" for ``--fp16``) is set on the model AND is what the table's GEMMs run
        under: the table is built once, so a model whose precision is changed afterwards refuses to make a store (``make_store``)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        args = ckpt["args"] if isinstance(ckpt["args"], Namespace) else Namespace(**ckpt["args"])
        for k_, v in (overrides or {}).items():
            setattr(args, k_, v)
        sd = ckpt["model"]
        d, H, L = args.decoder_embed_dim, args.decoder_attention_heads, args.graph_layer
        hgt = HGT(in_dim=d, hidden_dim=getattr(args, "decoder_gcn_dim", d), out_dim=d, n_layers=L, n_heads=H)
        hgt.load_state_dict({k_[len("decoder.hgt_decoder."):]: v for k_, v in sd.items()
                             if k_.startswith("decoder.hgt_decoder.")})
        token_embed = None
        if reinit_nfeat:
            from . import ops
            from .token_embed import TokenEmbedding
            token_embed = TokenEmbedding.from_state_dict(sd, args, device, ops.precision_value(precision or "f32"))
            if token_embed.d != hgt.in_dim:
                raise ValueError(f"--reinit-nfeat: the embedding table has {token_embed.d} columns, the graph decoder reads {hgt.in_dim}")
            if vocab_size is not None and int(vocab_size) != token_embed.vocab:
                raise ValueError(f"vocabulary mismatch: the dictionary has {int(vocab_size)} entries, embed_tokens has {token_embed.vocab} rows")
        elif quantizer is None:
            if "decoder.tgt_quantizer.centroids_torch" in sd:
                quantizer = TorchPQCodec.from_arrays(sd["decoder.tgt_quantizer.centroids_torch"].numpy(),
                                                     sd["decoder.tgt_quantizer.A"].numpy() if "decoder.tgt_quantizer.A" in sd else None,
                                                     sd["decoder.tgt_quantizer.b"].numpy() if "decoder.tgt_quantizer.b" in sd else None)
            elif getattr(args, "quantizer_path", "") and os.path.exists(str(args.quantizer_path)):
                quantizer = TorchPQCodec.from_file(args.quantizer_path)      # .npz or the recipe's faiss `quantizer` file
            else:
                raise ValueError("no quantizer: the checkpoint has no decoder.tgt_quantizer.* buffers "
                                 "(fairseq_cli/convert_ckpt.py) and quantizer_path does not name a file; a checkpoint trained with "
                                 "--reinit-nfeat has none and is scored with --reinit-nfeat (reinit_nfeat=True)")
        if getattr(args, "adaptive_softmax_cutoff", None) is None or "decoder.adaptive_softmax.head.class_proj.weight" not in sd:
            # no adaptive softmax (transformer.py:845): the plain output layer of a `--arch transformer_lm` checkpoint
            asm = DenseSoftmax.from_state_dict(sd, args, device)
            if vocab_size is not None and int(vocab_size) != asm.vocab:
                raise ValueError(f"vocabulary mismatch: the dictionary has {int(vocab_size)} entries, the checkpoint's output layer "
                                 f"has {asm.vocab} rows")
            return cls(hgt, asm, quantizer, getattr(args, "orig_prob_ratio", 0.0), getattr(args, "short_cut", False), precision=precision,
                       token_embed=token_embed), args
        cut = [int(c) for c in str(args.adaptive_softmax_cutoff).split(",")]
        if vocab_size is None:
            n_bands = sd["decoder.adaptive_softmax.head.class_proj.weight"].shape[0] + 1
            vocab_size = cut[0] + sum(sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"].shape[0] for i in range(1, n_bands))
        asm = AdaptiveSoftmax.from_state_dict(sd, cut, vocab_size, device)
        return cls(hgt, asm, quantizer, getattr(args, "orig_prob_ratio", 0.0), getattr(args, "short_cut", False), precision=precision,
                   token_embed=token_embed), args

    def make_store(self, codes, n_store, device, vals=None, row0=0) -> "CodeStore | TokenStore":
        if getattr(self, "token_embed", None) is not None:            # --reinit-nfeat: labels + embedding table, no codes
            if vals is None or row0 != 0:
                raise ValueError("--reinit-nfeat: the store is the whole label table (vals) of the train split; there is nothing to shard")
            from . import ops
            built = self.token_embed.precision
            if built is not None and ops.precision_name(built) != self.precision:
                raise ValueError(f"--reinit-nfeat: the token-embedding table was built under precision {ops.precision_name(built)!r}, the model "
                                 f"now runs {self.precision!r}; pass precision= to from_checkpoint so that one arithmetic serves both")
            return TokenStore(embed=self.token_embed.table, vals=vals.to(device).contiguous(), n_store=n_store)
        q = self.tgt_quantizer
        t = lambda a: a.to(device).contiguous()
        return CodeStore(codes=codes, centroids=t(q.centroids_torch), n_store=n_store, row0=row0, vals=vals,
                         A=t(q.A) if q.pre_torch else None, b=t(q.b) if q.pre_torch and q.b.numel() else None)
