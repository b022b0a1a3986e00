"""Generate from the GNN-LM: the base LM's K/V-cache step, a kNN search of its row, and the incremental HGT step over a K'/V' cache.

    python -m gnnlm_amd.generate_gnn DATA --path GNN.pt [--base-path BASE.pt] --dstore-dir D --index-file F --gcn-k 128 \\
        --neighbor-context 2 [--probe 32] [--model-overrides ...] --n-prompts 8 --prompt-len 32 --max-len-b 64 \\
        [--sampling --sampling-topk 10 | --sampling --sampling-topp 0.9] [--temperature 0.8] [--unkpen X] [--seed 1] [--fp16] [--out F.npz]

What the reference only sketches: ``HGTLayer.infer`` (fairseq/models/hgt.py:81-297) is unreachable there (``extract_graph_features``
asserts ``incremental_state is None``, transformer.py:1028).  The step is exact: ntgt nodes never receive
from tgt nodes, a token's star edges read its own neighbours only and the causal edges run u -> w for u <= w inside the block, so the
row of a new token depends on its own input row, its own neighbours and the cached K' / V' rows of the tokens before it.

The loop is ``generate.Generator.generate``'s -- same rules, same pick kernels, same returns -- with the model behind it swapped:

  prefill   ``TransformerLM.prefill`` over the packed prompts; ONE ``search_sims(x, k=gcn_k)`` over all prompt rows; ``GnnLmModel
            .prefill_rows`` (``gnnlm_hgt_prefill``) fills the graph decoder's cache; the last row of every prompt goes on.
  head      the GNN-LM's own output layer over the GNN rows divided by the temperature; ``pad = -inf``; the unk penalty.
  pick      unchanged (``ops.topk_merge`` + ``ops.sample_topk``, or ``ops.sample_topp``).
  step      ``x = lm.step(next)``; ``ids = search_sims(x, gcn_k)[1]``; ``g = gnn.step_rows(x, ids)`` (``gnnlm_hgt_step``).

``x`` is both the tgt feature and the search query, as in the recipe: ``keys.npy`` of a split is both ``tgt_h`` and ``find_knn``'s query.

Refused by name, never approximated: ``--beam`` != 1, ``--knnlm``, ``--sweep-*``, ``--reinit-nfeat``, ``--store sharded | peer``, more
than one process, ``--min-len`` != 1, ``--no-repeat-ngram-size``, ``--intra-context``, ``--gcn-context-window``, ``orig_prob_ratio`` > 0.
"""
import argparse
import ast
import logging
import os
import sys
from argparse import Namespace

import numpy as np
import torch

from . import gen_common
from .generate import Generator, read_prompts
from .predict import MAX_TOPK, head_vocab

logger = logging.getLogger("gnnlm_amd.generate_gnn")


class IndexSearch:
    """``search_sims`` over a bare index (``ExactIndex``, ``IVFPQIndex``: anything with ``search_device``) for a caller that has no
    ``KNNModel`` around it: the index's own scores are the similarities (``do_not_recomp_ip``)."""

    def __init__(self, index):
        self.index = index

    def search_sims(self, queries, k=0, **unused):
        sims, ids = self.index.search_device(queries.float().contiguous(), k)[:2]
        return sims, ids


class GnnGenerator(Generator):
    def __init__(self, lm, gnn, knn, gcn_k, left, right, store=None):
        """lm: a ``TransformerLM`` (no head needed).  gnn: a ``GnnLmModel``; its store is ``store``, else ``gnn.store``
        (``GnnLmModel.make_store``).  knn: anything with ``search_sims(queries, k) -> (sims, ids)``.  ``gcn_k`` neighbours per token,
        ``left`` / ``right`` the neighbour context (``--neighbor-context``)."""
        self.lm, self.gnn, self.search = lm, gnn, knn
        self.store = store if store is not None else getattr(gnn, "store", None)
        if self.store is None:
            raise ValueError("GnnGenerator: the GnnLmModel's store is missing (pass store=gnn.make_store(...))")
        if gnn.orig_prob_ratio > 0:
            raise NotImplementedError("orig_prob_ratio > 0 is not built for generation")
        if gnn.hgt_decoder.in_dim != lm.d:
            raise ValueError(f"GnnGenerator: the base LM's rows are {lm.d} wide, the graph decoder reads {gnn.hgt_decoder.in_dim}")
        if gcn_k < 1:
            raise ValueError("--gcn-k must be at least 1")
        self.gcn_k, self.left, self.right = int(gcn_k), int(left), int(right)
        self.knn, self.knn_keytype, self.k, self.lmbda, self.knn_temperature = None, None, 0, 0.0, 1.0      # no kNN mix on top
        self.vocab = head_vocab(gnn.adaptive_softmax)
        self._cool = {}
        self.lm_cache = self.gnn_cache = self.last_run = None          # the two caches and the neighbour ids of the last run

    @property
    def head(self):
        return self.gnn.adaptive_softmax

    def _neighbours(self, x):
        return self.search.search_sims(x, k=self.gcn_k)[1].contiguous()

    def _start(self, prompts, max_new):
        from .ragged import as_ragged
        lm = self.lm
        tokens, off, lens, last = gen_common.pack_prompts(prompts, lm.device)
        rg = as_ragged(off, lm.device)                                   # one table for both prefills
        B, cap = len(prompts), int(lens.max()) + max_new - 1
        cache = self.lm_cache = lm.new_cache(B, cap)
        x, _ = lm.prefill(tokens, rg, cache, want_inner=False, want_ffn_input=False, check=False)
        ids = self._neighbours(x)
        self.gnn_cache = self.gnn.new_cache(B, cap, done=cache.done)
        g = self.gnn.prefill_rows(x, ids, self.gnn_cache, self.store, self.left, self.right, rg)
        self.last_run = {"prompt_ids": ids, "step_ids": []}              # (device tensors: nothing is read back here)
        return cache, g[last.to(g.device)], {}

    def _advance(self, nxt, cache):
        x, _ = self.lm.step(nxt, cache, want_inner=False, want_ffn_input=False)
        ids = self._neighbours(x)
        self.last_run["step_ids"].append(ids)
        return self.gnn.step_rows(x, ids, self.gnn_cache, self.store, self.left, self.right), {}

    def _out_of_range(self, cache):
        return int(cache.n_bad.item()) + int(self.gnn_cache.n_bad.item())


# ------------------------------------------------------------------------------------------------ the driver
def get_parser():
    p = argparse.ArgumentParser(prog="python -m gnnlm_amd.generate_gnn", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    gen_common.add_common_args(p, beam=1, max_len_help="tokens to generate per prompt",
                               out_help="write tokens / logp / lengths / prompts to this .npz")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--base-path", default=None, help="the base LM's checkpoint; default: the decoder.* weights of --path itself")
    p.add_argument("--gcn-k", type=int, default=128)
    p.add_argument("--neighbor-context", default="(2, 2)")
    p.add_argument("--reinit-nfeat", action="store_true", help="not built for generation: refused")
    p.add_argument("--store", default="auto", help="auto | replicated; sharded and peer are not built for generation: refused")
    p.add_argument("--intra-context", type=int, default=0, help="not built for generation: refused")
    p.add_argument("--gcn-context-window", type=int, default=0, help="not built for generation: refused")
    return p


def check_args(args):
    """Host only, before any device work: what this build does not compute is refused with the flag's name."""
    if args.beam != 1:
        raise ValueError(f"--beam {args.beam}: beam search through the GNN is not built (this driver decodes at --beam 1)")
    if args.min_len != 1:
        raise ValueError(f"--min-len {args.min_len} is not built (only --min-len 1)")
    if args.no_repeat_ngram_size:
        raise ValueError("--no-repeat-ngram-size is not built")
    if args.knnlm:
        raise ValueError("--knnlm: the kNN mix on top of the GNN-LM is not built for generation")
    for name in ("sweep_lmbda", "sweep_temperature", "sweep_k"):
        if getattr(args, name) is not None:
            raise ValueError(f"--{name.replace('_', '-')} belongs to eval_lm: generation runs one setting")
    if args.reinit_nfeat:
        raise ValueError("--reinit-nfeat is not built for generation (the step reads a code store)")
    if args.store in ("sharded", "peer"):
        raise ValueError(f"--store {args.store} is not built for generation (one process holds the whole code table)")
    if args.store not in ("auto", "replicated"):
        raise ValueError(f"--store {args.store}: auto or replicated")
    if args.intra_context:
        raise ValueError("--intra-context is not built for generation (the decode kernel has no window)")
    if args.gcn_context_window:
        raise ValueError("--gcn-context-window is not built for generation")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("generation runs in one process (WORLD_SIZE > 1 is not built)")
    Generator.check(args.max_len_b, args.sampling, args.sampling_topk, args.temperature, MAX_TOPK, args.sampling_topp)
    if getattr(args, "knn_model", None) is None and not (args.dstore_dir and args.index_file):
        raise ValueError("the graph's neighbours are searched per token: --dstore-dir and --index-file are required")
    if args.knn_sim_func not in gen_common.KNN_SIM_FUNCS:
        raise ValueError("Invalid knn similarity function!")
    if args.gcn_k < 1:
        raise ValueError("--gcn-k must be at least 1")
    nc = ast.literal_eval(str(args.neighbor_context))
    left, right = (nc, nc) if isinstance(nc, int) else nc
    if left < 0 or right < 0:
        raise ValueError(f"--neighbor-context {args.neighbor_context}: two non-negative context sizes")
    if args.prompt_ids is None and (args.n_prompts < 1 or args.prompt_len < 1):
        raise ValueError("--n-prompts and --prompt-len must be at least 1")
    return int(left), int(right)


def load_base_lm(path, device, overrides, precision):
    """The base LM of a checkpoint that may be a GNN-LM's: the graph decoder's and the quantizer's entries are left out of the
    state dict it is built from."""
    from .transformer_lm import TransformerLM
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    cargs = ckpt["args"] if isinstance(ckpt["args"], Namespace) else Namespace(**ckpt["args"])
    for k_, v in (overrides or {}).items():
        setattr(cargs, k_, v)
    sd = {k_: v for k_, v in ckpt["model"].items() if not k_.startswith(("decoder.hgt_decoder.", "decoder.tgt_quantizer."))}
    return TransformerLM.from_state_dict(sd, cargs, device, precision=precision)


def load_codes(dstore_dir, device):
    """``D/quantized-keys.npy``: uint8 [n_store, M], one code row per key of the datastore (language_modeling.py:274-276)."""
    path = os.path.join(dstore_dir, "quantized-keys.npy")
    if not os.path.exists(path):
        raise FileNotFoundError(f"the code table {path} was not found")
    codes = np.load(path, mmap_mode="r")
    if codes.ndim != 2 or codes.dtype != np.uint8:
        raise ValueError(f"{path}: {codes.dtype} {codes.shape}, expected uint8 [n_store, M] (one code row per key of the datastore)")
    return torch.from_numpy(np.array(codes)).to(device)


def main(args, lm=None, gnn=None, file=None):
    """-> dict(tokens, logp, lengths (numpy), prompts).  Prints fairseq's ``S-i`` / ``H-i`` lines to ``file`` (stdout)."""
    left, right = check_args(args)
    file = sys.stdout if file is None else file
    device = torch.device(args.device)
    torch.cuda.set_device(device)
    prompts = read_prompts(args)
    overrides = ast.literal_eval(args.model_overrides)
    precision = "fp16" if args.fp16 else None
    if gnn is None:
        from .model import GnnLmModel
        gnn, _ = GnnLmModel.from_checkpoint(args.path, device, overrides, precision=precision)
    elif args.fp16:
        gnn.precision = "fp16"
    if lm is None:
        lm = load_base_lm(args.base_path or args.path, device, overrides, precision)
    elif args.fp16:
        lm.precision = "fp16"
    knn = getattr(args, "knn_model", None)
    if knn is None:
        from .knn_model import KNNModel
        knn = KNNModel(index_file=args.index_file, dstore_dir=args.dstore_dir, probe=args.probe, cuda=-1, k=args.gcn_k,
                       no_load_keys=("do_not_recomp" in args.knn_sim_func), use_memory=True, metric_type=args.knn_sim_func, device=device)
    width = getattr(knn, "hidden_size", None)
    if width is not None and int(width) != lm.d:
        raise ValueError(f"the queries have width {lm.d}, the datastore {args.dstore_dir} holds keys of hidden_size {int(width)}")
    store = getattr(args, "code_store", None)
    if store is None:
        codes = load_codes(args.dstore_dir, device)
        n_keys = getattr(knn, "dstore_size", None)
        if n_keys is not None and int(n_keys) != codes.shape[0]:
            raise ValueError(f"quantized-keys.npy holds {codes.shape[0]} code rows, the datastore {int(n_keys)} keys")
        store = gnn.make_store(codes, codes.shape[0], device)
    how = "greedy" if not args.sampling else \
        (f"top-p {args.sampling_topp} (nucleus) sampling" if args.sampling_topp > 0 else f"top-{args.sampling_topk} sampling") + \
        f" at temperature {args.temperature}"
    logger.info("%d prompt(s), up to %d new tokens each, %s, %d neighbours per token, context (%d, %d), precision %s", len(prompts),
                args.max_len_b, how, args.gcn_k, left, right, gnn.precision)
    g = GnnGenerator(lm, gnn, knn, args.gcn_k, left, right, store=store)
    tokens, logp, lengths = g.generate(prompts, args.max_len_b, sampling=args.sampling, sampling_topk=args.sampling_topk,
                                       temperature=args.temperature, unk_penalty=args.unkpen, seed=args.seed, sampling_topp=args.sampling_topp)
    tokens, logp, lengths = tokens.cpu().numpy(), logp.cpu().numpy(), lengths.cpu().numpy()
    word = gen_common.word_of(args.data)
    for i, p in enumerate(prompts):
        n = int(lengths[i])
        print(f"S-{i}\t" + " ".join(word(t) for t in p[1:]), file=file)
        print(f"H-{i}\t{float(logp[i, :n].astype(np.float64).sum())}\t" + " ".join(word(int(t)) for t in tokens[i, :n]), file=file)
    res = {"tokens": tokens, "logp": logp, "lengths": lengths, "prompts": prompts}
    if args.out:
        pr, pr_len = gen_common.padded_prompts(prompts)
        np.savez(args.out, tokens=tokens, logp=logp, lengths=lengths, prompts=pr, prompt_lengths=pr_len)
    return res


def cli_main(argv=None):
    gen_common.cli_main(main, get_parser, argv)


if __name__ == "__main__":
    cli_main()
