"""What the base LM's drivers share on the host: ``generate`` and ``beam_search`` (flags, refusals, prompts, output), and with them
``eval_base_lm`` (the checkpoint and the ``KNNModel``)."""
import logging
import os
import sys

import numpy as np
import torch

PAD, EOS, UNK = 1, 2, 3         # fairseq Dictionary
KNN_SIM_FUNCS = ("do_not_recomp_ip", "do_not_recomp_l2", "ip", "l2")


# ------------------------------------------------------------------------------------------------ flags and refusals
def add_common_args(p, beam, max_len_help, out_help):
    """The flags ``generate`` and ``beam_search`` both take (one of them only to refuse it by name); ``beam`` is --beam's default."""
    p.add_argument("data", help="the data directory (DATA/<split>.bin/.idx, optionally dict.txt)")
    p.add_argument("--path", required=True, help="the --arch transformer_lm* checkpoint")
    p.add_argument("--model-overrides", default="{}")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--gen-subset", default="test")
    p.add_argument("--n-prompts", type=int, default=8)
    p.add_argument("--prompt-len", type=int, default=32)
    p.add_argument("--prompt-ids", default=None, help="one prompt as comma-separated token ids (instead of cutting prompts from the split)")
    p.add_argument("--max-len-b", type=int, default=64, help=max_len_help)
    p.add_argument("--beam", type=int, default=beam, help="beam_search: 1 .. 32; generate decodes at 1 and refuses anything else")
    p.add_argument("--min-len", type=int, default=1, help="beam_search: eos is forbidden while the hypothesis (the scored prompt included) "
                                                          "is shorter; generate refuses anything but 1")
    p.add_argument("--sampling", action="store_true", help="generate: sample, from the top --sampling-topk or from the nucleus of "
                                                           "--sampling-topp (one of the two); beam_search refuses it")
    p.add_argument("--sampling-topk", type=int, default=-1, help="generate: sample from the K most likely tokens, K <= 2048")
    p.add_argument("--sampling-topp", type=float, default=-1.0,
                   help="generate: sample from the smallest set of tokens whose probabilities sum to P or more (fairseq/search.py:174-217; the "
                        "sum is not renormalised); P >= 1 samples from (essentially) the whole vocabulary, P <= 0 is off; beam_search refuses it")
    p.add_argument("--temperature", type=float, default=1.0,
                   help="the GENERATION temperature (fairseq/options.py:548): the decoder output is divided by it.  The kNN temperature, "
                        "which eval_lm calls --temperature (options.py:496), is --knn-temperature here")
    p.add_argument("--knn-temperature", type=float, default=1.0, help="the temperature of the kNN distribution (eval_lm's --temperature)")
    p.add_argument("--unkpen", type=float, default=0.0)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--no-repeat-ngram-size", type=int, default=0, help="not built: refused")
    p.add_argument("--graph", action="store_true", help="not built (HGTLayer.infer): refused")
    for name in ("--sweep-lmbda", "--sweep-temperature", "--sweep-k"):
        p.add_argument(name, default=None, help="belongs to eval_lm: refused")
    p.add_argument("--knnlm", action="store_true")
    p.add_argument("--k", type=int, default=1024)
    p.add_argument("--lmbda", type=float, default=0.25, help="weight of the kNN distribution with --knnlm; 0 is refused (it would load the "
                   "datastore and generate from the base LM alone: drop --knnlm for that)")
    p.add_argument("--probe", type=int, default=32)
    p.add_argument("--dstore-dir", default=None)
    p.add_argument("--index-file", default=None)
    p.add_argument("--knn-sim-func", default="do_not_recomp_ip")
    p.add_argument("--knn-keytype", default=None)
    p.add_argument("--out", default=None, help=out_help)
    return p


def check_unbuilt(args):
    """The flags neither driver computes, and more than one process."""
    if args.no_repeat_ngram_size:
        raise ValueError("--no-repeat-ngram-size is not built")
    if args.graph:
        raise ValueError("--graph: generation through the GNN (HGTLayer.infer) is not built")
    for name in ("sweep_lmbda", "sweep_temperature", "sweep_k"):
        if getattr(args, name) is not None:
            raise ValueError(f"--{name.replace('_', '-')} belongs to eval_lm: generation runs one setting")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise NotImplementedError("generation runs in one process (WORLD_SIZE > 1 is not built)")


def check_knn_store(args):
    if args.knnlm and getattr(args, "knn_model", None) is None and not (args.dstore_dir and args.index_file):
        raise ValueError("--knnlm needs --dstore-dir and --index-file")


def check_knn_sim_func(args):
    if args.knnlm and args.knn_sim_func not in KNN_SIM_FUNCS:
        raise ValueError("Invalid knn similarity function!")


def check_knn_and_prompts(args):
    """The tail of both drivers' ``check_args``: the kNN mixture's flags, then the prompts'."""
    check_knn_store(args)
    if args.knnlm and not 0.0 < args.lmbda < 1.0:
        raise ValueError(f"--lmbda {args.lmbda} with --knnlm: the mixture needs 0 < lmbda < 1 (without kNN: drop --knnlm)")
    check_knn_sim_func(args)
    if args.prompt_ids is None and (args.n_prompts < 1 or args.prompt_len < 1):
        raise ValueError("--n-prompts and --prompt-len must be at least 1")


def check_decode(max_new, temperature):
    if max_new < 1:
        raise ValueError("max_new (--max-len-b) must be at least 1")
    if not temperature > 0:
        raise ValueError("--temperature must be greater than 0")


# ------------------------------------------------------------------------------------------------ the model and the store
def load_model(args, device, model=None):
    """The checkpoint of --path (with --model-overrides, --fp16), or the caller's ``model`` put to --fp16."""
    if model is None:
        import ast
        from .transformer_lm import TransformerLM
        model, _ = TransformerLM.from_checkpoint(args.path, device, ast.literal_eval(args.model_overrides), precision="fp16" if args.fp16 else None)
    elif args.fp16:
        model.precision = "fp16"
    return model


def load_knn(args, model, device, queries="have"):
    """--knnlm: ``args.knn_model`` (tests, tools) or the ``KNNModel`` of --index-file / --dstore-dir, refused when its keys are not as
    wide as the model's rows; None without --knnlm.  ``queries``: the caller's words for its rows in that refusal."""
    if not args.knnlm:
        return None
    from .knn_model import KNNModel
    knn = getattr(args, "knn_model", None) or KNNModel(
        index_file=args.index_file, dstore_dir=args.dstore_dir, probe=args.probe, cuda=-1, k=args.k,
        no_load_keys=("do_not_recomp" in args.knn_sim_func), use_memory=True, metric_type=args.knn_sim_func, device=device)
    width = getattr(knn, "hidden_size", None)
    if width is not None and int(width) != model.d:
        raise ValueError(f"--knnlm: the queries {queries} width {model.d}, the datastore {args.dstore_dir} holds keys of hidden_size {int(width)}")
    return knn


# ------------------------------------------------------------------------------------------------ prompts
def pack_prompts(prompts, device):
    """A list of non-empty lists of token ids -> ``(tokens int64 [n_tok] on the device, offsets int32 [B + 1] on the host, lengths
    int64 numpy [B], last int64 [B] on the host: the packed row of every prompt's last token)``."""
    if not prompts or any(len(p) < 1 for p in prompts):
        raise ValueError("generate: every prompt needs at least one token")
    lens = np.asarray([len(p) for p in prompts], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    tokens = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=device)
    return tokens, torch.from_numpy(off.astype(np.int32)), lens, torch.from_numpy(off[1:] - 1)


def last_rows(x, extra, last):
    """The rows ``last`` of a prefill's ``(x, extra)``: what the first pick is made from."""
    last = last.to(x.device)
    return x[last], {k_: ([v[0][last]] if isinstance(v, list) else v[last]) for k_, v in extra.items()}


def padded_prompts(prompts):
    """--out: ``prompts`` int64 [B, longest] padded with ``pad``, and ``prompt_lengths``."""
    pr = np.full((len(prompts), max(len(p) for p in prompts)), PAD, dtype=np.int64)
    for i, p in enumerate(prompts):
        pr[i, :len(p)] = p
    return pr, np.asarray([len(p) for p in prompts])


def word_of(data):
    """token id -> its word in DATA/dict.txt, or the id itself where there is none."""
    from .eval_lm import load_symbols
    symbols = load_symbols(data)
    return lambda t: symbols[t] if symbols is not None and 0 <= t < len(symbols) else str(t)


def cli_main(main, get_parser, argv=None):
    logging.basicConfig(format="%(asctime)s | %(levelname)s | %(name)s | %(message)s", level=os.environ.get("LOGLEVEL", "INFO").upper(),
                        stream=sys.stderr)
    main(get_parser().parse_args(argv))
