#!/usr/bin/env python3
"""``run_index_build`` -- producer of the kNN index, mirror of ``knn/run_index_build.py`` + ``knn/index_builder.py`` for the
index family the recipes use (``--index-type OPQ64_1024,IVF4096,PQ64 --metric cosine``,
gnnlm_scripts/wiki103/find_knn.sh:8-13).  The reference hands training and adding to faiss; here both run on the GPU
(``IVFPQIndex.train``, ``IVFPQIndex.add``) and the result is written next to where the reference puts its file:
``<dstore-dir>/faiss_store.<metric><suffix>.gnnlm.npz`` (``KNNModel`` / ``find_knn`` pick it up from the reference's
``--index-file`` path).  An offline tool: a "next" row of SURVEY.md 8f, not the eval hot path."""
import argparse
import logging
import os
import re

import numpy as np
import torch

from .data_store import DataStore
from .ivfpq import IVFPQIndex

LOGGING = logging.getLogger("gnnlm_amd.run_index_build")


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--dstore-dir", type=str, required=True)
    p.add_argument("--index-type", type=str, default="OPQ64_1024,IVF4096,PQ64")
    p.add_argument("--metric", type=str, default="cosine", choices=["l2", "ip", "cosine"],
                   help="l2: squared distances (the reference's own default, knn/run_index_build.py:50); the recipes pass cosine")
    p.add_argument("--suffix", type=str, default="")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--max-train", type=int, default=1000000)
    p.add_argument("--chunk-size", type=int, default=1 << 18)
    p.add_argument("--nprobe", type=int, default=32)
    p.add_argument("--opq-iters", type=int, default=10, help="rounds of OPQ training when --index-type has an OPQ block (0: random rotation)")
    p.add_argument("--overwrite", action="store_true", help="retrain and rebuild even if the trained / final index files exist")
    p.add_argument("--save-every", type=int, default=0,
                   help="rewrite the index file every this many chunks, so that a killed build resumes from it (0: save at the end only; "
                        "the reference rewrites after every chunk, knn/index_builder.py:108).  Every save merges ALL rows filed so far into "
                        "new arrays and rebuilds the index's device layouts: copy traffic grows with (keys / (K * chunk))^2, so keep K * chunk "
                        "a sizeable share of the datastore")
    p.add_argument("--cuda", type=int, default=0)
    return p


def parse_index_type(s):
    """'OPQ64_1024,IVF4096,PQ64' -> (nlist, M); the OPQ block fixes the rotation's shape (``parse_opq_block``)."""
    ivf, pq = re.search(r"IVF(\d+)", s), re.search(r"(?:^|,)PQ(\d+)", s)
    if not (ivf and pq):
        raise ValueError(f"--index-type {s!r}: only OPQ*,IVF<nlist>,PQ<M> indexes are built")
    return int(ivf.group(1)), int(pq.group(1))


def parse_opq_block(s, hidden):
    """The output dimension of the index type's OPQ block, ``quantize_features.parse_index``'s rule: 'OPQ16_64,IVF1048576,PQ16' -> 64
    (the rotation reduces ``hidden`` to 64 dimensions, gnnlm_scripts/one_billion/find_knn.sh:8-21), 'OPQ64_1024,...' -> 1024, no OPQ
    block or one without '_<d_out>' -> None (a square rotation).  d_out must divide into the PQ block's M sub-spaces and not exceed
    ``hidden``."""
    opq = re.search(r"OPQ(\d+)(?:_(\d+))?", s)
    if opq is None or opq.group(2) is None:
        return None
    pq = re.search(r"(?:^|,)PQ(\d+)", s)
    M, d_out = int(pq.group(1)) if pq else int(opq.group(1)), int(opq.group(2))
    if d_out <= 0 or d_out % M or d_out > hidden:
        raise ValueError(f"--index-type {s!r}: d_out = {d_out} must divide into {M} sub-spaces and not exceed the keys' {hidden} dimensions")
    return d_out


def main(args):
    """The reference's protocol (knn/index_builder.py:66-109): train once and keep the trained index next to the final one
    (``faiss_store.trained.<metric><suffix>.gnnlm.npz``), then add the datastore's rows from where the final file stops (its
    ``ntotal``): a datastore that has grown costs its new rows only, and a build that was killed resumes."""
    if not torch.cuda.is_available():
        raise RuntimeError("gnnlm_amd.run_index_build needs a GPU (no CPU fallback)")
    out = os.path.join(args.dstore_dir, f"faiss_store.{args.metric}{args.suffix}.gnnlm.npz")
    trained = os.path.join(args.dstore_dir, f"faiss_store.trained.{args.metric}{args.suffix}.gnnlm.npz")
    ds = DataStore.from_pretrained(args.dstore_dir)
    device = torch.device("cuda", max(args.cuda, 0))
    if os.path.exists(out) and not args.overwrite:
        start = int(np.load(out)["list_off"][-1])                                # index.ntotal (index_builder.py:101)
        if start == ds.dstore_size:
            LOGGING.info("%s exists, use --overwrite to rebuild", out)
            return out
        if start > ds.dstore_size:
            raise ValueError(f"{out} holds {start} keys, the datastore only {ds.dstore_size}: --overwrite rebuilds the index")
        index = IVFPQIndex.load(out, device=device)
        LOGGING.info("%s holds %d of %d keys: adding the rest", out, start, ds.dstore_size)
    elif os.path.exists(trained) and not args.overwrite:
        index = IVFPQIndex.load(trained, device=device)
        LOGGING.info("trained index %s exists, use --overwrite to retrain", trained)
    else:
        nlist, M = parse_index_type(args.index_type)
        nlist = max(1, min(nlist, ds.dstore_size // 30 or 1))                   # index_builder.py:56: at least ~30 keys per list
        index = IVFPQIndex.train(ds.keys, nlist, M, device=device, cosine=(args.metric == "cosine"), nprobe=args.nprobe,
                                 train_size=args.max_train, seed=args.seed, chunk=args.chunk_size,
                                 opq_iters=args.opq_iters if "OPQ" in args.index_type else 0, metric="l2" if args.metric == "l2" else "ip",
                                 d_out=parse_opq_block(args.index_type, ds.keys.shape[1]))
        index.save(trained)
    # a file that is reused fixes the index's shape; the seed and the OPQ rounds that made it are not on record in it
    want_nlist, want_M = parse_index_type(args.index_type)
    LOGGING.info("index: %d lists, PQ%d, %d of %d keys", index.nlist, index.M, index.ntotal, ds.dstore_size)
    want_d = parse_opq_block(args.index_type, ds.keys.shape[1]) or ds.keys.shape[1]
    if index.M != want_M or index.nlist > want_nlist or index.R.shape[0] != want_d:
        LOGGING.warning("the index file on disk has %d lists, PQ%d and a rotation to %d dimensions, --index-type %s asks for %d lists, "
                        "PQ%d and %d dimensions: the file wins (--overwrite retrains; --seed / --opq-iters of a reused file are "
                        "whatever trained it)", index.nlist, index.M, index.R.shape[0], args.index_type, want_nlist, want_M, want_d)
    # every --save-every chunks the rows added so far are merged and the file rewritten (0: at the end only)
    span = args.save_every * args.chunk_size if args.save_every > 0 else max(ds.dstore_size, 1)
    while index.ntotal < ds.dstore_size:
        lo, hi = index.ntotal, min(ds.dstore_size, index.ntotal + span)
        index = index.add(ds.keys[lo:hi], chunk=args.chunk_size)                # ids lo .. hi - 1: np.arange(start, end), index_builder.py:107
        index.save(out + ".part.npz")                                          # a build killed while it writes leaves the last complete file
        os.replace(out + ".part.npz", out)
    print(f"Save index of {index.ntotal} keys ({index.nlist} lists, PQ{index.M}) to {out}")
    return out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(get_parser().parse_args())
