#!/usr/bin/env python3
"""``edit_index`` -- take keys out of a kNN IVF-PQ index file and / or merge index files, without retraining and without
re-encoding (``IVFPQIndex.remove`` / ``merge``: faiss's ``remove_ids`` / ``merge_from``; the reference's ``knn/index_builder.py``
only trains and adds, so it has no counterpart):

    python -m gnnlm_amd.edit_index --index-file IN --out OUT [--remove-ranges 100:200,5000:5100] [--remove-ids-file ids.npy]
                                   [--merge OTHER ...] [--cuda 0]

``IN`` and every ``OTHER`` are this package's ``.gnnlm.npz`` files or the reference's faiss files (``faiss_io.sniff``); ``OUT`` is
always a ``.gnnlm.npz`` file, written through ``OUT.part.npz`` and ``os.replace``.  Ids are datastore rows (token positions): a removal
changes neither the ids of the other keys nor ``vals.npy``; a document is one range ``lo:hi`` (half-open).  Removals apply to ``IN``
first, then the ``OTHER`` files are merged in the order given (all must share ``IN``'s trained part, e.g. built from one
``faiss_store.trained.*`` file range by range); ids present in two files are not checked, as in ``add``.

An edited file must NOT be put where ``run_index_build`` resumes from (``<dstore-dir>/faiss_store.<metric><suffix>.gnnlm.npz``
while the datastore still grows): that tool reads the file's ``ntotal`` as "rows 0 .. ntotal - 1 are present" and would add rows
from there, leaving out the rows behind a removed one and adding others twice.  An offline tool, not the eval hot path."""
import argparse
import logging
import os

import numpy as np
import torch

LOGGING = logging.getLogger("gnnlm_amd.edit_index")


def get_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--index-file", type=str, required=True, help="the index to edit: a .gnnlm.npz file or a faiss [OPQ,]IVF,PQ file")
    p.add_argument("--out", type=str, required=True, help="the edited index, a .gnnlm.npz file (never --index-file itself)")
    p.add_argument("--remove-ranges", type=str, default="", help="half-open id ranges lo:hi, comma-separated (a single id: id:id+1)")
    p.add_argument("--remove-ids-file", type=str, default="", help="a .npy file of ids to remove (any order, duplicates allowed)")
    p.add_argument("--merge", type=str, nargs="*", default=[], help="index files with the same trained part whose keys are merged in")
    p.add_argument("--metric", type=str, default="cosine", choices=["l2", "ip", "cosine"],
                   help="of a faiss file (its header does not say whether keys are normalised); a .gnnlm.npz file carries its own")
    p.add_argument("--cuda", type=int, default=0)
    return p


def parse_ranges(s):
    """'100:200,5000:5100' -> [(100, 200), (5000, 5100)]; anything else than integers lo:hi with lo < hi raises ``ValueError``"""
    out = []
    for item in filter(None, (x.strip() for x in s.split(","))):
        parts = item.split(":")
        try:
            lo, hi = (int(x) for x in parts)
        except ValueError:
            raise ValueError(f"--remove-ranges {item!r}: expected lo:hi with integer lo < hi") from None
        if lo >= hi:
            raise ValueError(f"--remove-ranges {item!r}: expected lo:hi with integer lo < hi")
        out.append((lo, hi))
    return out


def check_args(args):
    """The refusals that need no device: nothing to do, the output over the input, malformed ranges.  -> the parsed ranges"""
    ranges = parse_ranges(args.remove_ranges)
    if not (ranges or args.remove_ids_file or args.merge):
        raise ValueError("edit_index: nothing to do (--remove-ranges, --remove-ids-file or --merge)")
    same = lambda a, b: os.path.abspath(a) == os.path.abspath(b) or (os.path.exists(a) and os.path.exists(b) and os.path.samefile(a, b))
    if any(same(args.out, src) for src in [args.index_file] + list(args.merge)):
        raise ValueError("edit_index: --out must not be one of the input files")
    if not args.out.endswith(".gnnlm.npz"):
        raise ValueError("edit_index: --out is written in this package's format and ends in .gnnlm.npz")
    return ranges


def load_index(path, device, metric="cosine"):
    from . import faiss_io
    from .ivfpq import IVFPQIndex
    if faiss_io.sniff(path) in ("IxPT", "IwPQ"):
        return IVFPQIndex.from_faiss_file(path, device=device, cosine=(metric == "cosine"))
    return IVFPQIndex.load(path, device=device)


def main(args):
    ranges = check_args(args)
    if not torch.cuda.is_available():
        raise RuntimeError("gnnlm_amd.edit_index needs a GPU (no CPU fallback)")
    device = torch.device("cuda", max(args.cuda, 0))
    index = load_index(args.index_file, device, args.metric)
    before = index.ntotal
    ids = np.load(args.remove_ids_file).reshape(-1) if args.remove_ids_file else None
    if ranges or ids is not None:
        index = index.remove(ids=ids, ranges=ranges or None)
    removed, merged = before - index.ntotal, 0
    for path in args.merge:
        other = load_index(path, device, args.metric)
        index = index.merge(other)
        merged += other.ntotal
    index.save(args.out + ".part.npz")                                          # a run killed while it writes leaves no half file under --out
    os.replace(args.out + ".part.npz", args.out)
    LOGGING.info("%s: %d keys before, %d removed, %d merged, %d after -> %s", args.index_file, before, removed, merged, index.ntotal, args.out)
    print(f"Save index of {index.ntotal} keys ({before} before, {removed} removed, {merged} merged) to {args.out}")
    return args.out


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    main(get_parser().parse_args())
