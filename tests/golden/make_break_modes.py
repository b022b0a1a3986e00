#!/usr/bin/env python3
"""Generate tests/golden/break_modes.npz by RUNNING THE REFERENCE'S OWN slicing code.

    python tests/golden/make_break_modes.py <reference source tree>

What is executed from the reference tree (nothing of it is copied into this repo, nothing compiled from it is kept):
  * fairseq/data/token_block_utils_fast.pyx   compiled where it lies with ``pyximport`` (Cython) into a TEMPORARY build
                                              directory that is removed again; ``_get_slice_indices_fast`` and
                                              ``_get_block_to_dataset_index_fast`` are called on seeded sentence sizes

Outputs are arrays only: the seeded sizes, and for every (case, mode, block size) the slice indices and the block -> sentence
index the reference returned.  Key layout: ``sizes_<case>``, ``slices_<case>_<mode>_<block>``, ``b2d_<case>_<mode>_<block>``;
``cases`` / ``modes`` / ``blocks`` list what is there.
"""
import importlib.util
import os
import shutil
import sys
import tempfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
MODES = ("complete", "complete_doc", "eos")
BLOCKS = (8, 32, 64, 256)
DOCUMENT_SEP_LEN = 1


def make_sizes():
    """Seeded sentence sizes: a few hundred sentences, some of one token (document separators to complete_doc), some longer
    than every block size, runs of separators, a separator first and last."""
    rng = np.random.RandomState(20240611)
    cases = {"quoted": np.array([5, 3, 1, 9, 4, 1, 1, 7, 2], dtype=np.int64)}
    a = rng.geometric(1.0 / 27.0, size=300).astype(np.int64)
    a[rng.choice(300, 25, replace=False)] = 1
    a[rng.choice(300, 6, replace=False)] = rng.randint(257, 700, size=6)
    cases["sentences"] = a
    b = rng.randint(1, 61, size=200).astype(np.int64)
    b[[0, 1, 57, 58, 59, 199]] = 1
    b[[20, 120]] = (300, 65)
    cases["edges"] = b
    cases["short"] = rng.randint(1, 4, size=120).astype(np.int64)
    return cases


def load_reference(ref, build_dir):
    import pyximport
    pyximport.install(setup_args={"include_dirs": [np.get_include()]}, build_dir=build_dir, inplace=False, language_level=3)
    path = os.path.join(ref, "fairseq", "data", "token_block_utils_fast.pyx")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    sys.path.insert(0, os.path.dirname(path))
    try:
        return importlib.import_module("token_block_utils_fast")
    finally:
        sys.path.pop(0)


def main(ref):
    build_dir = tempfile.mkdtemp(prefix="break_modes_build_")
    try:
        mod = load_reference(ref, build_dir)
        cases = make_sizes()
        out = {"cases": np.array(sorted(cases)), "modes": np.array(MODES), "blocks": np.array(BLOCKS, dtype=np.int64),
               "document_sep_len": np.array(DOCUMENT_SEP_LEN, dtype=np.int64)}
        for name, sizes in cases.items():
            out[f"sizes_{name}"] = sizes
            for mode in MODES:
                for block in BLOCKS:
                    sl = np.asarray(mod._get_slice_indices_fast(sizes, mode, int(block), DOCUMENT_SEP_LEN), dtype=np.int64).reshape(-1, 2)
                    out[f"slices_{name}_{mode}_{block}"] = sl
                    out[f"b2d_{name}_{mode}_{block}"] = np.asarray(mod._get_block_to_dataset_index_fast(sizes, sl), dtype=np.int64).reshape(-1, 3)
        path = os.path.join(OUT, "break_modes.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")
    finally:
        shutil.rmtree(build_dir, ignore_errors=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
