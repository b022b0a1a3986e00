"""How a split is cut into samples: ``--sample-break-mode none | complete | complete_doc | eos``.

Host-side restatement of ``TokenBlockDataset``'s slicing (fairseq/data/token_block_dataset.py:75-105, the loops of
fairseq/data/token_block_utils_fast.pyx:50-103) and of the ``--gcn-context-window`` prefix of
``GraphTokenBlockDataset.get_basic_info`` (token_block_dataset.py:246-285), pinned against the reference's own output in
tests/golden/break_modes.npz.  ``sizes`` are the sentence lengths of ``DATA/{split}.idx``.

  none          blocks of ``block_size`` tokens, whatever the sentences
  complete      whole sentences, as many as fit ``block_size``; a sentence longer than the block is a block of its own
  complete_doc  the same, never across a document boundary: a sentence of ``document_sep_len`` tokens separates documents
                and is dropped, and so is a block that would hold a single token
  eos           one sentence per block
"""
import numpy as np

BREAK_MODES = ("none", "complete", "complete_doc", "eos")
RAGGED_MODES = BREAK_MODES[1:]


def slice_indices(sizes, break_mode, block_size, document_sep_len=1):
    """int64 [n_blocks, 2]: token range [start, end) of every sample, in corpus order."""
    mode = "none" if break_mode is None else break_mode
    if mode not in BREAK_MODES:
        raise ValueError("Invalid break_mode: " + str(break_mode))
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1)
    ends = np.cumsum(sizes)
    total = int(ends[-1]) if sizes.size else 0
    if mode == "eos":
        return np.stack([ends - sizes, ends], axis=1)
    if mode == "none":
        starts = np.arange(0, total, block_size, dtype=np.int64)
        return np.stack([starts, np.minimum(starts + block_size, total)], axis=1)
    doc = mode == "complete_doc"
    keep = 2 if doc else 1                                # complete_doc drops one-token blocks ("only keep non-empty documents")
    out, tok, cur = [], 0, 0                              # blocks so far, first token of the open block, its tokens so far
    for sz in sizes.tolist():
        sep = doc and sz == document_sep_len
        if not sep and (cur == 0 or cur + sz <= block_size):
            cur += sz
            continue
        if cur >= keep:
            out.append((tok, tok + cur))
        tok, cur = tok + cur, 0
        if sep:
            tok += sz                                     # the separator itself belongs to no block
        else:
            cur = sz                                      # the sentence that did not fit opens the next block
    if cur >= keep:
        out.append((tok, tok + cur))
    return np.asarray(out, dtype=np.int64).reshape(-1, 2)


def block_ranges(sizes, break_mode, block_size, context_window=0, document_sep_len=1):
    """``(context_start, start, end)`` of every sample of a ragged mode.  Only ``[start, end)`` is scored; with
    ``--gcn-context-window w`` sample i > 0 also carries up to ``w`` tokens in front of it, cut from the sentences of sample
    i - 1 onwards: the context starts at ``max(first token of the sentence sample i - 1 starts in, start - w)`` (for these modes
    that is sample i - 1's own start; separators dropped between the two samples lie inside the buffer and count)."""
    sl = slice_indices(sizes, break_mode, block_size, document_sep_len)
    if context_window <= 0 or len(sl) == 0:
        return [(int(s), int(s), int(e)) for s, e in sl]
    cum = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    first_sent = np.searchsorted(cum, sl[:, 0], side="right") - 1          # sentence every sample starts in
    out = [(int(sl[0, 0]), int(sl[0, 0]), int(sl[0, 1]))]
    for i in range(1, len(sl)):
        s, e = int(sl[i, 0]), int(sl[i, 1])
        out.append((max(int(cum[first_sent[i - 1]]), s - context_window), s, e))
    return out
