"""Batches of blocks of UNEQUAL length (``--sample-break-mode eos | complete | complete_doc``), packed back to back.

The reference pads the ragged samples and batches their graphs as a disjoint union (monolingual_dataset.py:237-261); here the
tokens of a batch are one run of rows and a ``gnnlm_ragged_t`` cuts it into the blocks the causal attention stays inside.  The
lengths are host-known, so the tables -- block offsets and the (block, query tile) work list of ``gnnlm_causal_attn_varlen`` --
are built on the host and go to the device ONCE per :class:`BlockTable` (a driver builds one for the whole split and its batches
are views into it: nothing per batch over PCIe).
"""
import ctypes

import numpy as np
import torch

from . import _lib


class RaggedBatch:
    """One batch of a :class:`BlockTable`: blocks ``[b0, b1)``.  ``block_off`` / ``tiles`` are device views, ``lengths`` /
    ``offsets`` (batch-relative, ``[n_blocks + 1]``) live on the host."""

    def __init__(self, table, block_off, tiles, lengths):
        self.table, self.block_off, self.tiles = table, block_off, tiles
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.n_blocks, self.n_tiles, self.n_tok = int(self.lengths.shape[0]), int(tiles.shape[0]), int(self.offsets[-1])
        self._seg = None

    def desc(self):
        d = _lib.gnnlm_ragged_t()
        d.block_off, d.tiles = self.block_off.data_ptr(), self.tiles.data_ptr()
        d.n_blocks, d.n_tiles, d.n_tok = self.n_blocks, self.n_tiles, self.n_tok
        return d

    @property
    def segment_ids(self):
        """int64 [n_tok] on the device: the block of every row (built on first use from the device offsets, no host data)."""
        if self._seg is None:
            off = (self.block_off[1:-1] - self.block_off[0]).to(torch.int64)
            rows = torch.arange(self.n_tok, device=self.block_off.device)
            self._seg = torch.bucketize(rows, off, right=True)
        return self._seg


class BlockTable:
    """Block and tile tables of a sequence of blocks, uploaded once.  ``lengths``: tokens per block (each >= 1); ``batches``: list of
    ``(b0, b1)`` block ranges that will be scored together (default: all blocks as one batch)."""

    def __init__(self, lengths, device, batches=None):
        lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
        if lengths.size == 0 or lengths.min() < 1:
            raise ValueError("BlockTable: every block needs at least one token")
        off = np.concatenate([[0], np.cumsum(lengths)])
        if off[-1] >= 2 ** 31:
            raise ValueError("BlockTable: more than 2^31 - 1 tokens in one table")
        self.lengths, self.off_host = lengths, np.ascontiguousarray(off, dtype=np.int32)
        self.batches = [(0, len(lengths))] if batches is None else [(int(a), int(b)) for a, b in batches]
        L = _lib.lib()
        L.gnnlm_ragged_tiles.restype = ctypes.c_int64
        L.gnnlm_ragged_tiles.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        parts, self.tile_start = [], [0]
        for b0, b1 in self.batches:
            if not 0 <= b0 < b1 <= len(lengths):
                raise ValueError(f"BlockTable: bad batch ({b0}, {b1})")
            sub = np.ascontiguousarray(self.off_host[b0:b1 + 1])
            n = L.gnnlm_ragged_tiles(sub.ctypes.data, b1 - b0, None)
            t = np.empty((n, 2), dtype=np.int32)
            if L.gnnlm_ragged_tiles(sub.ctypes.data, b1 - b0, t.ctypes.data) != n:
                raise _lib.GnnlmError("gnnlm_ragged_tiles failed")
            parts.append(t)
            self.tile_start.append(self.tile_start[-1] + n)
        self.off_dev = torch.from_numpy(self.off_host).to(device)
        self.tiles_dev = torch.from_numpy(np.concatenate(parts)).to(device)

    def __len__(self):
        return len(self.batches)

    def batch(self, i=0):
        b0, b1 = self.batches[i]
        return RaggedBatch(self, self.off_dev[b0:b1 + 1], self.tiles_dev[self.tile_start[i]:self.tile_start[i + 1]], self.lengths[b0:b1])


def packed_rows(off, first, n):
    """Row list of ``n = off[-1] - off[0]`` packed rows on the device: row j of segment b (``off`` int [n_seg + 1], device) is
    ``first[b] + (j - (off[b] - off[0]))``.  Pure device arithmetic on resident tables: no host data, no synchronisation."""
    rel = (off - off[0]).to(torch.int64)
    j = torch.arange(n, device=off.device)
    seg = torch.bucketize(j, rel[1:-1], right=True)
    return first.to(torch.int64)[seg] + j - rel[seg]


def as_ragged(block_off, device):
    """``NeighborGraph.block_off`` / ``BlockBatch.block_off``: a :class:`RaggedBatch`, or offsets ``[n_blocks + 1]`` (host sequence or
    tensor; a convenience that uploads a table per call -- drivers build one :class:`BlockTable`)."""
    if block_off is None or isinstance(block_off, RaggedBatch):
        return block_off
    off = block_off.detach().cpu().numpy() if torch.is_tensor(block_off) else np.asarray(block_off)
    off = off.astype(np.int64).reshape(-1)
    if off.size < 2:
        raise ValueError("block_off: need at least one block")
    return BlockTable(np.diff(off), device).batch(0)
