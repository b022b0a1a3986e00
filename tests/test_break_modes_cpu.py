"""--sample-break-mode complete / complete_doc / eos on the host: the slicing against the reference's own output
(tests/golden/break_modes.npz, written by tests/golden/make_break_modes.py from the reference's compiled
``_get_slice_indices_fast``), the --gcn-context-window prefix rule, the driver's errors and the additive C ABI."""
import os
import struct

import numpy as np
import pytest

from gnnlm_amd import _lib, token_blocks
from gnnlm_amd.eval_lm import block_ranges, get_parser, sample_blocks


def test_slicing_equals_the_reference(golden):
    g = golden("break_modes")
    assert int(g["document_sep_len"]) == 1
    n = 0
    for case in g["cases"]:
        sizes = g[f"sizes_{case}"]
        for mode in g["modes"]:
            for block in g["blocks"]:
                ref = g[f"slices_{case}_{mode}_{block}"]
                got = token_blocks.slice_indices(sizes, str(mode), int(block), 1)
                assert got.dtype == np.int64 and got.shape == ref.shape and np.array_equal(got, ref), (case, mode, block)
                n += 1
    assert n >= 3 * 4 * 3
    big = g["sizes_sentences"]
    assert (big == 1).sum() >= 20 and big.max() > 256 and len(big) >= 300          # what the fixture is there to cover


def test_partition_and_dropped_separators(golden):
    g = golden("break_modes")
    for case in g["cases"]:
        sizes = g[f"sizes_{case}"].astype(np.int64)
        total = int(sizes.sum())
        cum = np.concatenate([[0], np.cumsum(sizes)])
        for block in (8, 32, 64, 256):
            for mode in ("eos", "complete"):
                sl = token_blocks.slice_indices(sizes, mode, block)
                assert sl[0, 0] == 0 and sl[-1, 1] == total and np.array_equal(sl[1:, 0], sl[:-1, 1]) and (sl[:, 1] > sl[:, 0]).all()
                assert np.isin(sl[:, 0], cum).all()                                  # cut at sentence boundaries only
            assert np.array_equal(token_blocks.slice_indices(sizes, "eos", block)[:, 1], cum[1:])
            comp = token_blocks.slice_indices(sizes, "complete", block)
            lens = comp[:, 1] - comp[:, 0]
            assert all(n <= block or n in sizes for n in lens)                      # longer than the block: one long sentence alone
            # complete_doc: what is missing are separator sentences (one token) -- and one-token documents, which the reference drops
            doc = token_blocks.slice_indices(sizes, "complete_doc", block)
            covered = np.zeros(total, bool)
            for s, e in doc:
                assert not covered[s:e].any()
                covered[s:e] = True
            sent_of = np.repeat(np.arange(len(sizes)), sizes)
            missing = np.unique(sent_of[~covered])
            assert (sizes[missing] == 1).all()
            assert set(np.nonzero(sizes == 1)[0]) <= set(missing)                  # every separator is gone
            assert (doc[:, 1] - doc[:, 0] > 1).all()


def test_quoted_case_and_none_mode():
    sizes = [5, 3, 1, 9, 4, 1, 1, 7, 2]
    want = {"complete": [[0, 8], [8, 9], [9, 18], [18, 24], [24, 31], [31, 33]],
            "complete_doc": [[0, 8], [9, 18], [18, 22], [24, 31], [31, 33]],
            "eos": [[0, 5], [5, 8], [8, 9], [9, 18], [18, 22], [22, 23], [23, 24], [24, 31], [31, 33]]}
    for mode, ref in want.items():
        assert token_blocks.slice_indices(sizes, mode, 8).tolist() == ref, mode
    for n_tok, block, w in ((33, 8, 0), (33, 8, 3), (10, 4, 3), (256, 256, 0), (7, 16, 2)):
        got = sample_blocks("/nonexistent", "test", "none", block, n_tok, w)         # `none` needs no file at all
        assert got == block_ranges(n_tok, block, w)
        assert [(s, e) for _, s, e in got] == [tuple(r) for r in token_blocks.slice_indices([n_tok], "none", block).tolist()]
    assert sample_blocks("/nonexistent", "test", None, 4, 10) == block_ranges(10, 4)


def test_unknown_mode_and_missing_index(tmp_path):
    with pytest.raises(ValueError, match="Invalid break_mode: sentence"):
        token_blocks.slice_indices([3, 4], "sentence", 8)
    with pytest.raises(ValueError, match="Invalid break_mode: sentence"):
        sample_blocks(str(tmp_path), "test", "sentence", 8, 7)
    for mode in ("eos", "complete", "complete_doc"):
        with pytest.raises(FileNotFoundError, match=r"test\.idx"):
            sample_blocks(str(tmp_path), "test", mode, 8, 7)
    sizes = np.array([3, 4], dtype=np.int32)
    with open(tmp_path / "test.idx", "wb") as f:
        f.write(b"MMIDIDX\x00\x00" + struct.pack("<QBQ", 1, 4, 2) + sizes.tobytes())
    assert sample_blocks(str(tmp_path), "test", "eos", 8, 7) == [(0, 0, 3), (3, 3, 7)]
    with pytest.raises(ValueError, match="hold 7 tokens"):
        sample_blocks(str(tmp_path), "test", "eos", 8, 9)
    assert get_parser().parse_args(["d", "--path", "p"]).sample_break_mode == "none"


def test_context_window_rule_by_hand():
    """sizes 5 3 1 9 4 1 1 7 2 (cum 0 5 8 9 18 22 23 24 31 33), window 4.
    eos: block i starts at cum[i]; its context reaches back to max(start of sentence i - 1, start - 4).
    complete_doc, block 8: [0,8] [9,18] [18,22] [24,31] [31,33].  Block [9,18): previous block starts in sentence 0 (token 0):
    max(0, 9 - 4) = 5 -- the dropped separator at token 8 lies inside the context.  Block [24,31): previous block [18,22) starts
    in sentence 4 (token 18): max(18, 20) = 20 -- tokens 22, 23 (two dropped separators) are context.  Block [18,22): previous
    block starts at 9: max(9, 14) = 14."""
    sizes = [5, 3, 1, 9, 4, 1, 1, 7, 2]
    eos = token_blocks.block_ranges(sizes, "eos", 8, 4)
    assert eos == [(0, 0, 5), (1, 5, 8), (5, 8, 9), (8, 9, 18), (14, 18, 22), (18, 22, 23), (22, 23, 24), (23, 24, 31), (27, 31, 33)]
    doc = token_blocks.block_ranges(sizes, "complete_doc", 8, 4)
    assert doc == [(0, 0, 8), (5, 9, 18), (14, 18, 22), (20, 24, 31), (27, 31, 33)]
    wide = token_blocks.block_ranges(sizes, "eos", 8, 100)                           # never further back than the previous block's sentence
    assert [c for c, _, _ in wide] == [0, 0, 5, 8, 9, 18, 22, 23, 24]
    assert token_blocks.block_ranges(sizes, "complete", 8, 0) == [(s, s, e) for s, e in token_blocks.slice_indices(sizes, "complete", 8).tolist()]


def test_abi_is_additive():
    L = _lib.lib()
    assert L.gnnlm_abi_version() == _lib.ABI_VERSION == 12
    declared = _lib.exported_symbols()
    for sym in ("gnnlm_causal_attn_varlen", "gnnlm_ragged_tiles", "gnnlm_hgt_forward_ragged", "gnnlm_hgt_workspace_bytes_ragged"):
        assert sym in declared and hasattr(L, sym), sym
    import ctypes
    assert "gnnlm_ragged_t" in _lib.STRUCTS and L.gnnlm_sizeof(b"gnnlm_ragged_t") == ctypes.sizeof(_lib.STRUCTS["gnnlm_ragged_t"]) == 32


def test_tile_table_is_heaviest_first():
    """gnnlm_ragged_tiles on the host: every (block, query tile) once, tiles of long blocks first."""
    import ctypes
    L = _lib.lib()
    off = np.array([0, 1, 33, 97, 98, 398], dtype=np.int32)                          # lengths 1 32 64 1 300
    n = L.gnnlm_ragged_tiles(off.ctypes.data, 5, None)
    assert n == 1 + 1 + 2 + 1 + 10
    t = np.empty((n, 2), dtype=np.int32)
    assert L.gnnlm_ragged_tiles(off.ctypes.data, 5, t.ctypes.data) == n
    assert sorted(map(tuple, t.tolist())) == sorted([(0, 0), (1, 0), (2, 0), (2, 1), (3, 0)] + [(4, q) for q in range(10)])
    assert (np.diff(t[:, 1]) <= 0).all() and t[0].tolist() == [4, 9]
    bad = np.array([0, 4, 4], dtype=np.int32)
    assert L.gnnlm_ragged_tiles(bad.ctypes.data, 2, None) == -1                      # an empty block
