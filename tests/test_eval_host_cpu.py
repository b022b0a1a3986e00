"""The host rules the two evaluation drivers share (``eval_lm`` with and without ``--graph``): batch planning, the
``--save-knnlm-dstore`` writer, the break-mode and ``--remove-bpe`` checks, the closing report.  Expected values are written out."""
import json
import logging
import math

import numpy as np
import pytest
import torch

from gnnlm_amd.eval_lm import (DstoreWriter, budget_batches, check_break_mode, equal_length_batches, get_parser, report_result,
                               word_output_setup, write_result_json)


def parse(*flags):
    return get_parser().parse_args(["data", "--path", "ckpt"] + list(flags))


def test_budget_batches():
    assert budget_batches([5], 4) == [(0, 1)]                                       # an over-long item alone
    assert budget_batches([2, 2, 2], 4) == [(0, 2), (2, 3)]                         # exact fit, then the rest
    assert budget_batches([3, 2, 2], 4) == [(0, 1), (1, 3)]
    assert budget_batches([1, 1, 1], 100, 1) == [(0, 1), (1, 2), (2, 3)]
    assert budget_batches([1, 1, 1], 100, 0) == [(0, 3)]
    assert budget_batches([1, 1, 1], 100, None) == [(0, 3)]
    assert budget_batches([9, 1, 9, 1, 1], 4, 2) == [(0, 1), (1, 2), (2, 3), (3, 5)]
    assert budget_batches([], 4) == []


def test_equal_length_batches():
    # (context start, start, end, sample id): lengths 4 4 3 4 with the context in front counted
    blocks = [(0, 0, 4, 0), (2, 4, 6, 1), (5, 6, 8, 2), (6, 8, 10, 3)]
    ids = lambda batches: [[b[3] for b in g] for g in batches]
    assert ids(equal_length_batches(blocks, 2)) == [[0, 1], [2], [3]]
    assert ids(equal_length_batches(blocks, 1)) == [[0], [1], [2], [3]]
    assert ids(equal_length_batches(blocks[:2] + blocks[3:], 2)) == [[0, 1], [3]]   # the cap, not the lengths, ends the first batch
    assert equal_length_batches(blocks, 2)[0] == blocks[:2]                          # the blocks themselves, unchanged
    assert equal_length_batches([], 2) == []


@pytest.mark.parametrize("fp16,vocab,kdt,vdt", [(True, 100, np.float16, np.int16), (True, 40000, np.float16, np.int32),
                                                (False, 100, np.float32, np.int32), (False, 40000, np.float32, np.int32)])
def test_dstore_writer(tmp_path, caplog, fp16, vocab, kdt, vdt):
    g = torch.Generator().manual_seed(3)
    keys = torch.randn(6, 4, generator=g) * 3.0
    vals = torch.tensor([5, 99, 0, vocab - 1, 7, 8])
    with caplog.at_level(logging.INFO, logger="gnnlm_amd.eval_lm"):
        wr = DstoreWriter(str(tmp_path), "valid", "gcn_feat", 5, 4, vocab, fp16)
        assert wr.dir == str(tmp_path / "valid_dstore-gcn_feat")
        wr.append(keys[:3], vals[:3], 0)
        assert wr.idx == 3 and not [r for r in caplog.records if r.levelno >= logging.WARNING]
        wr.append(keys[3:], vals[3:], torch.tensor([17])[0])                        # (the --graph driver hands in a 0-d tensor)
        assert wr.idx == 5
        with pytest.raises(ValueError, match="the scorer returned 3-dimensional keys, the datastore was opened for 4"):
            wr.append(keys[:1, :3], vals[:1], 0)
        wr.close()
    warnings = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING]
    assert warnings == ["exceed offset at sample 17"]
    infos = [r.getMessage() for r in caplog.records if r.levelno == logging.INFO]
    info = {"dstore_size": 5, "hidden_size": 4, "vocab_size": vocab, "dstore_fp16": fp16, "val_size": 1}
    assert infos == ["keytype being saved: gcn_feat", f"dstore info: {info}", f"Saved 5 data to {wr.dir}"]
    text = open(tmp_path / "valid_dstore-gcn_feat" / "info.json").read()
    assert json.loads(text) == info and text == json.dumps(info, indent=4, sort_keys=True)
    got_k = np.memmap(tmp_path / "valid_dstore-gcn_feat" / "keys.npy", mode="r", dtype=kdt, shape=(5, 4))
    got_v = np.memmap(tmp_path / "valid_dstore-gcn_feat" / "vals.npy", mode="r", dtype=vdt, shape=(5, 1))
    want_k = keys[:5].to(torch.float16 if fp16 else torch.float32).numpy()
    assert got_k.tobytes() == want_k.tobytes()
    assert got_v[:, 0].tolist() == [5, 99, 0, vocab - 1, 7]
    assert (tmp_path / "valid_dstore-gcn_feat" / "keys.npy").stat().st_size == 5 * 4 * np.dtype(kdt).itemsize
    assert (tmp_path / "valid_dstore-gcn_feat" / "vals.npy").stat().st_size == 5 * np.dtype(vdt).itemsize


@pytest.mark.parametrize("keytype", [None, ""])
def test_dstore_writer_without_key_type(tmp_path, keytype):
    wr = DstoreWriter(str(tmp_path), "train", keytype, 2, 3, 10, False)
    assert wr.dir == str(tmp_path / "train_dstore")
    wr.append(torch.ones(2, 3), torch.tensor([1, 2]), 0)
    wr.close()
    assert sorted(p.name for p in (tmp_path / "train_dstore").iterdir()) == ["info.json", "keys.npy", "vals.npy"]


def test_report_result(capsys, caplog):
    with caplog.at_level(logging.INFO, logger="gnnlm_amd.eval_lm"):
        ppl = report_result(-1000.0 * math.log(2), 500, 512, 2.0)
    lines = ["Evaluated 512 tokens in 2.0s (256.00 tokens/s)", "Loss (base 2): 2.0000, Perplexity: 4.00"]
    assert capsys.readouterr().out.splitlines() == lines
    assert [r.getMessage() for r in caplog.records] == lines
    assert ppl == pytest.approx(4.0, rel=1e-12)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="gnnlm_amd.eval_lm"):
        assert report_result(-1000.0 * math.log(2), 500, 512, 2.0, quiet=True) == ppl       # a rank that does not report
    assert capsys.readouterr().out == "" and not caplog.records
    report_result(-3.0, 7, 7, 0.0)                                                  # no time measured: no division by zero
    assert capsys.readouterr().out.splitlines() == ["Evaluated 7 tokens in 0.0s (7000000000.00 tokens/s)",
                                                    "Loss (base 2): 0.6183, Perplexity: 1.54"]


def test_write_result_json(tmp_path):
    res = {"score_sum": -1.5, "count": 3, "word_stats": {"a": object()}, "rank": 0}
    want = {"score_sum": -1.5, "count": 3, "rank": 0}
    one = tmp_path / "one.json"
    write_result_json(str(one), res)
    assert json.load(open(one)) == want and not (tmp_path / "one.json.rank0").exists()
    r1 = tmp_path / "r1.json"
    write_result_json(str(r1), res, rank=1, world=2)
    assert json.load(open(str(r1) + ".rank1")) == want and not r1.exists()
    r0 = tmp_path / "r0.json"
    write_result_json(str(r0), res, rank=0, world=2)
    assert json.load(open(r0)) == want and json.load(open(str(r0) + ".rank0")) == want
    write_result_json(None, res)                                                    # no --result-json: nothing to do
    assert sorted(p.name for p in tmp_path.iterdir()) == ["one.json", "r0.json", "r0.json.rank0", "r1.json.rank1"]


def test_check_break_mode():
    assert check_break_mode(parse()) == "none"
    assert check_break_mode(parse("--sample-break-mode", "")) == "none"
    for mode in ("none", "complete", "complete_doc", "eos"):
        assert check_break_mode(parse("--sample-break-mode", mode)) == mode
    with pytest.raises(ValueError, match="^Invalid break_mode: sentence$"):
        check_break_mode(parse("--sample-break-mode", "sentence"))
    with pytest.raises(ValueError, match="complete_doc drops the document separators"):
        check_break_mode(parse("--sample-break-mode", "complete_doc", "--save-knnlm-dstore"))
    assert check_break_mode(parse("--sample-break-mode", "complete", "--save-knnlm-dstore")) == "complete"


def test_word_output_setup(tmp_path):
    data = str(tmp_path)
    assert word_output_setup(parse()) == (None, None, 0)
    with pytest.raises(NotImplementedError):
        word_output_setup(parse("--remove-bpe", "sentencepiece"))
    args = parse("--remove-bpe")
    args.data = data
    with pytest.raises(ValueError, match="--remove-bpe needs the data directory's dict.txt"):
        word_output_setup(args)
    args = parse("--output-word-stats")
    args.data = data
    assert word_output_setup(args) == (None, None, 0)                               # no dict.txt: words are printed as ids
    (tmp_path / "dict.txt").write_text("the 10\nhel@@ 5\nlo 5\n@@x 1\n", encoding="utf-8")
    symbols = ["<s>", "<pad>", "</s>", "<unk>", "the", "hel@@", "lo", "@@x"]
    assert word_output_setup(args) == (symbols, None, 0)
    args = parse("--remove-bpe")                                                    # the flag's own value "@@ ", stripped on the right
    args.data = data
    assert word_output_setup(args) == (symbols, {5}, 2)
    args = parse("--remove-bpe", "lo")
    args.data = data
    assert word_output_setup(args) == (symbols, {6}, 2)
