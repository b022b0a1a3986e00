"""Host logic of the kNN-LM tuning sweep: the three flags, the order of the grid points, the printed lines and the C ABI's
declarations.  No GPU."""
import math
import os
import re
from argparse import Namespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["DATA", "--path", "CKPT", "--graph", "--use-precompute-feat"]
KNN = ["--knnlm", "--k", "8", "--lmbda", "0.25", "--temperature", "0.5"]


def parse(extra):
    from gnnlm_amd import eval_lm
    return eval_lm.parse_sweep(eval_lm.get_parser().parse_args(BASE + extra))


def test_no_sweep_is_none():
    from gnnlm_amd import eval_lm
    assert parse([]) is None and parse(KNN) is None
    # a namespace that does not know the options at all (bench.py builds its own)
    assert eval_lm.parse_sweep(Namespace(knnlm=True, k=8, lmbda=0.25, temperature=1.0)) is None


def test_lists_and_defaults():
    assert parse(KNN + ["--sweep-lmbda", "0,0.1, 0.25,1"]) == ([8], [0.5], [0.0, 0.1, 0.25, 1.0])
    assert parse(KNN + ["--sweep-temperature", "1.0,0.1"]) == ([8], [1.0, 0.1], [0.25])
    assert parse(KNN + ["--sweep-k", "4,8,1"]) == ([4, 8, 1], [0.5], [0.25])
    assert parse(KNN + ["--sweep-k", "4", "--sweep-temperature", "2", "--sweep-lmbda", "0.5"]) == ([4], [2.0], [0.5])
    # --lmbda 0 with a sweep is a sweep (the search still runs)
    assert parse(["--knnlm", "--k", "8", "--sweep-lmbda", "0.1"]) == ([8], [1.0], [0.1])


@pytest.mark.parametrize("extra, msg", [
    (["--sweep-lmbda", "0.1"], "need --knnlm"),                                  # no --knnlm
    (KNN + ["--sweep-lmbda", "0.1,x"], "comma-separated"),
    (KNN + ["--sweep-lmbda", ""], "comma-separated"),
    (KNN + ["--sweep-lmbda", "0.1,,0.2"], "comma-separated"),
    (KNN + ["--sweep-k", "4.5"], "comma-separated list of integers"),
    (KNN + ["--sweep-k", "4,9"], "1 .. --k"),
    (KNN + ["--sweep-k", "0"], "1 .. --k"),
    (KNN + ["--sweep-temperature", "0"], "> 0"),
    (KNN + ["--sweep-temperature", "-1"], "> 0"),
    (KNN + ["--sweep-temperature", "nan"], "> 0"),
    (KNN + ["--sweep-lmbda", "1.5"], "0 .. 1"),
    (KNN + ["--sweep-lmbda", "-0.1"], "0 .. 1"),
    (KNN + ["--sweep-lmbda", "nan"], "0 .. 1"),
    (KNN + ["--sweep-lmbda", "0.1,0.1"], "repeated"),
    (KNN + ["--sweep-k", ",".join(["1"] * 9)], "at most 8"),
    (KNN + ["--sweep-temperature", ",".join(str(1 + j) for j in range(17))], "at most 16"),
    (KNN + ["--sweep-lmbda", ",".join(str(j / 32) for j in range(17))], "at most 16"),
    (["--knnlm", "--k", "2048", "--sweep-lmbda", "0.1"], "1024"),
    (["--save-knnlm-dstore", "--dstore-mmap", "X", "--sweep-lmbda", "0.1"], "--knnlm"),
    (["--knnlm", "--save-knnlm-dstore", "--dstore-mmap", "X", "--sweep-lmbda", "0.1"], "--save-knnlm-dstore"),
])
def test_refused_before_any_device_work(extra, msg):
    with pytest.raises(ValueError, match=msg):
        parse(extra)


def test_point_order_is_one_order_everywhere():
    """k slowest, lmbda fastest: ops.grid_points, the driver's table and the C header say the same."""
    from gnnlm_amd import eval_lm, ops
    sweep = ([4, 8], [1.0, 0.1], [0.0, 0.1, 0.25])
    pts = ops.grid_points(*sweep)
    assert pts == [(k, t, l) for k in sweep[0] for t in sweep[1] for l in sweep[2]]
    assert pts[0] == (4, 1.0, 0.0) and pts[1] == (4, 1.0, 0.1) and pts[3] == (4, 0.1, 0.0) and pts[6] == (8, 1.0, 0.0)
    for g, (k, t, l) in enumerate(pts):                 # the header's formula
        assert g == (sweep[0].index(k) * len(sweep[1]) + sweep[1].index(t)) * len(sweep[2]) + sweep[2].index(l)
    rows = eval_lm.sweep_table(sweep, [-(100.0 + g) for g in range(12)], 41)
    assert [(r["k"], r["temperature"], r["lmbda"]) for r in rows] == pts
    assert all(set(r) >= {"k", "temperature", "lmbda", "score_sum", "ppl"} for r in rows)
    assert rows[5]["score_sum"] == -105.0 and rows[5]["ppl"] == 2 ** (105.0 / 41 / math.log(2))
    hdr = open(os.path.join(ROOT, "include", "gnnlm.h")).read()
    assert "g = (ik * n_temperatures + it) * n_lmbdas + il" in hdr


def test_sweep_lines():
    from gnnlm_amd import eval_lm
    sweep = ([4, 1024], [1.0, 0.01], [0.0, 0.25])
    rows = eval_lm.sweep_table(sweep, [-200.0, -190.0, -200.0, -150.0, -200.0, -185.0, -200.0, -150.5], 50)
    lines = eval_lm.sweep_lines(rows)
    assert len(lines) == 8
    loss = 150.0 / 50 / math.log(2)
    assert lines[3] == "sweep k=4 temperature=0.01 lmbda=0.25 loss={:.4f} ppl={:.2f}  <- best".format(loss, 2 ** loss)
    assert lines[0] == "sweep k=4 temperature=1 lmbda=0 loss={:.4f} ppl={:.2f}".format(200.0 / 50 / math.log(2), 2 ** (200.0 / 50 / math.log(2)))
    assert sum(l_.endswith("<- best") for l_ in lines) == 1
    pat = re.compile(r"^sweep k=\d+ temperature=\S+ lmbda=\S+ loss=-?\d+\.\d{4} ppl=\d+\.\d{2}(  <- best)?$")
    assert all(pat.match(l_) for l_ in lines)


def test_header_declares_the_entry_points():
    from gnnlm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gnnlm.h")).read()
    assert re.search(r"#define\s+GNNLM_ABI_VERSION\s+12\b", hdr) and _lib.ABI_VERSION == 12
    syms = _lib.exported_symbols()
    assert "gnnlm_knn_interp_grid" in syms and "gnnlm_rows_sum_f64" in syms
    st = _lib.STRUCTS["gnnlm_knn_interp_grid_t"]
    f = dict(st._fields_)
    assert len(f["ks"]()) >= 8 and len(f["temperatures"]()) >= 16 and len(f["lmbdas"]()) >= 16
    assert {"n_ks", "n_temperatures", "n_lmbdas", "out_logp", "out_pknn", "out_recall", "knn_vals"} <= set(f)
    assert eval_lm_caps() == (len(f["ks"]()), len(f["temperatures"]()), len(f["lmbdas"]()))


def eval_lm_caps():
    from gnnlm_amd import eval_lm
    return eval_lm.SWEEP_MAX["k"], eval_lm.SWEEP_MAX["temperature"], eval_lm.SWEEP_MAX["lmbda"]
