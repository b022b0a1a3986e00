"""csrc/ivfpq8_layout.h against the host that allocates the int8 IVF-PQ search's buffers (IVFPQIndex in gnnlm_amd/ivfpq.py), without a
device.  The header is asked through tests/ivfpq8_layout_main.cpp, built with the host compiler alone; the expected values on this
side are written by hand from the documented layout, so a change on one side only fails here:

    a group = 8 queries; a histogram = 1024 bins of 16 (sum_u 0 .. 16320); a survivor counter = one 64-byte line of 16 int32;
    a query's byte table = 2 x 256 x 32 bytes; a survivor record = {row, list | sum << 18}, row < 2^19 inside its list;
    task-table rows = n * P // 8 + nlist + 1; scan grid = min(8 ceil(groups / 8), 8 ceil(max(cus, 8) / 8));
    LDS: threshold pass 128 KiB tables + 8 x 1024 x 4 = 160 KiB, filter 128 KiB + 768 + 16 waves x 240 x 8, re-score 64 KiB + 1024 x 64.
"""
import os
import re
import shutil
import subprocess

import pytest

from gnnlm_amd.ivfpq import IVFPQIndex

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gnn-lm_amd", "csrc")


@pytest.fixture(scope="module")
def layout_program(tmp_path_factory):
    """tests/ivfpq8_layout_main.cpp: csrc/ivfpq8_layout.h behind a command line, built with the host compiler alone"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not found")
    exe = str(tmp_path_factory.mktemp("ivfpq8_layout") / "ivfpq8_layout_main")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(HERE, "ivfpq8_layout_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def ask(exe, mode, rows=()):
    r = subprocess.run([exe, mode], input="".join(" ".join(str(v) for v in row) + "\n" for row in rows), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = [l.split() for l in r.stdout.split("\n")[:-1]]
    assert not rows or len(out) == len(rows)
    return out


@pytest.fixture(scope="module")
def constants(layout_program):
    return {k: int(v) for k, v in ask(layout_program, "constants")}


def test_constants_by_value(constants):
    """every constant of the header, by the value the layout documents"""
    assert constants == dict(QG=8, TQ=32, QLUT_BYTES=2 * 256 * 32, TAB_BYTES=128 * 1024, WAVE_CAP=240, SCAN_CTL=768,
                             SCAN_LDS=128 * 1024 + 768 + 16 * 240 * 8, HIST_BINS=1024, HIST_SHIFT=4, SUMS_LDS=160 * 1024,
                             SURV_CNT_STRIDE=16, SURV_ROW_BITS=19, SURV_LIST_BITS=18, SURV_EXCESS_MAX=254, SURV_SUM_BIG=16383)


def test_index_constants_are_the_headers(constants):
    """what IVFPQIndex allocates by: bins, counter stride, queries per group, the byte table, the record's bit widths"""
    ix = IVFPQIndex
    assert ix.HIST_BINS == constants["HIST_BINS"]
    assert ix.CNT_STRIDE == constants["SURV_CNT_STRIDE"]
    assert ix.QG == constants["QG"]
    assert ix.QLUT_SHAPE == (2, 256, 32) and ix.QLUT_SHAPE[0] * ix.QLUT_SHAPE[1] * ix.QLUT_SHAPE[2] == constants["QLUT_BYTES"]
    assert constants["TAB_BYTES"] == ix.QG * constants["QLUT_BYTES"]
    assert ix.QMETA == 4 and ix.WORK_CTR_SHAPE == (8, 16)
    assert (ix.SURV_ROW_BITS, ix.SURV_LIST_BITS) == (constants["SURV_ROW_BITS"], constants["SURV_LIST_BITS"])
    # the histogram covers every integer sum: 64 bytes of 0 .. 255
    assert (64 * 255) >> constants["HIST_SHIFT"] < constants["HIST_BINS"]
    # ... and gnnlm_ivfpq_scan8 refuses what the record cannot hold, in these words
    src = open(os.path.join(CSRC, "ivfpq8_scan.hip")).read()
    m = re.search(r"the survivor records hold (\d+) bits of list and (\d+) bits of row: need 0 < nlist <= 2\^(\d+) and max_list < 2\^(\d+)", src)
    assert m, "the refusal text of ivfpq_scan8"
    assert [int(g) for g in m.groups()] == [ix.SURV_LIST_BITS, ix.SURV_ROW_BITS, ix.SURV_LIST_BITS, ix.SURV_ROW_BITS]
    assert "d.nlist <= (1 << SURV_LIST_BITS)" in src and "d.max_list < (1ll << SURV_ROW_BITS)" in src


def test_choose_route_follows_the_record():
    """an index whose lists or list count outgrow the record leaves the int8 route"""
    from gnnlm_amd.ivfpq import choose_route
    assert choose_route(64, 10 ** 6, (1 << 19) - 1, 1 << 18, None, "ip", 4 << 30)[0] == "int8"
    assert choose_route(64, 10 ** 6, 1 << 19, 1 << 18, None, "ip", 4 << 30)[0] != "int8"
    assert choose_route(64, 10 ** 6, (1 << 19) - 1, (1 << 18) + 1, None, "ip", 4 << 30)[0] != "int8"


def test_group_capacity(layout_program):
    cases = [(n, P, nlist) for n in (0, 1, 7, 8, 9, 4096) for P in (1, 6, 32) for nlist in (1, 17, 4096)]
    for (n, P, nlist), (G, fill) in zip(cases, ask(layout_program, "groups", cases)):
        assert IVFPQIndex.n_groups_cap(n, P, nlist) == int(G) == n * P // 8 + nlist + 1, (n, P, nlist)
        assert int(fill) == max(8 * int(G), 2 * (nlist + 1)), (n, P, nlist)      # one thread per slot of grp_q, or per scratch word
        assert int(G) >= -(-n * P // 8) and int(G) >= min(n * P, nlist)            # (enough for full groups + one partial per list)


def test_record_round_trip(layout_program):
    cases = [(row, lst, s) for row in (0, (1 << 19) - 1) for lst in (0, (1 << 18) - 1) for s in (0, 16320, 16383)]
    for (row, lst, s), got in zip(cases, ask(layout_program, "pack", cases)):
        w0, w1, l_back, s_back = (int(v) for v in got)
        assert (w0, w1) == (row, lst | s << 18), (row, lst, s)                     # the documented {row, list | sum << 18}
        assert (l_back, s_back) == (lst, s) and w1 < 1 << 32


def test_scan_grid(layout_program):
    cases = [(g, cus) for g in (1, 8, 9, 255, 256, 257, 10 ** 6) for cus in (1, 8, 256)]
    for (g, cus), (grid,) in zip(cases, ask(layout_program, "grid", cases)):
        want = min(8 * -(-g // 8), 8 * -(-max(cus, 8) // 8))
        assert int(grid) == want and int(grid) % 8 == 0 and int(grid) >= 8, (g, cus)   # the kernel's XCD arithmetic: b % 8, b / 8


def test_lds_and_tables_grid(layout_program, constants):
    lds = {k: int(v) for k, v in ask(layout_program, "lds")}
    assert lds["sums"] == 160 * 1024 == constants["SUMS_LDS"]
    assert lds["scan"] == constants["SCAN_LDS"] <= 160 * 1024
    assert lds["rescore"] == 128 * 1024 == 64 * 256 * 4 + 1024 * 64
    ns = [(0,), (1,), (31,), (32,), (33,), (32768,)]
    assert [int(g) for (g,) in ask(layout_program, "tables", ns)] == [0, 1, 1, 1, 2, 1024]
