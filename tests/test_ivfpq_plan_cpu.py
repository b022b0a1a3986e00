"""The arithmetic of the IVF-PQ search's host path, without a device: ``plan_search`` (every per-call quantity) and ``choose_route``
(which kernels an index is searched with) of gnnlm_amd.ivfpq.  The expected values are worked out by hand from the expressions
the search used while they were spread over ``_search_once`` / ``_search_block`` / ``_search_block_mfma``:

    nprobe = min(nprobe, nlist);  dense = max(1, min(dense_probes, nprobe));  ccap = min(cap, 16384) on the int8 route, else cap
    query_block (None) = GNNLM_IVF_QUERY_BLOCK or 32768 on the int8 route, else 1024
    qb = query_block on the int8 route, else max(1, min(query_block, score_bytes // (4 * dense * max_list)))
    S = threshold_sample if dense < nprobe and ntotal / nlist * dense >= sample_min_keys_per_k * k, else 1
    rank = k if S == 1, else max(1, min(k, ceil(k / S) + ceil(sample_sigmas * sqrt(k * (S - 1)) / S)))
    fold = labels attached and int8 route and k <= 1024 and GNNLM_IVF_SELECT != "0"
"""
import pytest

from gnnlm_amd.ivfpq import SearchNumbers, choose_route, plan_search

# the reference's index (OPQ64_1024,IVF4096,PQ64 over 103 M keys) on the int8 route, defaults of the constructor, environment unset
BIG = SearchNumbers(route="int8", nprobe=32, nlist=4096, ntotal=103_227_021, max_list=60_000, score_bytes=6 << 30, has_vals=True,
                    threshold_sample=4, sample_min_keys_per_k=64, sample_sigmas=4.5, select=True, env_query_block=32768)
SMALL = BIG._replace(ntotal=6000, nlist=64)


def plan(ix, k=1024, dense_probes=6, cap=32768, **kw):
    return plan_search(ix, k, dense_probes, cap, **kw)


def test_reference_shape():
    p = plan(BIG)                                   # 151 211 keys in 6 lists >= 64 * 1024; 256 + ceil(4.5 * sqrt(3072) / 4 = 62.4)
    assert (p.k, p.nprobe, p.dense, p.S, p.rank, p.cap, p.ccap, p.query_block, p.qb) == (1024, 32, 6, 4, 319, 32768, 16384, 32768, 32768)
    p = plan(BIG, k=64)                             # 16 + ceil(4.5 * sqrt(192) / 4 = 15.6)
    assert (p.S, p.rank) == (4, 32)


def test_sampling_needs_keys_behind_the_threshold_and_lists_behind_it():
    p = plan(SMALL, k=64)                           # 562.5 keys in the dense lists < 64 * 64
    assert (p.S, p.rank) == (1, 64)
    p = plan(BIG, dense_probes=32)                  # nothing behind the threshold
    assert (p.dense, p.S, p.rank) == (32, 1, 1024)
    p = plan(BIG._replace(nlist=4))
    assert (p.nprobe, p.dense, p.S) == (4, 4, 1)
    p = plan(BIG, dense_probes=0)
    assert p.dense == 1
    p = plan(SMALL._replace(sample_min_keys_per_k=0, sample_sigmas=-1e9), k=64)   # a margin far below zero: the best of the sample
    assert (p.S, p.rank) == (4, 1)
    assert plan(BIG._replace(threshold_sample=1)).rank == 1024


def test_candidate_columns():
    assert plan(BIG, cap=64).ccap == 64
    assert plan(BIG, cap=65536).ccap == 16384 and plan(BIG, cap=65536).cap == 65536
    assert plan(BIG._replace(route="packed"), cap=16384).ccap == 16384
    assert plan(BIG._replace(route="rowmajor"), cap=65536).ccap == 65536


def test_query_blocks():
    f32 = BIG._replace(route="packed", max_list=1_000_000)
    p = plan(f32, dense_probes=2)                   # (6 << 30) // (4 * 2 * 1 000 000) = 805
    assert (p.query_block, p.qb) == (1024, 805)
    p = plan(f32._replace(max_list=1000), dense_probes=2)
    assert (p.query_block, p.qb) == (1024, 1024)
    assert plan(f32._replace(max_list=0, score_bytes=0), dense_probes=2).qb == 1
    assert plan(f32._replace(route="rowmajor"), dense_probes=2, query_block=300).qb == 300
    p = plan(BIG._replace(env_query_block=8192))    # the int8 route: the environment's block, whatever the lists' lengths
    assert (p.query_block, p.qb) == (8192, 8192)
    p = plan(BIG._replace(env_query_block=8192), query_block=128)
    assert (p.query_block, p.qb) == (128, 128)


def test_who_splits_the_payloads():
    assert plan(BIG).fold is True and plan(BIG).select is True
    assert plan(BIG._replace(has_vals=False)).fold is False
    assert plan(BIG._replace(route="packed")).fold is False
    assert plan(BIG, k=1025).fold is False
    assert plan(BIG._replace(select=False)).fold is False and plan(BIG._replace(select=False)).select is False
    # rows searched again: the state of the pass they belong to
    assert plan(BIG, k=1025, fold=True).fold is True and plan(BIG, fold=False).fold is False


@pytest.mark.parametrize("scan", [None, "f32", "rowmajor"])
@pytest.mark.parametrize("M", [16, 32, 64])
def test_route_inner_product(M, scan):
    want = "rowmajor" if scan == "rowmajor" or M == 16 else "int8" if M == 64 and scan is None else "packed"
    assert choose_route(M, 6000, 200, 64, scan) == (want, None)
    assert choose_route(M, 0, 0, 64, scan) == ("rowmajor", None)                     # no keys: nothing to pack


def test_route_int8_limits():
    """a survivor record addresses 2^19 rows of 2^18 lists, row numbers are 32 bits: beyond any of them the packed float32 scan"""
    assert choose_route(64, (1 << 32) - 1, (1 << 19) - 1, 1 << 18) == ("int8", None)
    assert choose_route(64, 1 << 32, 200, 64) == ("packed", None)
    assert choose_route(64, 6000, 1 << 19, 64) == ("packed", None)
    assert choose_route(64, 6000, 200, (1 << 18) + 1) == ("packed", None)


@pytest.mark.parametrize("scan", [None, "f32", "rowmajor"])
@pytest.mark.parametrize("M", [16, 32, 64])
def test_route_l2(M, scan):
    """the per-list table while it fits (nlist * M KiB), else one float per key; M = 64 takes the packed scan with the key's float
    unless the row-major scan is asked for; never the int8 filter"""
    nlist = 64
    fits, beyond = nlist * M * 1024, nlist * M * 1024 - 1
    packed = M == 64 and scan != "rowmajor"
    assert choose_route(M, 6000, 200, nlist, scan, "l2", fits) == (("packed", "key_term") if packed else ("rowmajor", "list_term"))
    assert choose_route(M, 6000, 200, nlist, scan, "l2", beyond) == ("packed" if packed else "rowmajor", "key_term")
    assert choose_route(M, 0, 0, nlist, scan, "l2", beyond) == ("rowmajor", None)      # no keys: no float per key, nothing to pack
