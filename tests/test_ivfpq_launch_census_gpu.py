"""Which kernels one IVFPQIndex.search_device enqueues, route by route: the launches per profile id (the library's own event
profiler) of one search, against a table recorded from the search's host path as it was while ``ivfpq.py`` decided the route by
``tiles is not None`` in nine places (`PYTHONPATH=. python tests/test_ivfpq_launch_census_gpu.py` in a fresh process prints it), and
the result of the profiled call against an un-profiled one, bit for bit.  A stage that went missing, ran twice or took the other
branch changes a count; the numbers themselves are the other IVF-PQ tests' business.  Only the index's public surface is used, so
the same file runs against any earlier state of the package."""
import os

import numpy as np
import pytest
import torch

from gnnlm_amd import _lib
from gnnlm_amd.ivfpq import IVFPQIndex

pytestmark = pytest.mark.gpu

N, D, NLIST, NQ = 6000, 256, 64, 300
FAIL = dict(threshold_sample=4, sample_min_keys_per_k=0, sample_sigmas=-1e9)      # a sampled rank of 1: the threshold is too high

# route -> index arrays ("m64" / "m16"), constructor arguments, attributes set afterwards, search arguments, environment
ROUTES = {
    "int8-labels": dict(labels=True, return_vals=True),
    "int8": dict(),
    "int8-select0": dict(labels=True, return_vals=True, env={"GNNLM_IVF_SELECT": "0"}),
    "int8-k1100": dict(ctor=dict(nprobe=32), k=1100),                               # ~3000 probed keys: gnnlm_topk_merge ranks them
    "int8-cap64": dict(ctor=dict(cand_cap=64)),
    "int8-sample-rows": dict(attrs=dict(FAIL, sample_fail_frac=1.0)),
    "int8-sample-stop": dict(attrs=FAIL),
    "int8-blocks": dict(query_block=128),
    "f32-packed": dict(ctor=dict(scan="f32")),
    "l2-key_term": dict(ctor=dict(metric="l2", cosine=False)),
    "m16-ip": dict(arrays="m16", ctor=dict(scan="rowmajor")),
    "m16-l2-list_term": dict(arrays="m16", ctor=dict(scan="rowmajor", metric="l2", cosine=False)),
}

# launches per kernel id (gnnlm_kernel_name) of the profiled search; the selections of csrc/ivfpq_select.hip count as topk_merge_kernel,
# the threshold pass as ivfpq_sums_kernel.  `passes` searches through the int8 filter, `rounds` through the two-round float32 scan
GEMM, TOPK, SCAN, SCAN8, RESCORE, SUMS, TAU = (
    "gemm_nt_f32_kernel", "topk_merge_kernel", "ivfpq_scan_kernel", "ivfpq_scan8_kernel", "ivfpq_rescore_kernel", "ivfpq_sums_kernel",
    "ivfpq_tau_kernel")
int8 = lambda passes: {GEMM: 2 * passes, RESCORE: passes, SCAN8: passes, SUMS: passes, TAU: passes, TOPK: 2 * passes}
F32 = {GEMM: 3, SCAN: 2, TOPK: 3}
EXPECTED = {
    "int8-labels": int8(1),
    "int8": int8(1),
    "int8-select0": int8(1),
    "int8-k1100": int8(1),
    "int8-cap64": int8(4),                  # the call at 64 survivors and again at 128; then 16 rows on their own, at 128 and at 256
    "int8-sample-rows": int8(2),            # the call, then its rows once more with an exact threshold pass
    "int8-sample-stop": int8(2),            # the call, then the call without sampling
    "int8-blocks": int8(3),
    "f32-packed": F32,
    "l2-key_term": F32,
    "m16-ip": F32,
    "m16-l2-list_term": F32,
}


def _inputs():
    rs = np.random.RandomState(5)
    centres = rs.randn(40, D).astype(np.float32)
    keys = (centres[rs.randint(0, 40, N)] + 0.6 * rs.randn(N, D).astype(np.float32)).astype(np.float16)
    labels = rs.randint(0, 50000, N).astype(np.int32)
    q = (centres[rs.randint(0, 40, NQ)] + 0.6 * rs.randn(NQ, D).astype(np.float32)).astype(np.float32)
    return keys, labels, q / np.sqrt((q ** 2).sum(1, keepdims=True))


def make_world(dev):
    """-> (index arrays by M, labels, queries); the two builds of the module"""
    keys, labels, q = _inputs()
    arrays = {}
    for name, M in (("m64", 64), ("m16", 16)):
        b = IVFPQIndex.build(keys, NLIST, M, device=dev, cosine=True, nprobe=8, iters=3, seed=3, scan="rowmajor")
        arrays[name] = (b.R, b.coarse, b.pq, b.list_off, b.list_ids, b.list_codes)
    return arrays, torch.from_numpy(labels).to(dev), torch.from_numpy(q).to(dev)


@pytest.fixture(scope="module")
def world():
    return make_world(torch.device("cuda:0"))


def _index(r, world):
    arrays, labels, _ = world
    index = IVFPQIndex(*arrays[r.get("arrays", "m64")], **dict(dict(nprobe=8), **r.get("ctor", {})))
    for name, value in r.get("attrs", {}).items():
        setattr(index, name, value)
    return index.attach_vals(labels) if r.get("labels") else index


def census(name, world):
    """-> (launch counts of the profiled search, its result, the result of the same search un-profiled, the two indexes).  Every
    search gets an index of its own: what a search adapts for good (cand_cap, threshold_sample) starts where the constructor left it."""
    r = ROUTES[name]
    args = (world[2], r.get("k", 64), r.get("query_block"), bool(r.get("return_vals")))
    saved = {k: os.environ.get(k) for k in r.get("env", {})}
    os.environ.update(r.get("env", {}))
    try:
        plain_index = _index(r, world)
        plain = plain_index.search_device(*args)
        index = _index(r, world)
        torch.cuda.synchronize()
        _lib.profile_begin()
        try:
            out = index.search_device(*args)
        finally:
            prof = _lib.profile_end()
    finally:
        for k, v in saved.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
    return {k: v["launches"] for k, v in sorted(prof.items())}, out, plain, (index, plain_index)


@pytest.mark.parametrize("name", list(ROUTES))
def test_launches_per_kernel_id(name, world):
    counts, out, plain, (index, plain_index) = census(name, world)
    print(name, counts)
    assert counts == EXPECTED[name]
    assert len(out) == len(plain) == (3 if ROUTES[name].get("return_vals") else 2)
    for o, p in zip(out, plain):
        assert torch.equal(o, p)
    assert torch.isfinite(out[0][:, 0]).all() and (out[1][:, 0] >= 0).all() and int(out[1].max()) < N
    # the route is the one its name says, and it left the index as the un-profiled search left its own
    assert (index.tiles is not None) == name.startswith("int8") and (index.packed_codes is not None) == (name[:2] in ("f3", "l2"))
    assert (index.key_term is not None) == (name == "l2-key_term") and (index.list_term is not None) == (name == "m16-l2-list_term")
    assert (index.cand_cap, index.threshold_sample) == (plain_index.cand_cap, plain_index.threshold_sample)
    assert (index.threshold_sample == 1) == (name == "int8-sample-stop")
    requeried = int(index.stats["requeried"])
    assert requeried == int(plain_index.stats["requeried"]) and (requeried > 0) == (name in ("int8-cap64", "int8-sample-rows"))


if __name__ == "__main__":
    import pprint
    w = make_world(torch.device("cuda:0"))
    table = {}
    for name in ROUTES:
        table[name], _, _, (ix, _) = census(name, w)
        print("#", name, "requeried", int(ix.stats["requeried"]), "cand_cap", ix.cand_cap, "threshold_sample", ix.threshold_sample)
    pprint.pprint(table, width=150, sort_dicts=False)
