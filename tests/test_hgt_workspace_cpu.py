"""Workspace sizes of the two orchestrators that carve their own scratch: gnnlm_hgt_workspace_bytes, gnnlm_hgt_workspace_bytes_ragged
and gnnlm_adaptive_workspace_bytes are host code (no launch, no allocation), so they run without a GPU on descriptors whose
pointers are dummies.  The byte counts are part of what callers see: EXPECTED was recorded from the library as it was before the
carves were moved out of api.hip (`PYTHONPATH=. python tests/test_hgt_workspace_cpu.py` in a fresh process, GNNLM_LIB pointing at that
build, prints the table), and every branch of the HGT carve has a case."""
import ctypes

from gnnlm_amd import _lib

PTR = 0x1000                         # a non-null pointer nobody follows
D, H, M, DSUB, T, KG, LEFT, RIGHT, NB = 64, 4, 8, 8, 8, 6, 2, 2, 3
N_TOK = NB * T


def _layers(n, folded=False):
    arr = (_lib.STRUCTS["gnnlm_hgt_layer_t"] * n)()
    if folded:                       # the size function reads layers[0]'s rotation-folded weights (row-keyed K / V)
        for f in ("wq_n0", "bq_n0", "wk_n0", "bk_n0", "wv_n0", "bv_n0"):
            setattr(arr[0], f, PTR)
    return arr


def _hgt(n_layers=1, m=M, folded=False, **kw):
    layers = _layers(n_layers, folded)
    desc = _lib.STRUCTS["gnnlm_hgt_t"](d=D, n_heads=H, n_layers=n_layers, left=LEFT, right=RIGHT, M=m, dsub=DSUB, n_store=1000,
                                       layers=ctypes.addressof(layers), **kw)
    desc._keep = layers
    return desc


def _io(n_blocks=NB, t=T, kg=KG, **kw):
    return _lib.STRUCTS["gnnlm_hgt_io_t"](n_blocks=n_blocks, T=t, kg=kg, **kw)


def _merged(**kw):
    return _io(group_ids=PTR, group_index=PTR, n_unique=N_TOK * KG, **kw)


# name -> (model, io, ragged block table or None)
HGT_CASES = {
    "L1": (_hgt(1), _io(), None),
    "L1-out_ntgt": (_hgt(1), _io(out_ntgt=PTR), None),
    "L2": (_hgt(2), _io(), None),
    "L3": (_hgt(3), _io(), None),
    "L2-merged": (_hgt(2), _merged(), None),
    "L2-merged-count-on-device": (_hgt(2), _merged(n_unique_dev=PTR), None),
    "L2-merged-fetched": (_hgt(2), _merged(fetched_codes=PTR, fetched_valid=PTR), None),
    "L2-merged-fetched-cache": (_hgt(2), _merged(fetched_codes=PTR, fetched_valid=PTR, state_cache=PTR, cache_cap=512, group_slot=PTR,
                                                 code_cache=PTR), None),
    "L2-merged-cache": (_hgt(2), _merged(state_cache=PTR, cache_cap=512, group_slot=PTR), None),
    "L2-row-keyed": (_hgt(2, folded=True, opq_at=PTR), _merged(n_unique_dev=PTR, row_table=PTR), None),
    "L2-row-keyed-off-no-table": (_hgt(2, folded=True, opq_at=PTR), _merged(n_unique_dev=PTR), None),
    "L2-row-keyed-off-no-fold": (_hgt(2, opq_at=PTR), _merged(n_unique_dev=PTR, row_table=PTR), None),
    "L1-token-kg<=d": (_hgt(1, token_embed=PTR, ld_token_embed=D, n_vocab=100), _io(), None),
    "L1-token-kg>d": (_hgt(1, token_embed=PTR, ld_token_embed=D, n_vocab=100), _io(kg=D + 2), None),
    "L2-token": (_hgt(2, token_embed=PTR, ld_token_embed=D, n_vocab=100), _io(), None),
    "L2-wide-pq": (_hgt(2, m=16), _io(), None),
    "L2-dense0-wide-pq": (_hgt(2, m=16), _io(ntgt_feats=PTR, ld_ntgt=D, ntgt_valid=PTR), None),      # the carve's own, wider, dpq
    "L2-dense0": (_hgt(2), _io(ntgt_feats=PTR, ld_ntgt=D, ntgt_valid=PTR, out_ntgt=PTR), None),
    "L2-ragged": (_hgt(2), _io(n_blocks=1, t=14), _lib.STRUCTS["gnnlm_ragged_t"](block_off=PTR, tiles=PTR, n_blocks=3, n_tiles=3, n_tok=14)),
    "L1-ragged": (_hgt(1), _io(n_blocks=1, t=14), _lib.STRUCTS["gnnlm_ragged_t"](block_off=PTR, tiles=PTR, n_blocks=3, n_tiles=3, n_tok=14)),
    "L2-no-blocks": (_hgt(2), _io(n_blocks=0), None),
    "L2-no-tokens": (_hgt(2), _io(t=0), None),
    "L2-T-not-multiple-of-4": (_hgt(2), _io(t=7), None),
}


def _adaptive(cutoff, dim):
    w = _lib.STRUCTS["gnnlm_adaptive_softmax_t"](d=D, n_bands=len(cutoff), head_w=PTR)
    for i, c in enumerate(cutoff):
        w.cutoff[i] = c
        w.dim[i] = dim[i]
    return w


# name -> (weights, rows)
ADAPTIVE_CASES = {
    "1-band": (_adaptive([300], [0]), 24),
    "3-bands": (_adaptive([100, 300, 1000], [0, 32, 16]), 24),
    "tail-wider-than-head": (_adaptive([100, 5000], [0, 16]), 24),
    "no-rows": (_adaptive([100, 300, 1000], [0, 32, 16]), 0),
}

EXPECTED = {
    "hgt": {
        "L1": 101728,
        "L1-out_ntgt": 1030208,
        "L2": 1030208,
        "L3": 1030208,
        "L2-merged": 1030208,
        "L2-merged-count-on-device": 1034304,
        "L2-merged-fetched": 1030976,
        "L2-merged-fetched-cache": 1030208,
        "L2-merged-cache": 1030208,
        "L2-row-keyed": 1238784,
        "L2-row-keyed-off-no-table": 1034304,
        "L2-row-keyed-off-no-fold": 1034304,
        "L1-token-kg<=d": 101728,
        "L1-token-kg>d": 108224,
        "L2-token": 1030208,
        "L2-wide-pq": 2000960,
        "L2-dense0-wide-pq": 2000960,
        "L2-dense0": 1030208,
        "L2-ragged": 599440,
        "L1-ragged": 57656,
        "L2-no-blocks": 256,
        "L2-no-tokens": 256,
        "L2-T-not-multiple-of-4": 902360,
    },
    "adaptive": {"1-band": 3936, "3-bands": 8032, "tail-wider-than-head": 19296, "no-rows": 512},
}


def measure():
    L = _lib.lib()
    hgt = {}
    for name, (m, io, rg) in HGT_CASES.items():
        if rg is None:
            hgt[name] = L.gnnlm_hgt_workspace_bytes(ctypes.byref(m), ctypes.byref(io))
        else:
            hgt[name] = L.gnnlm_hgt_workspace_bytes_ragged(ctypes.byref(m), ctypes.byref(io), ctypes.byref(rg))
    ada = {name: L.gnnlm_adaptive_workspace_bytes(ctypes.byref(w), n) for name, (w, n) in ADAPTIVE_CASES.items()}
    return {"hgt": hgt, "adaptive": ada}


def test_workspace_sizes_are_the_recorded_ones():
    got = measure()
    assert got == EXPECTED, {k: {n: (v, EXPECTED[k].get(n)) for n, v in got[k].items() if v != EXPECTED[k].get(n)} for k in got}


def test_cases_tell_the_carve_branches_apart():
    """a case that costs what its plain neighbour costs would not notice its branch being dropped"""
    e = EXPECTED["hgt"]
    assert e["L1"] < e["L1-out_ntgt"] == e["L2"] == e["L3"]                                           # the ntgt buffers; depth is free
    assert e["L2-merged"] < e["L2-merged-count-on-device"]                                            # win_counts
    assert e["L2-merged-fetched-cache"] == e["L2-merged-cache"] == e["L2-merged"] < e["L2-merged-fetched"]     # nb_row only without a cache
    assert e["L2-row-keyed-off-no-table"] == e["L2-row-keyed-off-no-fold"] == e["L2-merged-count-on-device"] < e["L2-row-keyed"]
    assert e["L1-token-kg<=d"] == e["L1"]                                                             # the labels live in aout
    m, io = _hgt(1), _io(kg=D + 2)
    assert e["L1-token-kg>d"] > _lib.lib().gnnlm_hgt_workspace_bytes(ctypes.byref(m), ctypes.byref(io))       # ... or on their own
    assert e["L2"] < e["L2-wide-pq"] == e["L2-dense0-wide-pq"]                                        # the carve ignores ntgt_feats
    assert e["L1-ragged"] < e["L2-ragged"] and e["L2-no-blocks"] == e["L2-no-tokens"] == 256
    a = EXPECTED["adaptive"]
    assert a["no-rows"] < a["1-band"] < a["3-bands"] < a["tail-wider-than-head"]


def test_null_descriptors_size_to_zero():
    L = _lib.lib()
    m, io, _ = HGT_CASES["L2"]
    assert L.gnnlm_hgt_workspace_bytes(None, ctypes.byref(io)) == 0 and L.gnnlm_hgt_workspace_bytes(ctypes.byref(m), None) == 0
    assert L.gnnlm_hgt_workspace_bytes_ragged(ctypes.byref(m), ctypes.byref(io), None) == 0
    assert L.gnnlm_adaptive_workspace_bytes(None, 8) == 0


if __name__ == "__main__":
    import pprint
    pprint.pprint(measure(), width=100, sort_dicts=False)
