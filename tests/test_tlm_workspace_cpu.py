"""Workspace sizes of the base LM's two orchestrators: gnnlm_transformer_lm_workspace_bytes and
gnnlm_transformer_lm_step_workspace_bytes are host code (no launch, no allocation), so they run without a GPU on descriptors whose
pointers are dummies.  The byte counts are what callers allocate: EXPECTED was recorded from the library as it was while the forward
and the step each had a carve of their own (`PYTHONPATH=. python tests/test_tlm_workspace_cpu.py` in a fresh process, GNNLM_LIB
pointing at that build, prints the table).  The cases: the wide buffer sized by 3 d and by ffn, depth (free), no / one / many rows;
for the step, one chunk of keys, a full chunk, one key more, and the whole cache, at the narrowest and the widest head."""
import ctypes
import re

from gnnlm_amd import _lib

PTR = 0x1000                         # a non-null pointer nobody follows
CHUNK = int(re.search(r"#define\s+GNNLM_DECODE_CHUNK\s+(\d+)", open(_lib.HEADER).read()).group(1))
CAP = 3 * CHUNK + 5


def _model(d, H, ffn, L):
    return _lib.STRUCTS["gnnlm_tlm_t"](L=L, d=d, H=H, ffn=ffn, E=PTR, ld_e=d, n_vocab=50, layers=PTR)


def _io(n_tok):
    io = _lib.STRUCTS["gnnlm_tlm_io_t"](tokens=PTR, out=PTR, max_len=n_tok)
    io.blocks.n_tok, io.blocks.n_blocks = n_tok, min(n_tok, 1)
    return io


def _cache(B, d, L, cap=CAP):
    return _lib.STRUCTS["gnnlm_kv_cache_t"](k=PTR, v=PTR, ld_row=d, ld_seq=cap * d, ld_layer=B * cap * d, L=L, B=B, cap=cap, d=d, len=PTR)


def _step_io(max_len):
    return _lib.STRUCTS["gnnlm_tlm_step_io_t"](tokens=PTR, out=PTR, max_len=max_len)


# name -> (d, H, ffn, L, n_tok)
FORWARD_CASES = {f"ffn{ffn}-L{L}-n{n}": (64, 4, ffn, L, n) for ffn in (96, 256) for L in (1, 2) for n in (0, 1, 37)}
# name -> (d, H, ffn, L, B, max_len): d = 128 with H = 8 is d_k 16, with H = 1 d_k 128
STEP_CASES = {f"B{B}-dk{128 // H}-len{n}": (128, H, 256, 2, B, n) for B in (1, 4) for H in (8, 1) for n in (1, CHUNK, CHUNK + 1, CAP)}

EXPECTED = {
    "forward": {
        "ffn96-L1-n0": 256, "ffn96-L1-n1": 1792, "ffn96-L1-n37": 57088,
        "ffn96-L2-n0": 256, "ffn96-L2-n1": 1792, "ffn96-L2-n37": 57088,
        "ffn256-L1-n0": 256, "ffn256-L1-n1": 2048, "ffn256-L1-n37": 66560,
        "ffn256-L2-n0": 256, "ffn256-L2-n1": 2048, "ffn256-L2-n37": 66560,
    },
    "step": {
        "B1-dk16-len1": 3968, "B1-dk16-len128": 3968, "B1-dk16-len129": 4608, "B1-dk16-len389": 5888,
        "B1-dk128-len1": 3856, "B1-dk128-len128": 3856, "B1-dk128-len129": 4384, "B1-dk128-len389": 5440,
        "B4-dk16-len1": 15104, "B4-dk16-len128": 15104, "B4-dk16-len129": 17664, "B4-dk16-len389": 22784,
        "B4-dk128-len1": 14656, "B4-dk128-len128": 14656, "B4-dk128-len129": 16768, "B4-dk128-len389": 20992,
    },
}


def forward_bytes(d, H, ffn, L, n_tok):
    m, io = _model(d, H, ffn, L), _io(n_tok)
    return _lib.lib().gnnlm_transformer_lm_workspace_bytes(ctypes.byref(m), ctypes.byref(io))


def step_bytes(d, H, ffn, L, B, max_len, cap=CAP):
    m, c, io = _model(d, H, ffn, L), _cache(B, d, L, cap), _step_io(max_len)
    return _lib.lib().gnnlm_transformer_lm_step_workspace_bytes(ctypes.byref(m), ctypes.byref(c), ctypes.byref(io))


def measure():
    return {"forward": {name: forward_bytes(*c) for name, c in FORWARD_CASES.items()},
            "step": {name: step_bytes(*c) for name, c in STEP_CASES.items()}}


def test_workspace_sizes_are_the_recorded_ones():
    got = measure()
    assert got == EXPECTED, {k: {n: (v, EXPECTED[k].get(n)) for n, v in got[k].items() if v != EXPECTED[k].get(n)} for k in got}


def test_cases_tell_the_carve_branches_apart():
    """a case that costs what its plain neighbour costs would not notice its branch being dropped"""
    f, s = EXPECTED["forward"], EXPECTED["step"]
    for n in (1, 37):
        assert f[f"ffn96-L1-n{n}"] == f[f"ffn96-L2-n{n}"] < f[f"ffn256-L1-n{n}"] == f[f"ffn256-L2-n{n}"]      # max(3 d, ffn); depth is free
    assert f["ffn96-L1-n0"] == f["ffn256-L2-n0"] < f["ffn96-L1-n1"] < f["ffn96-L1-n37"]
    for B in (1, 4):
        for dk in (16, 128):
            a = [s[f"B{B}-dk{dk}-len{n}"] for n in (1, CHUNK, CHUNK + 1, CAP)]
            assert a[0] == a[1] < a[2] < a[3]                                                                  # whole chunks of keys
    assert s[f"B1-dk16-len{CAP}"] > s[f"B1-dk128-len{CAP}"] and s["B4-dk16-len1"] > s["B1-dk16-len1"]         # H * (d_k + 4) per chunk
    # the step's rows are the forward's, the attention scratch comes on top
    assert s["B4-dk16-len1"] > forward_bytes(128, 8, 256, 2, 4)


def test_descriptors_nobody_can_size_give_zero():
    L = _lib.lib()
    m, io = _model(64, 4, 96, 1), _io(37)
    assert L.gnnlm_transformer_lm_workspace_bytes(None, ctypes.byref(io)) == 0 and L.gnnlm_transformer_lm_workspace_bytes(ctypes.byref(m), None) == 0
    assert forward_bytes(0, 4, 96, 1, 37) == 0 and forward_bytes(-4, 4, 96, 1, 37) == 0 and forward_bytes(64, 4, 0, 1, 37) == 0
    assert forward_bytes(64, 4, 96, 1, -1) == 0
    m, c, sio = _model(128, 8, 256, 2), _cache(4, 128, 2), _step_io(1)
    for args in ((None, ctypes.byref(c), ctypes.byref(sio)), (ctypes.byref(m), None, ctypes.byref(sio)), (ctypes.byref(m), ctypes.byref(c), None)):
        assert L.gnnlm_transformer_lm_step_workspace_bytes(*args) == 0
    assert step_bytes(0, 8, 256, 2, 4, 1) == 0 and step_bytes(128, 0, 256, 2, 4, 1) == 0 and step_bytes(128, -1, 256, 2, 4, 1) == 0
    assert step_bytes(128, 8, 256, 2, 4, CAP + 1) == 0 and step_bytes(128, 8, 256, 2, 4, -1) == 0 and step_bytes(128, 8, 256, 2, -1, 1) == 0
    assert step_bytes(128, 8, 256, 2, 4, CAP) > 0 and step_bytes(128, 8, 256, 2, 0, 1) > 0                     # (the edges that do size)


if __name__ == "__main__":
    import pprint
    pprint.pprint(measure(), width=100, sort_dicts=False)
