"""Seeded inputs of the --fp16 fixture (tests/golden/hgt_fp16.npz), shared by its maker (tests/golden/make_fp16.py, which runs
the reference on them) and by the tests (which regenerate them and check the checksum the fixture carries).  Plain numpy
``RandomState`` streams of our own; nothing here comes from the reference but the NAMES and SHAPES of its HGT's parameters,
which both sides check against the module they load the values into."""
import functools

import numpy as np

# name: model dims, block shape, store.  PQ without a pre-transform (M * dsub = d): the ntgt features are centroid look-ups, exact in
# any arithmetic, so what the cases measure is the HGT itself.
HGT_CASES = {
    "d32L1": dict(d=32, H=2, L=1, T=8, kg=4, l=2, r=2, n_store=60, M=4, dsub=8, seed=101),
    "d128L3": dict(d=128, H=8, L=3, T=12, kg=6, l=2, r=2, n_store=400, M=16, dsub=8, seed=102),
    # the ntgt projections of a 2-layer model run over one row per context group (the centre's query / output rows, the next
    # layer's K / V): 64 * 320 = 20 k groups x K = 256 make them big-tile (pre-converted image) GEMMs, which need > 16256 rows
    # at N = 256; k_g = 64 gave 4 k rows and 64x64 / 128x128 tiles only.  n_store is large so that few groups merge.
    "d256L2": dict(d=256, H=8, L=2, T=64, kg=320, l=2, r=2, n_store=1000000, M=32, dsub=8, seed=103),
}
ASM_CASE = dict(vocab=5000, cutoff=[500, 2000], d=128, n=300, factor=4, seed=104)


def hgt_param_shapes(d, H, L):
    """(name, shape) of every parameter of the reference's HGT(in = hidden = out = d, 2 node types, 2 edge types), sorted by name."""
    dk = d // H
    out = []
    for i in range(L):
        for t in range(2):
            for lin in ("k_linears", "q_linears", "v_linears", "a_linears"):
                out += [(f"gcs.{i}.{lin}.{t}.weight", (d, d)), (f"gcs.{i}.{lin}.{t}.bias", (d,))]
            out += [(f"gcs.{i}.norms.{t}.weight", (d,)), (f"gcs.{i}.norms.{t}.bias", (d,))]
        out += [(f"gcs.{i}.relation_pri", (2, H)), (f"gcs.{i}.relation_att", (2, H, dk, dk)),
                (f"gcs.{i}.relation_msg", (2, H, dk, dk)), (f"gcs.{i}.skip", (2,))]
    return sorted(out)


@functools.lru_cache(maxsize=None)
def hgt_inputs(name):
    """-> dict(sd, cen, codes, nb, tgt): float32 / uint8 / int64 numpy arrays of case ``name`` (generated once; read-only by convention)."""
    c = HGT_CASES[name]
    rs = np.random.RandomState(c["seed"])
    r = lambda *s: rs.randn(*s).astype(np.float32)
    sd = {}
    for nm, shape in hgt_param_shapes(c["d"], c["H"], c["L"]):
        if nm.endswith("bias"):
            v = 0.1 * r(*shape)
        elif "norms" in nm or nm.endswith("relation_pri") or nm.endswith("skip"):
            v = 1.0 + 0.1 * r(*shape)
        else:                                              # Linear weights and the per-head relation matrices: 1 / sqrt(fan in)
            v = r(*shape) / np.float32(np.sqrt(shape[-1]))
        sd[nm] = v.astype(np.float32)
    cen = (0.5 * r(c["M"], 256, c["dsub"])).astype(np.float32)
    codes = rs.randint(0, 256, size=(c["n_store"], c["M"])).astype(np.uint8)
    nb = rs.randint(0, c["n_store"], size=(c["T"], c["kg"])).astype(np.int64)
    nb[rs.rand(*nb.shape) < 0.03] = -1
    nb[1, 1] = -1
    nb[3, :] = -1                                          # a token without a valid neighbour
    nb[0, 0], nb[2, 0] = 0, c["n_store"] - 1               # contexts clipped at both ends of the store
    tgt = r(c["T"], c["d"]).astype(np.float16).astype(np.float32)        # fp16-representable, as the stored features are
    return {"sd": sd, "cen": cen, "codes": codes, "nb": nb, "tgt": tgt}


def asm_inputs():
    """-> dict(emb, proj, class_proj, x, target): the tied adaptive softmax of ASM_CASE and 300 rows to score."""
    c = ASM_CASE
    rs = np.random.RandomState(c["seed"])
    cut = list(c["cutoff"]) + [c["vocab"]]
    emb, proj, prev = [], [], 0
    for i, hi in enumerate(cut):
        dim = int(c["d"] // c["factor"] ** i)
        emb.append((rs.randn(hi - prev, dim) * dim ** -0.5).astype(np.float32))
        proj.append(None if i == 0 else (rs.randn(c["d"], dim) * c["d"] ** -0.5).astype(np.float32))
        prev = hi
    class_proj = (rs.randn(len(cut) - 1, c["d"]) * c["d"] ** -0.5).astype(np.float32)
    x = rs.randn(c["n"], c["d"]).astype(np.float16).astype(np.float32)
    target = rs.randint(0, c["vocab"], size=c["n"]).astype(np.int64)
    target[:6] = [0, 499, 500, 1999, 2000, c["vocab"] - 1]                # both ends of every band
    return {"emb": emb, "proj": proj, "class_proj": class_proj, "x": x, "target": target}


def checksum(inputs):
    """float64 [sum, sum of |.|] over every array of an inputs dict, in sorted key order (lists / dicts flattened)."""
    s = a = 0.0

    def walk(v):
        nonlocal s, a
        if v is None:
            return
        if isinstance(v, dict):
            for k in sorted(v):
                walk(v[k])
        elif isinstance(v, (list, tuple)):
            for e in v:
                walk(e)
        else:
            x = np.asarray(v, dtype=np.float64)
            s += float(x.sum())
            a += float(np.abs(x).sum())
    walk(inputs)
    return np.array([s, a], dtype=np.float64)
