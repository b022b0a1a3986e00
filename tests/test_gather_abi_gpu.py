"""gnnlm_pq_gather_decode, gnnlm_pq_encode and gnnlm_gather_rows_peer at the descriptor level (include/gnnlm.h: gnnlm_gather_t,
gnnlm_shards_t, gnnlm_peer_gather_t): every field on both kernels of the gather, against the numpy restatement of tests/gather_ref.py.
Descriptors are filled by hand and passed to ``_lib.call_desc``; the ``ops`` wrappers are not used.

The case tables, their inputs and the routes live in gather_ref.py; tests/test_gather_ref_cpu.py shows without a GPU that each case takes
the route written next to it and that a kernel which ignored one field of a case would give other bits.  No index handed to a kernel
for a valid slot points outside its buffer.

Bars: gathered data is exact -- rows, labels, validity, the zero rows, every element the kernels must not write (a NaN / byte sentinel
in the pad columns, in the rows beyond a device-side count and in the guard behind every buffer), and a second call against the first.
The one tolerance is the derived bound B of gather_ref.encode_ref for the argmin of gnnlm_pq_encode."""
import ctypes

import numpy as np
import pytest
import torch

import gather_ref as ref

pytestmark = pytest.mark.gpu

SENT_BITS = 0x7FC0BEEF                                                        # a NaN with a payload of its own
SENT_BYTE = 0xA5
GUARD_GROUPS = 8                                                              # sentinel groups behind every gather output
GUARD = 64                                                                    # sentinel bytes behind the other outputs
GATHER_FIELDS = ["codes", "vals", "vals_itemsize", "n_store", "row0", "n_local", "M", "dsub", "centroids", "ids", "n_groups", "left", "right",
                 "out_x", "ld_x", "out_codes", "out_labels", "out_valid", "direct", "in_valid", "in_index", "shards", "n_groups_dev"]
SHARDS_FIELDS = ["n", "rows_per_rank", "base", "row0", "rows"]
PEER_FIELDS = ["shard", "shard_row0", "shard_rows", "world", "row_bytes", "rows_per_rank", "n_store", "rows", "n", "out", "out_valid"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_mirrors_carry_the_fields():
    from gnnlm_amd import _lib
    assert set(GATHER_FIELDS) <= {f for f, _ in _lib.gnnlm_gather_t._fields_}
    assert set(SHARDS_FIELDS) <= {f for f, _ in _lib.gnnlm_shards_t._fields_}
    assert set(PEER_FIELDS) <= {f for f, _ in _lib.gnnlm_peer_gather_t._fields_}
    for name in ("gnnlm_gather_t", "gnnlm_shards_t", "gnnlm_peer_gather_t"):
        assert _lib.lib().gnnlm_sizeof(name.encode()) == ctypes.sizeof(getattr(_lib, name))


class Buffers:
    def __init__(self, dev):
        self.dev, self.keep = dev, []

    def up(self, x, shift=0):
        """device address of a copy of x; shift > 0: the copy starts that many bytes behind a 16-byte boundary"""
        raw = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        if shift:
            raw = np.concatenate([np.zeros(shift, dtype=np.uint8), raw])
        t = torch.from_numpy(raw.copy()).to(self.dev)
        self.keep.append(t)
        assert t.data_ptr() % 16 == 0
        return t.data_ptr() + shift

    def sentinel(self, nbytes, byte=SENT_BYTE):
        t = torch.full((nbytes,), byte, dtype=torch.uint8, device=self.dev)
        assert t.data_ptr() % 16 == 0
        return t

    def sentinel32(self, n):
        return torch.from_numpy(np.full(n, SENT_BITS, dtype=np.uint32).view(np.int32)).to(self.dev)

    def shards(self, sh, shift=0):
        """device address of a gnnlm_shards_t over copies of the shards"""
        from gnnlm_amd import _lib
        st = _lib.gnnlm_shards_t()
        st.n, st.rows_per_rank = sh["n"], sh["rows_per_rank"]
        for g in range(sh["n"]):
            st.base[g] = None if sh["base"][g] is None else self.up(sh["base"][g])
            st.row0[g], st.rows[g] = sh["row0"][g], sh["rows"][g]
        return self.up(np.frombuffer(ctypes.string_at(ctypes.byref(st), ctypes.sizeof(st)), dtype=np.uint8))


# ======================================================================================================== gather_decode
class Gather(Buffers):
    """gnnlm_gather_t over the arrays of a case of gather_ref.make_gather_case.  Every call gets fresh outputs: sentinels, with GUARD_GROUPS
    groups of sentinel rows behind the rows of the request."""

    def __init__(self, dev, c):
        from gnnlm_amd import _lib
        super().__init__(dev)
        self.c = c
        kw = c["kw"]
        d = self.d = _lib.gnnlm_gather_t()
        d.M, d.dsub, d.left, d.right, d.n_groups = kw["M"], kw["dsub"], kw["left"], kw["right"], kw["n_groups"]
        d.n_store, d.row0, d.n_local = kw.get("n_store", 0), kw.get("row0", 0), kw.get("n_local", 0)
        if c["code_buf"] is not None:
            d.codes = self.up(c["code_buf"], kw.get("codes_mod16", 0)) + c["code_off"] * kw["M"]
            assert d.codes % 16 == kw.get("codes_mod16", 0)
        if c["vals_buf"] is not None:                                         # (vals_itemsize stays 0 without a label table)
            d.vals = self.up(c["vals_buf"]) + c["vals_off"] * c["vals_buf"].itemsize
            d.vals_itemsize = c["vals_buf"].itemsize
        if "x" in kw["outs"]:
            d.centroids = self.up(kw["centroids"])
        if "ids" in kw:
            d.ids = self.up(kw["ids"])
        if kw.get("direct"):
            d.direct, d.in_valid = 1, self.up(kw["in_valid"])
            if kw.get("in_index") is not None:
                d.in_index = self.up(kw["in_index"])
        if kw.get("shards") is not None:
            d.shards = self.shards(kw["shards"])
        if "n_groups_dev" in kw:
            d.n_groups_dev = self.up(np.array([kw["n_groups_dev"]], dtype=np.int32))

    def call(self, **overrides):
        """-> {output: numpy array with the guard rows}; overrides: descriptor fields set after the outputs (a value or a function of
        the descriptor)"""
        from gnnlm_amd import _lib
        c, kw, d = self.c, self.c["kw"], self.d
        rows = c["S"] + GUARD_GROUPS * c["n_g"]
        shift = kw.get("out_codes_mod16", 0)
        self.out = {}
        if "x" in kw["outs"]:
            self.out["x"] = self.sentinel32(rows * kw["ld_x"])
            d.out_x, d.ld_x = self.out["x"].data_ptr(), kw["ld_x"]
        if "c" in kw["outs"]:
            self.out["c"] = self.sentinel(rows * kw["M"] + 16)
            d.out_codes = self.out["c"].data_ptr() + shift
        if "l" in kw["outs"]:
            self.out["l"] = self.sentinel32(rows)
            d.out_labels = self.out["l"].data_ptr()
        if "v" in kw["outs"]:
            self.out["v"] = self.sentinel(rows)
            d.out_valid = self.out["v"].data_ptr()
        for k, v in overrides.items():
            setattr(d, k, v(d) if callable(v) else v)
        _lib.call_desc("gnnlm_pq_gather_decode", d)
        torch.cuda.synchronize()
        got = {k: t.cpu().numpy() for k, t in self.out.items()}
        if "c" in got:
            assert (got["c"][:shift] == SENT_BYTE).all() and (got["c"][shift + rows * kw["M"]:] == SENT_BYTE).all()
            got["c"] = got["c"][shift:shift + rows * kw["M"]].reshape(rows, kw["M"])
        if "x" in got:
            got["x"] = got["x"].view(np.uint32).reshape(rows, kw["ld_x"])
        return got

    def untouched(self):
        torch.cuda.synchronize()
        return all((t.cpu().numpy().view(np.uint8 if t.dtype == torch.uint8 else np.uint32) == (SENT_BYTE if t.dtype == torch.uint8 else SENT_BITS)).all()
                   for t in self.out.values())


def check_gather(c, got, want):
    """written rows equal the reference as bits; every other row, the pad columns and the guard keep the sentinel"""
    x, codes, labels, valid, written = want
    S, D = c["S"], c["D"]
    w = np.concatenate([written, np.zeros(GUARD_GROUPS * c["n_g"], dtype=bool)])
    if "x" in got:
        assert np.array_equal(got["x"][:S][written, :D], x.view(np.uint32)[written])
        assert (got["x"][~w] == SENT_BITS).all() and (got["x"][:, D:] == SENT_BITS).all()
    if "c" in got:
        assert np.array_equal(got["c"][:S][written], codes[written]) and (got["c"][~w] == SENT_BYTE).all()
    if "l" in got:
        assert np.array_equal(got["l"][:S][written], labels[written]) and (got["l"][~w].view(np.uint32) == SENT_BITS).all()
    if "v" in got:
        assert np.array_equal(got["v"][:S][written], valid[written]) and (got["v"][~w] == SENT_BYTE).all()
    assert set(got) == {"x", "c", "l", "v"} & set(c["kw"]["outs"])


@pytest.mark.parametrize("case", ref.GATHER_CASES, ids=ref.gather_case_id)
def test_gather_decode_descriptor(dev, case):
    c = ref.make_gather_case(*case)
    want = ref.gather_ref(c["kw"])
    g = Gather(dev, c)
    assert g.d.vals_itemsize == (0 if c["vals_buf"] is None else c["vals_buf"].itemsize)
    got = g.call()
    check_gather(c, got, want)
    got2 = g.call()
    assert all(np.array_equal(got[k], got2[k]) for k in got)


def small_case(**spec):
    return ref.make_gather_case("wave", dict(dict(M=16, dsub=8, outs="xclv", vals="i32", win="win", left=2, right=2, G=20), **spec))


def test_gather_decode_accepts_a_zeroed_itemsize(dev):
    """a zero-initialised descriptor without a label table: vals = NULL, vals_itemsize = 0, with and without out_labels, on both kernels"""
    for route, spec in [("rows", dict(M=16, dsub=8, outs="cl", vals=None, win="win")), ("rows", dict(M=16, dsub=8, outs="cv", vals=None, win="win")),
                        ("wave", dict(M=8, dsub=4, outs="xl", vals=None, win="win")), ("wave", dict(M=8, dsub=4, outs="x", vals=None, win="win"))]:
        c = ref.make_gather_case(route, spec)
        assert ref.gather_route(c["kw"]) == route
        g = Gather(dev, c)
        assert g.d.vals is None and g.d.vals_itemsize == 0
        got = g.call()
        check_gather(c, got, ref.gather_ref(c["kw"]))
        assert "l" not in got or (got["l"][:c["S"]] == -1).all()


def test_gather_decode_empty_request(dev):
    """n_groups = 0 with every pointer NULL is OK; with outputs set, nothing is written"""
    from gnnlm_amd import _lib
    _lib.call_desc("gnnlm_pq_gather_decode", _lib.gnnlm_gather_t())
    g = Gather(dev, small_case())
    g.call(n_groups=0, ids=None, codes=None, centroids=None, vals=None)
    assert g.untouched()


def test_gather_decode_refusals(dev):
    """Descriptors gather_decode must refuse, each one field away from one it takes; every buffer is large enough for the shape the
    descriptor claims, and nothing is written."""
    from gnnlm_amd._lib import GnnlmError

    def refused(c, **fields):
        g = Gather(dev, c)
        with pytest.raises(GnnlmError):
            g.call(**fields)
        assert g.untouched()
        return g

    check_gather(small_case(), Gather(dev, small_case()).call(), ref.gather_ref(small_case()["kw"]))
    refused(small_case(), left=-1)
    refused(small_case(), dsub=6)                                             # dsub % 4 != 0
    refused(small_case(), centroids=None)                                     # out_x without centroids
    refused(small_case(), out_x=lambda d: d.out_x + 4)                        # out_x off the 16-byte boundary
    refused(small_case(), ld_x=16 * 8 + 2)                                    # ld_x % 4 != 0
    refused(small_case(), ids=None)                                           # a store request without ids
    for size in (0, 1, 3, 8):
        refused(small_case(), vals_itemsize=size)                             # a label table that is neither int16 nor int32
    direct = small_case(direct="valid", vals=None)
    Gather(dev, direct).call()
    refused(direct, in_valid=None)                                            # direct codes without in_valid
    sh = ref.make_gather_case("wave", dict(M=16, dsub=8, outs="xclv", vals=None, shards=(3, "full"), G=20))
    check_gather(sh, Gather(dev, sh).call(), ref.gather_ref(sh["kw"]))
    g = Gather(dev, sh)
    valid = g.up(np.ones(sh["S"], dtype=np.uint8))
    with pytest.raises(GnnlmError):                                           # a shard table with direct codes
        g.call(direct=1, in_valid=valid)
    assert g.untouched()
    g = Gather(dev, sh)
    vals = g.up(np.zeros(ref.N_STORE + 1, dtype=np.int32))
    with pytest.raises(GnnlmError):                                           # a shard table with out_labels and a label table
        g.call(vals=vals, vals_itemsize=4)
    assert g.untouched()


# ======================================================================================================== pq_encode
def run_encode(dev, c, byte):
    """-> (codes [n, M], guard) with the code buffer prefilled with ``byte``"""
    from gnnlm_amd import _lib
    b = Buffers(dev)
    n, M = c["n"], c["M"]
    out = b.sentinel(n * M + GUARD, byte)
    _lib.call("gnnlm_pq_encode", b.up(c["x"]), c["ldx"], b.up(c["cen"]), b.up(c["norm2"]), M, c["dsub"], n, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out[:n * M].reshape(n, M), out[n * M:]


@pytest.mark.parametrize("case", ref.ENCODE_CASES, ids=ref.encode_case_id)
def test_pq_encode_random(dev, case):
    c = ref.make_encode_case(case)
    M, dsub = c["M"], c["dsub"]
    dist, B = ref.encode_ref(c["x"][:, :M * dsub], c["cen"], c["norm2"])
    codes, guard = run_encode(dev, c, SENT_BYTE)
    excess, share, wrong = ref.encode_judge(codes, dist, B)
    print(f"pq_encode {ref.encode_case_id(case)}: worst excess {excess:.3f} of 2 B, {100 * share:.2f} % decided exactly, {wrong} of them wrong; "
          f"shape: {100 * ref.encode_shape_share(M, dsub):.2f} %")
    assert excess <= 1.0 and wrong == 0
    assert ref.encode_shape_share(M, dsub) >= 0.95 and (share >= 0.95 or c["n"] * M < 100)
    assert (guard == SENT_BYTE).all()
    codes2, guard2 = run_encode(dev, c, SENT_BYTE ^ 0xFF)                     # another prefill: a byte left unwritten would show
    assert np.array_equal(codes, codes2) and (guard2 == SENT_BYTE ^ 0xFF).all()


@pytest.mark.parametrize("case", ref.TIE_CASES, ids=ref.encode_case_id)
def test_pq_encode_ties(dev, case):
    c = ref.make_encode_case(case)
    codes, guard = run_encode(dev, c, SENT_BYTE)
    assert np.array_equal(codes, c["want"]) and (guard == SENT_BYTE).all()    # the lowest index, exactly, for every row
    codes2, guard2 = run_encode(dev, c, SENT_BYTE ^ 0xFF)
    assert np.array_equal(codes, codes2) and (guard2 == SENT_BYTE ^ 0xFF).all()


# ======================================================================================================== gather_rows_peer
class Peer(Buffers):
    def __init__(self, dev, c):
        from gnnlm_amd import _lib
        super().__init__(dev)
        self.c = c
        kw, sh = c["kw"], c["kw"]["shards"]
        d = self.d = _lib.gnnlm_peer_gather_t()
        for g in range(sh["n"]):
            d.shard[g] = None if sh["base"][g] is None else self.up(sh["base"][g])
            d.shard_row0[g], d.shard_rows[g] = sh["row0"][g], sh["rows"][g]
        d.world, d.row_bytes, d.rows_per_rank, d.n_store = kw["world"], kw["row_bytes"], kw["rows_per_rank"], kw["n_store"]
        d.rows, d.n = self.up(kw["rows"]), kw["n"]

    def call(self, **overrides):
        """-> (out [n, row_bytes], out_valid [n] or None); the guards are checked here.  Short rows need no alignment: they start one
        byte behind a 16-byte boundary."""
        from gnnlm_amd import _lib
        kw, d = self.c["kw"], self.d
        n, rb = kw["n"], kw["row_bytes"]
        shift = 1 if rb < 16 else 0
        self.out = [self.sentinel(16 + n * rb + GUARD)] + ([self.sentinel(n + GUARD)] if kw["out_valid"] else [])
        d.out = self.out[0].data_ptr() + shift
        d.out_valid = self.out[1].data_ptr() if kw["out_valid"] else None
        for k, v in overrides.items():
            setattr(d, k, v(d) if callable(v) else v)
        _lib.call_desc("gnnlm_gather_rows_peer", d)
        torch.cuda.synchronize()
        out = self.out[0].cpu().numpy()
        assert (out[:shift] == SENT_BYTE).all() and (out[shift + n * rb:] == SENT_BYTE).all()
        valid = self.out[1].cpu().numpy() if kw["out_valid"] else None
        assert valid is None or (valid[n:] == SENT_BYTE).all()
        return out[shift:shift + n * rb].reshape(n, rb), None if valid is None else valid[:n]

    def untouched(self):
        torch.cuda.synchronize()
        return all((t.cpu().numpy() == SENT_BYTE).all() for t in self.out)


@pytest.mark.parametrize("case", ref.PEER_CASES, ids=ref.peer_case_id)
def test_gather_rows_peer_descriptor(dev, case):
    c = ref.make_peer_case(*case)
    want, want_valid = ref.peer_ref(c["kw"])
    p = Peer(dev, c)
    out, valid = p.call()
    assert np.array_equal(out, want)
    assert (valid is None) == (not c["kw"]["out_valid"]) and (valid is None or np.array_equal(valid, want_valid))
    out2, valid2 = p.call()
    assert np.array_equal(out, out2) and (valid is None or np.array_equal(valid, valid2))


def test_gather_rows_peer_refusals(dev):
    from gnnlm_amd._lib import GnnlmError

    def refused(spec, **fields):
        p = Peer(dev, ref.make_peer_case(ref.peer_route(spec["row_bytes"]), spec))
        with pytest.raises(GnnlmError):
            p.call(**fields)
        assert p.untouched()

    spec = dict(row_bytes=128, world=3, variant="full", out_valid=True)       # (the buffers are sized for 128-byte rows and 16 shards)
    Peer(dev, ref.make_peer_case("lanes<8>", spec)).call()
    for rb in (0, 20, 4112):
        refused(spec, row_bytes=rb)
    refused(spec, world=0)
    refused(dict(spec, world=16), world=17)
    refused(spec, rows_per_rank=0)
    refused(spec, n_store=0)
    refused(spec, out=lambda d: d.out + 8)                                    # a misaligned output with rows of 16 bytes or more
    refused(dict(spec, row_bytes=16), out=lambda d: d.out + 4)
    refused(spec, shard=lambda d: type(d.shard)(d.shard[0], None, d.shard[2]))         # a NULL shard that holds rows
