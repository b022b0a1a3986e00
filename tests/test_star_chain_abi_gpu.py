"""gnnlm_star_attn / gnnlm_chain_attn at the descriptor level (include/gnnlm.h: gnnlm_star_attn_t, gnnlm_chain_attn_t): every field on
every route of the dispatch, against the float64 restatement of tests/star_chain_ref.py.  Descriptors are filled by hand and passed
to ``_lib.call_desc``; the ``ops`` wrappers are not used.  (The ctypes mirrors are generated from the header, so they carry every
field the header has: test_mirrors_carry_the_fields pins the ones used here.)

The case tables, their inputs and the routes live in star_chain_ref.py; tests/test_star_chain_ref_cpu.py shows without a GPU that each
shape takes the route written next to it and that a kernel which ignored one field of a case would miss the bar by a factor of 100
or read a poison row.  No index handed to a kernel points outside its buffer.

Bars: Z and out within 2e-5 of the reference (the bar of test_star_attn_pq / test_star_attn_dense / test_chain_attn, same input scale);
everything else exact -- has_nb, the zero rows, every element the kernels must not write (compared as bits with a NaN sentinel), and
a second call against the first."""
import ctypes
import os

import numpy as np
import pytest
import torch

import star_chain_ref as ref

pytestmark = pytest.mark.gpu

SENT_BITS = 0x7FC0BEEF                                                        # a NaN with a payload of its own
GUARD = 64
STAR_FIELDS = ["codes_direct", "codes_index", "x_index", "nb_valid", "nb_valid_stride", "n_store", "row0", "n_local", "shards", "ldx",
               "x_group_stride"]
CHAIN_FIELDS = ["radius_p1", "n_groups_dev", "kv_index", "scale", "ldo"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sentinel(n, dev):
    return torch.from_numpy(np.full(n, SENT_BITS, dtype=np.uint32).view(np.float32)).to(dev)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_mirrors_carry_the_fields():
    from gnnlm_amd import _lib
    assert set(STAR_FIELDS) <= {f for f, _ in _lib.gnnlm_star_attn_t._fields_}
    assert set(CHAIN_FIELDS) <= {f for f, _ in _lib.gnnlm_chain_attn_t._fields_}
    for name in ("gnnlm_star_attn_t", "gnnlm_chain_attn_t"):
        assert _lib.lib().gnnlm_sizeof(name.encode()) == ctypes.sizeof(getattr(_lib, name))


# ======================================================================================================== star attention
class Star:
    """gnnlm_star_attn_t over the arrays of a case of star_chain_ref.make_star_case, with the tensors it points to; Z and has_nb are
    followed by GUARD sentinel elements."""

    def __init__(self, dev, c):
        from gnnlm_amd import _lib
        self.dev, self.c, self.keep = dev, c, []
        kw = c["kw"]
        a = self.a = _lib.gnnlm_star_attn_t()
        a.U, a.ids = self.up(c["U"]), self.up(c["ids"])
        a.T, a.H, a.D, a.kg = c["T"], c["H"], c["D"], c["kg"]
        if "codes" in kw:
            a.codes = self.up(c["code_buf"]) + c["code_off"] * kw["M"]            # the window starts at row row0 of the table
            a.row0, a.n_local, a.M, a.dsub = kw.get("row0", 0), kw.get("n_local", 0), kw["M"], kw["dsub"]
            a.codes_direct, a.centroids = kw["codes_direct"], self.up(kw["centroids"])
            if kw.get("codes_index") is not None:
                a.codes_index = self.up(kw["codes_index"])
        else:
            a.X, a.ldx, a.x_group_stride = self.up(kw["X"]), kw["ldx"], kw["x_group_stride"]
        a.n_store = kw["n_store"]
        if kw.get("nb_valid") is not None:
            a.nb_valid, a.nb_valid_stride = self.up(kw["nb_valid"]), kw["nb_valid_stride"]
        if kw.get("x_index") is not None:
            a.x_index = self.up(kw["x_index"])
        # what the routes of star_chain_ref.star_route take for granted: aligned operands, the A/B switch unset
        assert all((getattr(a, f) or 0) % 16 == 0 for f in ("U", "codes", "centroids", "X"))
        assert "GNNLM_STAR_GENERIC" not in os.environ

    def up(self, x):
        t = torch.from_numpy(np.ascontiguousarray(x)).to(self.dev)
        self.keep.append(t)
        return t.data_ptr()

    def call(self):
        """-> (Z [T, H, D], has_nb [T], guard of Z, guard of has_nb) as numpy"""
        from gnnlm_amd import _lib
        c = self.c
        n = c["T"] * c["H"] * c["D"]
        Z, has = self.out = sentinel(n + GUARD, self.dev), sentinel(c["T"] + GUARD, self.dev)
        self.a.Z, self.a.has_nb = Z.data_ptr(), has.data_ptr()
        _lib.call_desc("gnnlm_star_attn", self.a)
        torch.cuda.synchronize()
        Z, has = Z.cpu().numpy(), has.cpu().numpy()
        return Z[:n].reshape(c["T"], c["H"], c["D"]), has[:c["T"]], Z[n:], has[c["T"]:]


@pytest.mark.parametrize("case", ref.STAR_CASES, ids=ref.star_case_id)
def test_star_attn_descriptor(dev, case):
    route, shape, opt = case
    c = ref.make_star_case(route, shape, opt)
    c["Z"], c["has"] = ref.star_ref(c["U"], c["ids"], **c["kw"])
    st = Star(dev, c)
    Z, has, gz, gh = st.call()
    err = float(np.abs(Z.astype(np.float64) - c["Z"]).max())
    print(f"star route={route} case={ref.star_case_id(case)}: max |Z - ref| = {err:.3e}")
    assert np.array_equal(bits(has), bits(c["has"]))
    assert err < ref.TOL
    assert (c["has"] == 0).any() or c["T"] == 1
    assert (bits(Z[c["has"] == 0]) == 0).all()                                # exactly zero without a valid neighbour
    assert (bits(gz) == SENT_BITS).all() and (bits(gh) == SENT_BITS).all()
    Z2, has2, gz2, gh2 = st.call()
    assert np.array_equal(bits(Z), bits(Z2)) and np.array_equal(bits(has), bits(has2))
    assert (bits(gz2) == SENT_BITS).all() and (bits(gh2) == SENT_BITS).all()


def test_star_attn_refusals(dev):
    """Descriptors star_attn must refuse; every buffer is large enough for the shape the descriptor claims, and nothing is written."""
    from gnnlm_amd._lib import GnnlmError

    def refused(st):
        with pytest.raises(GnnlmError):
            st.call()
        torch.cuda.synchronize()
        assert all((bits(t.cpu().numpy()) == SENT_BITS).all() for t in st.out)

    def pq(M, dsub, D=None):
        T, H, kg, D = 3, 2, 5, D or M * dsub
        rs = np.random.RandomState(M + dsub)
        kw = dict(codes=rs.randint(0, 255, size=(64, M)).astype(np.uint8), row0=0, n_local=64, M=M, dsub=dsub, codes_direct=0,
                  centroids=rs.randn(M, 256, dsub).astype(np.float32), n_store=64)
        return dict(T=T, H=H, D=D, kg=kg, U=rs.randn(T, H, D).astype(np.float32), ids=rs.randint(0, 64, size=(T, kg)).astype(np.int64),
                    kw=kw, code_buf=kw["codes"], code_off=0)

    def dense(D, ldx):
        T, H, kg = 3, 2, 5
        rs = np.random.RandomState(D)
        kw = dict(X=rs.randn(T * kg * ldx).astype(np.float32), ldx=ldx, x_group_stride=1, n_store=0)
        return dict(T=T, H=H, D=D, kg=kg, U=rs.randn(T, H, D).astype(np.float32), ids=rs.randint(0, 64, size=(T, kg)).astype(np.int64), kw=kw)

    Star(dev, pq(16, 4)).call()                                               # the descriptors below are one field away from these two
    Star(dev, dense(64, 68)).call()
    st = Star(dev, pq(16, 4))                                                 # both sources
    st.a.X, st.a.ldx, st.a.x_group_stride = st.up(np.zeros(15 * 64, dtype=np.float32)), 64, 1
    refused(st)
    st = Star(dev, pq(16, 4))                                                 # neither
    st.a.codes = None
    refused(st)
    refused(Star(dev, pq(4, 6)))                                              # dsub % 4 != 0 (M * dsub = D = 24)
    refused(Star(dev, pq(16, 4, D=128)))                                      # M * dsub != D
    refused(Star(dev, dense(1028, 1028)))                                     # D > 1024
    refused(Star(dev, dense(64, 66)))                                         # ldx % 4 != 0
    for make, field in ((lambda: pq(16, 4), "U"), (lambda: pq(16, 4), "centroids"), (lambda: pq(16, 4), "codes"), (lambda: dense(64, 68), "U")):
        st = Star(dev, make())                                                # one float off a 16-byte boundary: no kernel loads that
        setattr(st.a, field, getattr(st.a, field) + 4)
        refused(st)


# ======================================================================================================== chain attention
class Chain:
    def __init__(self, dev, c):
        from gnnlm_amd import _lib
        self.dev, self.c, self.keep = dev, c, []
        kw = c["kw"]
        d = self.d = _lib.gnnlm_chain_attn_t()
        d.Q, d.K, d.V, d.ld = self.up(c["Q"]), self.up(c["K"]), self.up(c["V"]), c["ld"]
        d.valid = self.up(c["valid"])
        d.n_groups, d.left, d.right, d.H, d.dk = kw["n_groups"], kw["left"], kw["right"], kw["H"], kw["dk"]
        d.ldo, d.radius_p1 = c["ldo"], kw["radius_p1"]
        if "scale" in kw:
            d.scale = self.up(kw["scale"])
        if "kv_index" in kw:
            d.kv_index = self.up(kw["kv_index"])
        if "n_groups_dev" in kw:
            d.n_groups_dev = self.up(np.array([kw["n_groups_dev"]], dtype=np.int32))

    up = Star.up

    def call(self):
        """-> (out [n_slots, ldo], guard) as numpy"""
        from gnnlm_amd import _lib
        c = self.c
        n = c["n_slots"] * c["ldo"]
        out = self.out = sentinel(n + GUARD, self.dev)
        self.d.out = out.data_ptr()
        _lib.call_desc("gnnlm_chain_attn", self.d)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        return out[:n].reshape(c["n_slots"], c["ldo"]), out[n:]


@pytest.mark.parametrize("case", ref.CHAIN_CASES, ids=ref.chain_case_id)
def test_chain_attn_descriptor(dev, case):
    c = ref.make_chain_case(case)
    want, mask = ref.chain_ref(c["Q"], c["K"], c["V"], c["valid"], **c["kw"])
    d = c["kw"]["H"] * c["kw"]["dk"]
    ch = Chain(dev, c)
    out, guard = ch.call()
    got = out[mask][:, :d]
    assert not np.isnan(got).any()                                            # a row that does not exist to the kernel was read
    err = float(np.abs(got.astype(np.float64) - want[mask]).max()) if mask.any() else 0.0
    print(f"chain case={ref.chain_case_id(case)}: max |out - ref| = {err:.3e}")
    assert err < ref.TOL
    assert (bits(out[mask & (c["valid"] == 0)][:, :d]) == 0).all()            # an invalid destination slot: a zero row
    assert (bits(out[~mask]) == SENT_BITS).all()                              # every other row stays as it was,
    assert (bits(out[:, d:]) == SENT_BITS).all() and (bits(guard) == SENT_BITS).all()      # and so does all that lies between and behind the rows
    out2, guard2 = ch.call()
    assert np.array_equal(bits(out), bits(out2)) and (bits(guard2) == SENT_BITS).all()


def test_chain_attn_refusals(dev):
    from gnnlm_amd._lib import GnnlmError

    def refused(c, **fields):
        ch = Chain(dev, c)
        for k, v in fields.items():
            setattr(ch.d, k, v)
        with pytest.raises(GnnlmError):
            ch.call()
        torch.cuda.synchronize()
        assert (bits(ch.out.cpu().numpy()) == SENT_BITS).all()

    Chain(dev, ref.make_chain_case(dict(left=4, right=3, dk=64, H=1, scale=True))).call()
    c = ref.make_chain_case(dict(left=4, right=4, dk=64, H=1, scale=True))    # n_g = 9 (the buffers hold nine slots per group)
    refused(c)
    c = ref.make_chain_case(dict(left=1, right=1, dk=260, H=1, scale=True))   # d_k = 260 (ld = 264)
    refused(c)
    refused(ref.make_chain_case(dict(left=1, right=1, dk=64, H=1, scale=True)), valid=None)
