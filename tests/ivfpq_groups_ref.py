"""The torch reference of the task table gnnlm_ivfpq_scan8 takes (include/gnnlm.h), shared by test_mirrors_cpu.py (the table's
own properties, on the CPU) and test_ivfpq_mfma_gpu.py (the device builder gnnlm_ivfpq_build_groups against it, and a search that
runs on this table instead)."""
import torch


def build_groups(pl, nlist, seg=None):
    """(query, probe) pairs of ``pl`` [nq, P] (list ids, -1 = none) -> groups of up to 8 queries that probe the same list,
    sorted by list: grp_list [G] int32, grp_q [G, 8] int32 (-1 padded), the number of groups in use as a one-element int32
    tensor on the device.  Torch ops on the tensor's device, no host round trip; G is the upper bound pairs / 8 + nlist + 1.
    With ``seg``: also grp_out [G, 8] int64, the offset (query * P + probe slot) * seg of the pair's segment in a [nq, P, seg]
    array (-1: none).  The tuple ``IVFPQIndex._groups`` returns."""
    nq, P = pl.shape
    dev = pl.device
    n = nq * P
    key = torch.where(pl < 0, torch.full_like(pl, nlist), pl).reshape(-1)
    skey, order = torch.sort(key, stable=True)
    cnt = torch.zeros(nlist + 1, dtype=torch.int64, device=dev).scatter_add_(0, key, torch.ones_like(key))   # pairs per list (last bucket: no list); no host sync, unlike bincount
    start = torch.cumsum(cnt, 0) - cnt
    gcnt = (cnt + 7) // 8
    goff = torch.cumsum(gcnt, 0) - gcnt                                       # first group of every list
    pos = torch.arange(n, device=dev) - start[skey]                           # position inside the run of one list
    gid = goff[skey] + pos // 8
    G = n // 8 + nlist + 1
    none = skey >= nlist                                                      # pairs without a list: their groups sort last and are
    grp_list = torch.full((G,), -1, dtype=torch.int32, device=dev)            # cut off by n_groups, their entries stay -1
    grp_list[gid] = torch.where(none, torch.full_like(skey, -1), skey).to(torch.int32)
    grp_q = torch.full((G, 8), -1, dtype=torch.int32, device=dev)
    grp_q[gid, pos % 8] = torch.where(none, torch.full_like(order, -1), torch.div(order, P, rounding_mode="floor")).to(torch.int32)
    n_groups = gcnt[:nlist].sum().reshape(1).to(torch.int32)                  # (the groups of the "no list" bucket sort last: cut off)
    if seg is None:
        return grp_list, grp_q, n_groups, G
    grp_out = torch.full((G, 8), -1, dtype=torch.int64, device=dev)
    grp_out[gid, pos % 8] = torch.where(none, torch.full_like(order, -1), order * seg)   # order = query * P + slot
    return grp_list, grp_q, n_groups, G, grp_out
