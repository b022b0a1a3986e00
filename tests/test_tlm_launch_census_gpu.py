"""Which kernels the base LM's orchestrators enqueue: the launches per profile id (the library's own event profiler) of one call each
of the forward, the prefill, the step on the prefilled cache, the beam step, and the step on an empty cache, against a table
recorded from the library as it was while the forward and the step each held a decoder layer loop of their own
(`PYTHONPATH=tests:. python tests/test_tlm_launch_census_gpu.py` in a fresh process, GNNLM_LIB pointing at that build, prints it).
A stage that went missing, ran twice or took the other branch changes a count; the numbers themselves are the business of
test_transformer_lm_gpu.py and test_generate_gpu.py.  Also bit for bit: the profiled outputs against the un-profiled ones, the prefill
against the forward, and -- a model without a final norm, which takes the copy the profiler does not count -- `out` against
`inner_states[-1]`.

Prompts of 1, 5 and 33 tokens (33 crosses the attention's 32-row tile) in a cache of 40."""
import numpy as np
import pytest
import torch

import test_transformer_lm_gpu as base
import transformer_lm_ref as tr
from gnnlm_amd import _lib

pytestmark = pytest.mark.gpu

PROMPTS, CAP = [1, 5, 33], 40
CALLS = ("forward", "prefill", "step", "beam step", "step on an empty cache")
WANTS = {"all": (True, True), "out": (False, False)}

CAUSAL, GEMM, LN, MISC = "causal_attn_kernel", "gemm_nt_f32_kernel", "layernorm_kernel", "misc"
# (case of transformer_lm_ref.GPU_CASES, outputs wanted) -> launches per kernel id of every call of CALLS
_RELU_L2 = {CAUSAL: 2, GEMM: 8, LN: 4, MISC: 3}            # misc: the embed and the two relus; the prefill adds a cache fill per layer
_GELU_L1 = {CAUSAL: 1, GEMM: 4, LN: 4, MISC: 1}            # misc: the embed; LayerNorm: the embedding's, the layer's two, the final one
EXPECTED = {
    (1, "all"): [_RELU_L2, dict(_RELU_L2, **{MISC: 5}), _RELU_L2, _RELU_L2, _RELU_L2],
    (1, "out"): [_RELU_L2, dict(_RELU_L2, **{MISC: 5}), _RELU_L2, _RELU_L2, _RELU_L2],
    (2, "all"): [_GELU_L1, dict(_GELU_L1, **{MISC: 2}), _GELU_L1, _GELU_L1, _GELU_L1],
    (2, "out"): [_GELU_L1, dict(_GELU_L1, **{MISC: 2}), _GELU_L1, _GELU_L1, _GELU_L1],
}


def _flat(x, extra):
    out = {"out": x}
    if extra["inner_states"][-1] is not None:
        out["last_inner"] = extra["inner_states"][-1]
    if "last_ffn_input" in extra:
        out["last_ffn_input"] = extra["last_ffn_input"]
    return {k: v.clone() for k, v in out.items()}


def calls(lm, case, want, dev, profiled):
    """-> (launch counts per call or None, outputs per call)"""
    c = tr.GPU_CASES[case]
    rs = np.random.RandomState(c["seed"] + 17)
    tokens = torch.from_numpy(rs.randint(0, c["V"], size=sum(PROMPTS)).astype(np.int64)).to(dev)
    nxt = [torch.from_numpy(rs.randint(0, c["V"], size=len(PROMPTS)).astype(np.int64)).to(dev) for _ in range(2)]
    off = np.concatenate([[0], np.cumsum(PROMPTS)])
    kw = dict(want_inner=WANTS[want][0], want_ffn_input=WANTS[want][1])
    cache, empty = lm.new_cache(len(PROMPTS), CAP), lm.new_cache(len(PROMPTS), CAP)
    own = torch.arange(len(PROMPTS), device=dev, dtype=torch.int32).unsqueeze(1).expand(len(PROMPTS), CAP).contiguous()   # every slot its own rows
    todo = {
        "forward": lambda: lm.extract_features(tokens, off, **kw),
        "prefill": lambda: lm.prefill(tokens, off, cache, **kw),
        "step": lambda: lm.step(nxt[0], cache, **kw),
        "beam step": lambda: lm.step(nxt[1], cache, src=own, **kw),
        "step on an empty cache": lambda: lm.step(nxt[0], empty, **kw),
    }
    counts, outs = [], []
    for name in CALLS:
        torch.cuda.synchronize()
        if profiled:
            _lib.profile_begin()
        try:
            x, extra = todo[name]()
        finally:
            if profiled:
                counts.append({k: v["launches"] for k, v in sorted(_lib.profile_end().items())})
        outs.append(_flat(x, extra))
    lm.check_tokens()
    assert cache.len.tolist() == [n + 2 for n in PROMPTS] and empty.len.tolist() == [1] * len(PROMPTS) and int(cache.n_bad.item()) == 0
    return (counts if profiled else None), outs


def census(case, want, dev):
    c = tr.GPU_CASES[case]
    lm = base.build(tr.make_model(pos_rows=tr.PAD + 1 + CAP, **c), dev)
    with torch.no_grad():
        _, plain = calls(lm, case, want, dev, False)
        counts, outs = calls(lm, case, want, dev, True)
    return counts, outs, plain


@pytest.mark.parametrize("want", list(WANTS))
@pytest.mark.parametrize("case", [1, 2])
def test_launches_per_kernel_id(case, want):
    counts, outs, plain = census(case, want, torch.device("cuda:0"))
    print(case, want, counts)
    assert counts == EXPECTED[(case, want)]
    for o, p in zip(outs, plain):
        assert sorted(o) == sorted(p) == sorted(["out"] + (["last_inner", "last_ffn_input"] if want == "all" else []))
        assert all(torch.equal(o[k], p[k]) for k in o) and all(torch.isfinite(v).all() for v in o.values())
    forward, prefill = outs[0], outs[1]
    assert all(torch.equal(forward[k], prefill[k]) for k in forward)                       # prefill is extract_features, bit for bit
    if want == "all" and not tr.GPU_CASES[case]["final_norm"]:
        assert all(torch.equal(o["out"], o["last_inner"]) for o in outs)                    # the copy behind the last layer


if __name__ == "__main__":
    import pprint
    pprint.pprint({(case, want): census(case, want, torch.device("cuda:0"))[0] for case in (1, 2) for want in WANTS}, width=150, sort_dicts=False)
