"""Writes tests/golden/beam_search.npz: what the reference's own beam search returns on a toy model.

    python tests/golden/make_beam_search.py <reference tree>

The reference's ``SequenceGenerator.generate`` (fairseq/sequence_generator.py) runs with its default strategy ``search.BeamSearch``
(fairseq/search.py) and the prompts as ``prefix_tokens``, as ``LanguageModelingTask.inference_step`` passes them.  Both files are
loaded by path, unchanged, under these stubs and one shim:

  * ``fairseq`` is an empty package whose ``search`` is the reference's file and whose ``utils`` is an empty module (the generator
    uses it only for alignments);
  * ``fairseq.data.data_utils`` is an empty module (used only by ``SequenceGeneratorWithAlignment``);
  * ``fairseq.models.FairseqIncrementalDecoder`` is an empty class: the toy model has no ``decoder``, so the generator takes its
    non-incremental branch and calls ``model.forward_decoder(tokens)`` with the whole history at every step -- no incremental state,
    no reorder;
  * the dictionary is an object with ``pad() = 1``, ``eos() = 2``, ``unk() = 3`` and ``len() = V``;
  * the shim: ``search.py:81`` divides integer tensors with ``torch.div(..., out=)``, which this torch refuses to round; the module
    sees a ``torch`` whose ``div`` passes ``rounding_mode="floor"`` for integer operands and is torch's own otherwise.

The model (``ToyLM`` of tests/beam_ref.py restates it): next-token logits = A[last token] + B[last but one] (the last token again
while the history holds one token) + len(history) * w, A and B seeded float32 [V, V] tables (the ``eos`` column of A shifted by the
case's ``eos_bias``), w a seeded float32 [V] vector; ``log_softmax`` in float32.  The history starts with ``eos`` (``tokens[:, 0]``).

Stored per case -- data only: A, B, w, the two prompts (equal length, no special symbols), the settings, and per hypothesis the
tokens (prompt, free tokens, ``eos``), the score and ``positional_scores`` as returned.

Every case asserts that the reference's candidates are free of ties: at every step the adjacent values among the best 2 * beam + 1
candidates of every sentence differ by at least 1e-4, so no expected result rests on ``torch.topk``'s unspecified tie order.  The seeds
below are ones for which that holds (a seed that breaks it fails the assertion; ``--search`` prints the first seeds that pass).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

PAD, EOS, UNK = 1, 2, 3
V, P = 20, 4
MARGIN = 1e-4
BASE = dict(lenpen=1.0, unnormalized=False, unkpen=0.0, min_len=1, max_len_b=P + 6, eos_bias=0.0, early=False)
CASES = {
    "beam1": dict(BASE, seed=1, beam=1),
    "beam3_lenpen": dict(BASE, seed=3, beam=3, lenpen=0.7),
    "beam5": dict(BASE, seed=3, beam=5),
    "beam5_unnormalized_unkpen": dict(BASE, seed=9, beam=5, unnormalized=True, unkpen=0.8),
    "beam3_min_len": dict(BASE, seed=2, beam=3, min_len=P + 4, eos_bias=3.0),
    "beam5_forced_eos": dict(BASE, seed=2, beam=5, max_len_b=P + 2, eos_bias=-2.0),
    "beam3_early": dict(BASE, seed=2, beam=3, eos_bias=4.0, early=True),
}


class _Torch:
    """torch, with ``div`` flooring integer operands (search.py:81)."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def div(a, b, out=None):
        if not torch.is_floating_point(a):
            return torch.div(a, b, rounding_mode="floor", out=out)
        return torch.div(a, b, out=out)


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    fairseq = types.ModuleType("fairseq")
    fairseq.__path__ = []
    utils, data, data_utils, models = (types.ModuleType(n) for n in ("fairseq.utils", "fairseq.data", "fairseq.data.data_utils", "fairseq.models"))
    data.data_utils = data_utils
    models.FairseqIncrementalDecoder = type("FairseqIncrementalDecoder", (), {})
    fairseq.utils = utils
    sys.modules.update({"fairseq": fairseq, "fairseq.utils": utils, "fairseq.data": data, "fairseq.data.data_utils": data_utils,
                        "fairseq.models": models})
    search = _load(ref, "fairseq/search.py", "fairseq.search")
    search.torch = _Torch()
    fairseq.search = search
    return _load(ref, "fairseq/sequence_generator.py", "fairseq.sequence_generator"), search


class Dictionary:
    def pad(self): return PAD
    def eos(self): return EOS
    def unk(self): return UNK
    def __len__(self): return V


def tables(seed, eos_bias):
    rs = np.random.RandomState(seed)
    A, B = (1.5 * rs.randn(V, V)).astype(np.float32), (1.5 * rs.randn(V, V)).astype(np.float32)
    w = (0.1 * rs.randn(V)).astype(np.float32)
    A[:, EOS] += np.float32(eos_bias)
    prompts = rs.randint(4, V, size=(2, P)).astype(np.int64)
    return A, B, w, prompts


class Toy(torch.nn.Module):
    def __init__(self, A, B, w):
        super().__init__()
        self.A, self.B, self.w = torch.from_numpy(A), torch.from_numpy(B), torch.from_numpy(w)

    def max_decoder_positions(self):
        return 1024

    def forward_decoder(self, tokens, encoder_out=None):
        a, b = tokens[:, -1], tokens[:, -2] if tokens.shape[1] > 1 else tokens[:, -1]
        z = self.A[a] + self.B[b] + torch.tensor(float(tokens.shape[1]), dtype=torch.float32) * self.w
        return z.unsqueeze(1), None

    def get_normalized_probs(self, net_output, log_probs):
        return torch.log_softmax(net_output[0].float(), dim=-1)


def run_case(sg, search, c):
    """-> (arrays to store, the smallest gap among the best 2 * beam + 1 candidates of any step)."""
    A, B, w, prompts = tables(c["seed"], c["eos_bias"])
    gaps = []

    class Watched(search.BeamSearch):
        def step(self, step, lprobs, scores):
            out = super().step(step, lprobs, scores)
            lp = lprobs[:, ::lprobs.shape[1], :] if step == 0 else lprobs        # (after the first step the scores were added in place)
            flat = lp.reshape(lp.shape[0], -1)
            top = torch.topk(flat, min(2 * c["beam"] + 1, flat.shape[1]), dim=1).values.double()
            for row in top:
                row = row[torch.isfinite(row)]
                if len(row) > 1:
                    gaps.append(float((row[:-1] - row[1:]).min()))
            return out

    d = Dictionary()
    gen = sg.SequenceGenerator(d, beam_size=c["beam"], max_len_a=0, max_len_b=c["max_len_b"], min_len=c["min_len"],
                               normalize_scores=not c["unnormalized"], len_penalty=c["lenpen"], unk_penalty=c["unkpen"],
                               search_strategy=Watched(d))
    src = torch.from_numpy(prompts)
    sample = {"net_input": {"src_tokens": src, "src_lengths": torch.full((2,), P, dtype=torch.int64)}}
    hyps = gen.generate([Toy(A, B, w)], sample, prefix_tokens=src)
    beam, width = c["beam"], c["max_len_b"] + 1
    tok = np.full((2, beam, width), PAD, np.int64)
    pos = np.zeros((2, beam, width), np.float32)
    score, length, count = np.zeros((2, beam), np.float32), np.zeros((2, beam), np.int64), np.zeros(2, np.int64)
    for i, hs in enumerate(hyps):
        count[i] = len(hs)
        for f, h in enumerate(hs):
            n = len(h["tokens"])
            tok[i, f, :n], pos[i, f, :n], score[i, f], length[i, f] = h["tokens"].numpy(), h["positional_scores"].numpy(), float(h["score"]), n
            assert (tok[i, f, :P] == prompts[i]).all() and tok[i, f, n - 1] == EOS
    if c["early"]:
        assert any(length[i, :count[i]].max() < width for i in range(2)), "no sentence filled its finalized slots before the length limit"
    if c["max_len_b"] < BASE["max_len_b"]:
        assert (length[:, 0] == width).any(), "the forced eos finalized nothing"
    if c["min_len"] > 1:
        assert length[length > 0].min() >= c["min_len"] + 1
    settings = {k: c[k] for k in ("seed", "beam", "lenpen", "unnormalized", "unkpen", "min_len", "max_len_b", "eos_bias")}
    arrays = dict(A=A, B=B, w=w, prompts=prompts, tokens=tok, positional_scores=pos, scores=score, lengths=length, counts=count,
                  settings=np.asarray(json.dumps(settings)))
    return arrays, min(gaps)


def main():
    import warnings
    warnings.filterwarnings("ignore", message="An output with one or more elements was resized")
    ref = sys.argv[1]
    sg, search = load_reference(ref)
    if "--search" in sys.argv:
        for name, c in CASES.items():
            ok = []
            for seed in range(1, 60):
                try:
                    _, gap = run_case(sg, search, dict(c, seed=seed))
                except AssertionError:
                    continue
                if gap >= 10 * MARGIN:
                    ok.append(seed)
                if len(ok) == 3:
                    break
            print(name, ok)
        return
    out = {}
    for name, c in CASES.items():
        arrays, gap = run_case(sg, search, c)
        print(f"{name}: seed {c['seed']}, smallest gap among the best 2 * beam + 1 candidates of a step = {gap:.3e}")
        assert gap >= MARGIN, name
        out.update({f"{name}/{k}": v for k, v in arrays.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "beam_search.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
