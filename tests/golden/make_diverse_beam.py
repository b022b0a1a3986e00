"""Writes tests/golden/diverse_beam.npz: what the reference's two diverse search strategies return on a toy model.

    python tests/golden/make_diverse_beam.py <reference tree>

The reference's ``SequenceGenerator.generate`` (fairseq/sequence_generator.py) runs with ``search_strategy=DiverseBeamSearch(d, G, s)``
(fairseq/search.py:105-164) or ``DiverseSiblingsSearch(d, r)`` (:291-353).  The files are loaded by path, unchanged, under the stubs of
make_beam_search.py (imported from there) and one more shim: ``search.py:142`` calls ``torch.add(tensor, number, tensor)``, a
signature this torch no longer has; the module sees a ``torch`` whose ``add`` passes the number as ``alpha``.

No ``prefix_tokens`` here: under forced prefix steps the reference's penalty counts depend on which ids ``torch.topk`` returns among
``-inf`` candidates, which is unspecified.  Instead the toy model is given the prompt itself: it has an ``encoder`` that returns the
prompts (so the generator carries each row's prompt through its reorders), and its history is ``eos``, the prompt, the generated
tokens.  The generator starts from the bare ``eos``; step 0 is the first free step.  The model is make_beam_search.py's (``ToyLM`` of
tests/beam_ref.py restates it over that history).

Stored per case -- data only: A, B, w, the two prompts, the settings, and per hypothesis the tokens (the generated ones and ``eos``),
the score and ``positional_scores`` as returned.

Every case asserts that no expected result rests on ``torch.topk``'s unspecified tie order: at every step the adjacent penalised
values among each group's best 2 * beam_g + 1 finite candidates differ by at least 1e-4; for siblings the same among every
hypothesis's best 2 * beam + 1 and among the best 2 * beam + 1 penalised values.  The seeds below are ones for which that holds
(``--search`` prints the first seeds that pass).
"""
import json
import os
import sys

import numpy as np
import torch

import make_beam_search as mb
from make_beam_search import EOS, PAD, P

MARGIN = 1e-4
MAX_NEW = 6
BASE = dict(beam=4, groups=0, strength=0.5, rate=-1.0, lenpen=1.0, eos_bias=0.0, shift=False)
CASES = {
    "groups2": dict(BASE, seed=2, groups=2),
    "groups3_strength1": dict(BASE, seed=3, beam=6, groups=3, strength=1.0),
    "groups4": dict(BASE, seed=1, groups=4),
    "groups2_strength0": dict(BASE, seed=1, groups=2, strength=0.0),
    "groups2_eos_shift": dict(BASE, seed=3, groups=2, eos_bias=2.0, shift=True),
    "siblings": dict(BASE, seed=3, rate=0.5),
    "siblings_rate0": dict(BASE, seed=3, rate=0.0),
}


class _Torch(mb._Torch):
    """make_beam_search's torch, and ``add(tensor, number, tensor)`` as ``add(tensor, tensor, alpha=number)`` (search.py:142)."""

    @staticmethod
    def add(a, b, c=None, **kw):
        return torch.add(a, b, **kw) if c is None else torch.add(a, c, alpha=b, **kw)


class Encoder(torch.nn.Module):
    def forward(self, src_tokens, src_lengths):
        return src_tokens

    def reorder_encoder_out(self, encoder_out, new_order):
        return encoder_out.index_select(0, new_order)


class Toy(mb.Toy):
    def __init__(self, A, B, w):
        super().__init__(A, B, w)
        self.encoder = Encoder()

    def forward_decoder(self, tokens, encoder_out=None):
        return super().forward_decoder(torch.cat([tokens[:, :1], encoder_out, tokens[:, 1:]], 1))


def gaps_of(sorted_rows, gaps):
    for row in sorted_rows.double().reshape(-1, sorted_rows.shape[-1]):
        row = row[torch.isfinite(row)]
        if len(row) > 1:
            gaps.append(float((row[:-1] - row[1:]).min()))


def run_case(sg, search, c):
    """-> (arrays to store, the smallest gap where an order decided at any step)."""
    A, B, w, prompts = mb.tables(c["seed"], c["eos_bias"])
    gaps, beam, shifted = [], c["beam"], []

    class WatchedBeam(search.BeamSearch):
        """the beam search inside a strategy: sees one group's penalised rows (or, for siblings, step 0)"""

        def step(self, step, lprobs, scores):
            out = super().step(step, lprobs, scores)
            lp = lprobs[:, ::lprobs.shape[1], :] if step == 0 else lprobs        # (after the first step the scores were added in place)
            flat = lp.reshape(lp.shape[0], -1)
            gaps_of(torch.topk(flat, min(2 * lprobs.shape[1] + 1, flat.shape[1]), dim=1).values, gaps)
            return out

    class WatchedGroups(search.DiverseBeamSearch):
        def step(self, step, lprobs, scores):
            s, i, b = super().step(step, lprobs, scores)
            first = (i[:, :beam] == EOS) & torch.isfinite(s[:, :beam]) & (torch.arange(beam)[None, :] % self.num_groups == 0)
            shifted.append(bool(first.any()) and step < MAX_NEW)
            return s, i, b

    class WatchedSiblings(search.DiverseSiblingsSearch):
        def step(self, step, lprobs, scores):
            if step > 0:
                lp = lprobs + scores[:, :, step - 1].unsqueeze(-1)
                top = torch.topk(lp, 2 * beam + 1, dim=2).values
                gaps_of(top, gaps)
                pen = top[:, :, :2 * beam] - torch.arange(1, 2 * beam + 1, dtype=lp.dtype) * self.diversity_rate
                gaps_of(torch.topk(pen.reshape(pen.shape[0], -1), 2 * beam + 1, dim=1).values, gaps)
            return super().step(step, lprobs, scores)

    d = mb.Dictionary()
    strategy = WatchedGroups(d, c["groups"], c["strength"]) if c["groups"] > 0 else WatchedSiblings(d, c["rate"])
    strategy.beam = WatchedBeam(d)
    gen = sg.SequenceGenerator(d, beam_size=beam, max_len_a=0, max_len_b=MAX_NEW, min_len=1, normalize_scores=True, len_penalty=c["lenpen"],
                               search_strategy=strategy)
    src = torch.from_numpy(prompts)
    sample = {"net_input": {"src_tokens": src, "src_lengths": torch.full((2,), P, dtype=torch.int64)}}
    hyps = gen.generate([Toy(A, B, w)], sample)
    width = MAX_NEW + 1
    tok = np.full((2, beam, width), PAD, np.int64)
    pos = np.zeros((2, beam, width), np.float32)
    score, length, count = np.zeros((2, beam), np.float32), np.zeros((2, beam), np.int64), np.zeros(2, np.int64)
    for i, hs in enumerate(hyps):
        count[i] = len(hs)
        for f, h in enumerate(hs):
            n = len(h["tokens"])
            tok[i, f, :n], pos[i, f, :n], score[i, f], length[i, f] = h["tokens"].numpy(), h["positional_scores"].numpy(), float(h["score"]), n
            assert tok[i, f, n - 1] == EOS
    assert (count == beam).all()
    if c["shift"]:
        assert any(shifted), "no eos was finalized out of group 0 before the length limit"
    settings = {k: c[k] for k in ("seed", "beam", "groups", "strength", "rate", "lenpen", "eos_bias")}
    settings["max_new"] = MAX_NEW
    arrays = dict(A=A, B=B, w=w, prompts=prompts, tokens=tok, positional_scores=pos, scores=score, lengths=length, counts=count,
                  settings=np.asarray(json.dumps(settings)))
    return arrays, min(gaps)


def main():
    import warnings
    warnings.filterwarnings("ignore", message="An output with one or more elements was resized")
    sg, search = mb.load_reference(sys.argv[1])
    search.torch = _Torch()
    if "--search" in sys.argv:
        for name, c in CASES.items():
            ok = []
            for seed in range(1, 80):
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
        print(f"{name}: seed {c['seed']}, smallest gap where an order decided = {gap:.3e}")
        assert gap >= MARGIN, name
        out.update({f"{name}/{k}": v for k, v in arrays.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "diverse_beam.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
