"""Writes tests/golden/sampling_topp.npz: what the reference's nucleus sampling keeps and returns on seeded rows.

    python tests/golden/make_sampling_topp.py <reference tree>

``fairseq/search.py`` is loaded by path, unchanged (it imports only ``math`` and ``torch``), and ``search.Sampling`` is built on a
dictionary object with the four methods it asks for (``pad``, ``unk``, ``eos``, ``__len__``).

Stored -- data only.  For every size V in ``SIZES`` the rows ``tests/topp_ref.py:rows_for(V)`` (float32), and for every p in ``PS`` and
both dtypes (the rows as they are, and cast to float64):

  keep_<dtype>_<V>_<i>   int64 [R, width]    ``Sampling._sample_topp``'s truncated indices where its trimmed probability is > 0, else -1
  prob_<dtype>_<V>_<i>   float64 [R, width]  the trimmed probabilities (0 where trimmed)

and from ``Sampling.step(1, lprobs, scores)`` with beam 1, float32, under ``torch.manual_seed(V)``:

  step_idx_<V>_<i>   int64 [R]     the indices returned
  step_score_<V>_<i> float32 [R]   the scores returned (the history scores passed in are zero)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import topp_ref as tp  # noqa: E402

SIZES = (5, 64, 257, 4097)
PS = (0.3, 0.5, 0.79, 1.5)


class Dict4:
    def __init__(self, n):
        self.n = n

    def pad(self):
        return tp.PAD

    def unk(self):
        return 3

    def eos(self):
        return tp.EOS

    def __len__(self):
        return self.n


def main(ref):
    spec = importlib.util.spec_from_file_location("ref_search", os.path.join(ref, "fairseq", "search.py"))
    search = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(search)
    out = {"sizes": np.asarray(SIZES), "ps": np.asarray(PS)}
    for V in SIZES:
        rows = tp.rows_for(V)
        out[f"rows_{V}"] = rows
        for i, p in enumerate(PS):
            s = search.Sampling(Dict4(V), sampling_topp=p)
            for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                lprobs = torch.from_numpy(rows).to(dtype).unsqueeze(1).clone()
                probs, idx = s._sample_topp(lprobs)
                probs, idx = probs[:, 0].double().numpy(), idx[:, 0].numpy()
                out[f"keep_{name}_{V}_{i}"] = np.where(probs > 0, idx, -1).astype(np.int64)
                out[f"prob_{name}_{V}_{i}"] = probs
            torch.manual_seed(V)
            s = search.Sampling(Dict4(V), sampling_topp=p)
            scores, indices, beams = s.step(1, torch.from_numpy(rows).unsqueeze(1).clone(), torch.zeros(rows.shape[0], 1, 1))
            assert int(beams.abs().sum()) == 0
            out[f"step_idx_{V}_{i}"] = indices[:, 0].numpy().astype(np.int64)
            out[f"step_score_{V}_{i}"] = scores[:, 0].numpy().astype(np.float32)
    path = os.path.join(HERE, "sampling_topp.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
