"""``--reinit-nfeat`` without a GPU: the ABI additions, the driver's parser and refusals, the checkpoint key handling."""
import ctypes
from argparse import Namespace

import pytest
import torch

from gnnlm_amd import _lib


def test_abi_is_still_12_and_additive():
    L = _lib.lib()
    assert L.gnnlm_abi_version() == _lib.ABI_VERSION == 12
    syms = _lib.exported_symbols()
    for s in ("gnnlm_token_gather", "gnnlm_neighbor_labels"):
        assert s in syms and hasattr(L, s)


def test_descriptor_mirrors():
    L = _lib.lib()
    for name in ("gnnlm_token_gather_t", "gnnlm_hgt_t", "gnnlm_star_attn_t", "gnnlm_gather_t"):
        assert L.gnnlm_sizeof(name.encode()) == ctypes.sizeof(_lib.STRUCTS[name]) > 0, name
    tg = [f for f, _ in _lib.gnnlm_token_gather_t._fields_]
    assert tg == ["ids", "n_groups", "left", "right", "n_store", "vals", "vals_itemsize", "n_vocab", "d", "embed", "ld_embed",
                  "out_x", "ld_x", "out_labels", "out_valid", "n_groups_dev"]
    # the grown descriptor: the new members are the LAST ones (nothing before them moved), zero = off
    h = [f for f, _ in _lib.gnnlm_hgt_t._fields_]
    assert h[-3:] == ["token_embed", "ld_token_embed", "n_vocab"] and h[-4] == "shards"
    m = _lib.gnnlm_hgt_t()
    assert not m.token_embed and m.ld_token_embed == 0 and m.n_vocab == 0
    assert _lib.gnnlm_hgt_t.shards.offset == 128 and _lib.gnnlm_hgt_t.token_embed.offset == 136       # (the pre-existing layout ends at 136)


def test_parser_and_refusals():
    from gnnlm_amd import eval_lm
    p = eval_lm.get_parser()
    assert p.parse_args(["data", "--path", "m.pt"]).reinit_nfeat is False
    a = p.parse_args(["data", "--path", "m.pt", "--reinit-nfeat"])
    assert a.reinit_nfeat is True and a.store == "auto"
    eval_lm.check_store_mode(a)
    for mode in ("sharded", "peer"):
        b = p.parse_args(["data", "--path", "m.pt", "--reinit-nfeat", "--store", mode])
        with pytest.raises(ValueError, match=f"--store {mode} with --reinit-nfeat"):
            eval_lm.check_store_mode(b)
        eval_lm.check_store_mode(p.parse_args(["data", "--path", "m.pt", "--store", mode]))       # without the flag: as before
    eval_lm.check_store_mode(p.parse_args(["data", "--path", "m.pt", "--reinit-nfeat", "--store", "replicated"]))


def test_out_of_range_label_is_refused():
    from gnnlm_amd import eval_lm
    vals = torch.tensor([3, 0, 23, 5, 24, 7, -1], dtype=torch.int32)
    eval_lm.check_labels(vals[:4], 24)
    with pytest.raises(ValueError, match=r"row 4 = 24"):
        eval_lm.check_labels(vals, 24)
    with pytest.raises(ValueError, match=r"row 6 = -1"):
        eval_lm.check_labels(torch.tensor([3, 0, 23, 5, 7, 7, -1], dtype=torch.int32), 24)
    with pytest.raises(ValueError, match=r"row 1 = 300"):
        eval_lm.check_labels(torch.tensor([3, 300, 400], dtype=torch.int16), 24)


def _sd(kind):
    g = torch.Generator().manual_seed(0)
    if kind == "plain":
        return {"decoder.embed_tokens.weight": torch.randn(24, 32, generator=g)}
    sd = {}
    for i, (size, dim) in enumerate([(8, 32), (8, 8), (8, 2)]):
        sd[f"decoder.embed_tokens.embeddings.{i}.0.weight"] = torch.randn(size, dim, generator=g)
        sd[f"decoder.embed_tokens.embeddings.{i}.1.weight"] = torch.randn(32, dim, generator=g)
    return sd


def test_state_dict_keys():
    from gnnlm_amd.token_embed import TokenEmbedding, band_weights, check_bands
    kind, bands = band_weights(_sd("adaptive"))
    assert kind == "adaptive" and [tuple(e.shape) for e, _ in bands] == [(8, 32), (8, 8), (8, 2)]
    assert [tuple(p.shape) for _, p in bands] == [(32, 32), (32, 8), (32, 2)]                     # band 0 has a projection of its own
    check_bands(bands, [8, 16])
    with pytest.raises(ValueError, match="band 0"):
        check_bands(bands, [10, 16])
    kind, w = band_weights(_sd("plain"))
    assert kind == "plain" and tuple(w.shape) == (24, 32)
    sd = _sd("adaptive")
    del sd["decoder.embed_tokens.embeddings.0.1.weight"]                                          # what the adaptive softmax never reads
    with pytest.raises(ValueError, match="projection"):
        band_weights(sd)
    with pytest.raises(ValueError, match="neither"):
        band_weights({"decoder.adaptive_softmax.head.class_proj.weight": torch.zeros(2, 32)})
    # up to the point a device is needed: no silent host table
    for k in ("adaptive", "plain"):
        with pytest.raises(_lib.GnnlmError, match="device"):
            TokenEmbedding.from_state_dict(_sd(k), Namespace(), device=None)
        with pytest.raises(_lib.GnnlmError, match="device"):
            TokenEmbedding.from_state_dict(_sd(k), Namespace(), device="cpu")


def test_token_store_and_errors():
    from gnnlm_amd.hgt import CodeStore, TokenStore, is_token_store, store_table
    st = TokenStore(embed=torch.zeros(24, 32), vals=torch.zeros(50, dtype=torch.int32), n_store=50)
    assert is_token_store(st) and st.n_vocab == 24 and st.row0 == 0 and st.codes is None and st.centroids is None and st.shards is None
    assert store_table(st) is st.embed
    cs = CodeStore(codes=torch.zeros(5, 4, dtype=torch.uint8), centroids=torch.zeros(4, 256, 4), n_store=5)
    assert not is_token_store(cs) and store_table(cs) is cs.codes


def test_no_quantizer_error_names_the_flag(tmp_path):
    """A checkpoint trained with --reinit-nfeat has no quantizer: without the flag the loader says which flag scores it; with the
    flag it gets as far as the device (the table is built by the HIP GEMM)."""
    from gnnlm_amd.hgt import HGT
    from gnnlm_amd.model import GnnLmModel
    hgt = HGT(in_dim=32, hidden_dim=32, out_dim=32, n_layers=1, n_heads=2)
    sd = {"decoder.hgt_decoder." + k: v for k, v in hgt.state_dict().items()}
    sd.update(_sd("adaptive"))
    args = Namespace(decoder_embed_dim=32, decoder_attention_heads=2, graph_layer=1, adaptive_softmax_cutoff="8,16", adaptive_input_cutoff="8,16")
    path = str(tmp_path / "m.pt")
    torch.save({"args": args, "model": sd}, path)
    with pytest.raises(ValueError, match="no quantizer.*--reinit-nfeat"):
        GnnLmModel.from_checkpoint(path, "cpu")
    with pytest.raises(_lib.GnnlmError, match="device"):
        GnnLmModel.from_checkpoint(path, "cpu", reinit_nfeat=True)


def test_table_precision_is_tied_to_the_model():
    """The adaptive table is built once, under one GEMM precision: a model whose precision differs from it refuses to make a store
    instead of silently mixing the two; a plain table is a copy under every precision."""
    from gnnlm_amd.hgt import HGT, TokenStore
    from gnnlm_amd.model import GnnLmModel
    from gnnlm_amd.token_embed import TokenEmbedding
    vals = torch.zeros(50, dtype=torch.int32)
    hgt = HGT(in_dim=32, hidden_dim=32, out_dim=32, n_layers=1, n_heads=2)
    model = GnnLmModel(hgt, None, token_embed=TokenEmbedding(torch.zeros(24, 32), "adaptive", 3))
    assert model.precision == "f32"
    with pytest.raises(ValueError, match="built under precision 'fp16'"):
        model.make_store(None, 50, "cpu", vals=vals)
    model.precision = "fp16"
    st = model.make_store(None, 50, "cpu", vals=vals)
    assert isinstance(st, TokenStore) and st.embed is model.token_embed.table and st.n_store == 50
    plain = GnnLmModel(hgt, None, precision="fp16", token_embed=TokenEmbedding(torch.zeros(24, 32), "plain"))
    assert plain.token_embed.precision is None and isinstance(plain.make_store(None, 50, "cpu", vals=vals), TokenStore)
    with pytest.raises(ValueError, match="nothing to shard"):
        plain.make_store(None, 50, "cpu", vals=vals, row0=5)
