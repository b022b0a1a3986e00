"""The command lines of ``gnnlm_amd.generate`` and ``gnnlm_amd.beam_search`` without a GPU: the flag set with its defaults, against a
table recorded from the two parsers as they were while each driver declared every flag itself, and the refusal matrices of the two
``test_command_line_refusals`` (test_generate_gpu.py, test_beam_search_gpu.py) through ``check_args`` alone -- the same exception
types, the same words.  (``--beam 25`` is refused against the model's vocabulary, by ``BeamGenerator.check_beam``: that one is
asked directly, with the V = 50 of those tests' model.)"""
import pytest

from gnnlm_amd import beam_search, generate

COMMON = {
    "data": "D", "path": "p", "model_overrides": "{}", "device": "cuda:0", "gen_subset": "test", "n_prompts": 8, "prompt_len": 32,
    "prompt_ids": None, "max_len_b": 64, "min_len": 1, "sampling": False, "sampling_topk": -1, "sampling_topp": -1.0, "temperature": 1.0,
    "knn_temperature": 1.0, "unkpen": 0.0, "fp16": False, "no_repeat_ngram_size": 0, "graph": False, "sweep_lmbda": None,
    "sweep_temperature": None, "sweep_k": None, "knnlm": False, "k": 1024, "lmbda": 0.25, "probe": 32, "dstore_dir": None, "index_file": None,
    "knn_sim_func": "do_not_recomp_ip", "knn_keytype": None, "out": None,
}
DEFAULTS = {
    generate: dict(COMMON, beam=1, seed=1),
    beam_search: dict(COMMON, beam=5, nbest=1, lenpen=1.0, unnormalized=False, score_prompt=False),
}

GENERATE_REFUSALS = [
    (["--beam", "2"], ValueError, "--beam"),
    (["--sampling", "--sampling-topk", "5", "--sampling-topp", "0.9"], ValueError, "--sampling-topp"),
    (["--sampling"], ValueError, "--sampling-topk"),
    (["--sampling", "--sampling-topk", "2049"], ValueError, "--sampling-topk"),
    (["--no-repeat-ngram-size", "3"], ValueError, "--no-repeat-ngram-size"),
    (["--min-len", "2"], ValueError, "--min-len"),
    (["--graph"], ValueError, "--graph"),
    (["--sweep-lmbda", "0.1,0.2"], ValueError, "--sweep-lmbda"),
    (["--sweep-temperature", "1,2"], ValueError, "--sweep-temperature"),
    (["--sweep-k", "8,16"], ValueError, "--sweep-k"),
    (["--knnlm"], ValueError, "--knnlm"),
    (["--knnlm", "--lmbda", "0", "--dstore-dir", "D", "--index-file", "F"], ValueError, "--lmbda"),
]
BEAM_REFUSALS = [
    (["--sampling"], ValueError, "--sampling"),
    (["--sampling-topk", "5"], ValueError, "--sampling"),
    (["--sampling-topp", "0.9"], ValueError, "--sampling-topp"),
    (["--no-repeat-ngram-size", "3"], ValueError, "--no-repeat-ngram-size"),
    (["--graph"], ValueError, "--graph"),
    (["--sweep-lmbda", "0.1,0.2"], ValueError, "--sweep-lmbda"),
    (["--sweep-temperature", "1,2"], ValueError, "--sweep-temperature"),
    (["--sweep-k", "8,16"], ValueError, "--sweep-k"),
    (["--beam", "33"], ValueError, "--beam"),
    (["--beam", "2", "--nbest", "3"], ValueError, "--nbest"),
    (["--score-prompt", "--knnlm", "--dstore-dir", "D", "--index-file", "F"], ValueError, "--score-prompt"),
    (["--knnlm"], ValueError, "--knnlm"),
]


def parse(driver, flags):
    return driver.get_parser().parse_args(["D", "--path", "p", "--max-len-b", "4"] + flags)


@pytest.mark.parametrize("driver", [generate, beam_search], ids=["generate", "beam_search"])
def test_flags_and_defaults_are_the_recorded_ones(driver):
    got = vars(driver.get_parser().parse_args(["D", "--path", "p"]))
    assert got == DEFAULTS[driver], {k: (got.get(k), DEFAULTS[driver].get(k)) for k in set(got) | set(DEFAULTS[driver])
                                     if got.get(k, KeyError) != DEFAULTS[driver].get(k, KeyError)}
    driver.check_args(parse(driver, []))                                          # the defaults themselves are accepted


@pytest.mark.parametrize("driver,flags,exc,word", [(generate, *r) for r in GENERATE_REFUSALS] + [(beam_search, *r) for r in BEAM_REFUSALS],
                         ids=lambda v: v.__name__.split(".")[-1] if hasattr(v, "__name__") else (" ".join(v) if isinstance(v, list) else None))
def test_check_args_refuses(driver, flags, exc, word):
    with pytest.raises(exc, match=word):
        driver.check_args(parse(driver, flags))


def test_more_than_one_process_and_a_beam_wider_than_the_vocabulary(monkeypatch):
    beam_search.check_args(parse(beam_search, ["--beam", "25"]))                  # the flags alone are fine: V decides
    with pytest.raises(ValueError, match="--beam"):
        beam_search.BeamGenerator.check_beam(4, 25, 1, 1.0, 50)                   # 2 * beam > V - 1 = 49
    beam_search.BeamGenerator.check_beam(4, 24, 1, 1.0, 50)
    monkeypatch.setenv("WORLD_SIZE", "2")
    for driver in (generate, beam_search):
        with pytest.raises(NotImplementedError, match="one process"):
            driver.check_args(parse(driver, []))
