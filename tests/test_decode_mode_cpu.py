"""The generation mode of an engine call (engine/mode.py DecodeMode): every rule it owns over the
16 modes sampling x controls x logprobs, written out as literal tables, and the five
``*_unsupported`` reasons, string for string."""
import dataclasses
import itertools

import pytest

from distributed_lms_raft_llm_amd.engine import gpt2_engine, mode as engine_mode
from distributed_lms_raft_llm_amd.engine.mode import GREEDY_AS_SAMPLING, DecodeMode
from distributed_lms_raft_llm_amd.models.config import GenerationControls, SamplingParams

SP = SamplingParams(0.7, 50, 0.9, 7)
CONTROLS = {"none": None, "bans": GenerationControls(2, 0, ()), "stop": GenerationControls(0, 0, ((1, 2),)),
            "both": GenerationControls(2, 3, ((1, 2), (7,)))}
GREEDY = SamplingParams(1.0, 1, 1.0, 0)

# (sampling set, controls, logprobs) -> the sampler: "sp" the call's own, "greedy" the top_k = 1
# constant, None the fused-argmax heads
SAMPLER = {
    (False, "none", False): None, (False, "none", True): "greedy",
    (False, "bans", False): "greedy", (False, "bans", True): "greedy",
    (False, "stop", False): None, (False, "stop", True): "greedy",
    (False, "both", False): "greedy", (False, "both", True): "greedy",
    (True, "none", False): "sp", (True, "none", True): "sp",
    (True, "bans", False): "sp", (True, "bans", True): "sp",
    (True, "stop", False): "sp", (True, "stop", True): "sp",
    (True, "both", False): "sp", (True, "both", True): "sp",
}
RECORDS_PROMPT_LEN = {(c, lp): c != "none" or lp for c in CONTROLS for lp in (False, True)}
CTL_KEY = {"none": (), "bans": ("ctl", 2, 0, ()), "stop": ("ctl", 0, 0, ((1, 2),)),
           "both": ("ctl", 2, 3, ((1, 2), (7,)))}

# the parent's five functions, (tp_size > 1, fp8 weights) sentences
UNSUPPORTED = {
    "sampling_unsupported": (
        "sampling is not supported with tensor parallelism (tp_size > 1): the device sampler ranks one "
        "rank's whole vocabulary; serve greedy or TP=1",
        "sampling is not supported with fp8 weights: the fp8 LM head has no f32-logits epilogue; serve "
        "greedy or weight_dtype='bf16'"),
    "kv_fp8_unsupported": (
        "the fp8 KV cache is not supported with tensor parallelism (tp_size > 1): the TP-fused decode path "
        "has no fp8-cache build; serve kv_dtype='bf16' or TP=1",
        "the fp8 KV cache is not supported with fp8 weights: the W8A8 QKV GEMM has no fp8-cache epilogue; "
        "serve kv_dtype='bf16' or weight_dtype='bf16'"),
    "prefix_unsupported": (
        "the prompt-prefix cache is not supported with tensor parallelism (tp_size > 1): the prefix store "
        "and its fill are built for one rank's whole cache; serve prefix_capacity=0 or TP=1",
        "the prompt-prefix cache is not supported with fp8 weights: the suffix-only prefill is verified on "
        "the bf16 GEMMs only; serve prefix_capacity=0 or weight_dtype='bf16'"),
    "controls_unsupported": (
        "generation controls are not supported with tensor parallelism (tp_size > 1): the device bans "
        "work on one rank's whole vocabulary; serve without controls or TP=1",
        "generation controls are not supported with fp8 weights: the fp8 LM head has no f32-logits "
        "epilogue for the bans; serve without controls or weight_dtype='bf16'"),
    "logprobs_unsupported": (
        "log-probabilities are not supported with tensor parallelism (tp_size > 1): the device log-softmax "
        "reduces one rank's whole vocabulary; serve without logprobs or TP=1",
        "log-probabilities are not supported with fp8 weights: the fp8 LM head has no f32-logits epilogue "
        "to take them from; serve without logprobs or weight_dtype='bf16'"),
}


def _modes():
    for s, c, lp in itertools.product((False, True), CONTROLS, (False, True)):
        yield (s, c, lp), DecodeMode(SP if s else None, CONTROLS[c], lp)


def test_the_matrix_is_the_16_modes():
    assert len(SAMPLER) == 16 == len(dict(_modes())) and set(SAMPLER) == set(dict(_modes()))
    assert DecodeMode() == DecodeMode(None, None, False) and hash(DecodeMode()) == hash(DecodeMode(None, None, False))
    with pytest.raises(dataclasses.FrozenInstanceError):
        DecodeMode().logprobs = True


def test_sampler_bans_and_stop():
    assert GREEDY_AS_SAMPLING == GREEDY
    for (s, c, lp), m in _modes():
        want = {"sp": SP, "greedy": GREEDY, None: None}[SAMPLER[s, c, lp]]
        assert m.sampler == want, (s, c, lp)
        assert (m.sampler is SP) == s
        assert bool(m.bans) == (c in ("bans", "both")) and (not m.bans or m.bans is CONTROLS[c]), (s, c, lp)
        assert m.stop == {"none": (), "bans": (), "stop": ((1, 2),), "both": ((1, 2), (7,))}[c], (s, c, lp)
        assert not m.bans or m.sampler is not None  # (the bans need the f32 logits)


def test_records_prompt_len_and_dataflow_ok():
    for (s, c, lp), m in _modes():
        assert m.records_prompt_len is RECORDS_PROMPT_LEN[c, lp], (s, c, lp)
        assert m.dataflow_ok is ((s, c, lp) == (False, "none", False)), (s, c, lp)
    assert DecodeMode().dataflow_ok and not DecodeMode().records_prompt_len and DecodeMode().sampler is None


def test_graph_keys():
    assert DecodeMode().graph_key == ()
    assert DecodeMode(sampling=SP).graph_key == (0.7, 50, 0.9)
    assert DecodeMode(controls=CONTROLS["bans"]).graph_key == ("ctl", 2, 0, ())
    assert DecodeMode(controls=CONTROLS["stop"]).graph_key == ("ctl", 0, 0, ((1, 2),))
    assert DecodeMode(logprobs=True).graph_key == ("logprobs",)
    assert DecodeMode(SP, CONTROLS["both"], True).graph_key == (0.7, 50, 0.9, "ctl", 2, 3, ((1, 2), (7,)), "logprobs")
    keys = {}
    for (s, c, lp), m in _modes():
        # the sampling's key, then the controls', then the log-probabilities' word
        assert m.graph_key == ((0.7, 50, 0.9) if s else ()) + CTL_KEY[c] + (("logprobs",) if lp else ()), (s, c, lp)
        keys[m.graph_key] = (s, c, lp)
    assert len(keys) == 16, "two modes share a graph key"
    for c, lp in itertools.product(CONTROLS, (False, True)):  # the seed is a device word
        a, b = (DecodeMode(SamplingParams(0.7, 50, 0.9, seed), CONTROLS[c], lp) for seed in (7, 8))
        assert a != b and a.graph_key == b.graph_key


def test_check_types_and_shapes():
    for _, m in _modes():
        m.check(1, False)
    with pytest.raises(TypeError, match="sampling: a SamplingParams"):
        DecodeMode(sampling=(0.7, 50, 0.9)).check(1, False)
    with pytest.raises(TypeError, match="controls: a GenerationControls"):
        DecodeMode(controls={"stop": ()}).check(1, False)
    for tp, fp8, i in ((2, False, 0), (8, False, 0), (1, True, 1), (2, True, 0)):
        for m, name in ((DecodeMode(sampling=SP), "sampling_unsupported"),
                        (DecodeMode(controls=CONTROLS["stop"]), "controls_unsupported"),
                        (DecodeMode(logprobs=True), "logprobs_unsupported")):
            with pytest.raises(ValueError) as e:
                m.check(tp, fp8)
            assert str(e.value) == UNSUPPORTED[name][i]
        DecodeMode().check(tp, fp8)  # greedy is served by every shape


def test_check_reports_logprobs_then_controls_then_sampling():
    ct = CONTROLS["both"]
    for tp, fp8, i in ((2, False, 0), (1, True, 1)):
        for m, name in ((DecodeMode(SP, ct, True), "logprobs_unsupported"),
                        (DecodeMode(SP, None, True), "logprobs_unsupported"),
                        (DecodeMode(SP, ct, False), "controls_unsupported"),
                        (DecodeMode((0.7, 50, 0.9), "no controls", True), "logprobs_unsupported"),
                        (DecodeMode((0.7, 50, 0.9), ct, False), "controls_unsupported")):
            with pytest.raises(ValueError) as e:
                m.check(tp, fp8)
            assert str(e.value) == UNSUPPORTED[name][i], (tp, fp8, m)
        with pytest.raises(TypeError, match="controls"):  # the controls' type ahead of the sampling's
            DecodeMode((0.7, 50, 0.9), "no controls", False).check(tp, fp8)
    with pytest.raises(TypeError, match="controls"):
        DecodeMode((0.7, 50, 0.9), "no controls", True).check(1, False)


def test_unsupported_strings_are_the_parents():
    assert set(UNSUPPORTED) == {n for n in vars(engine_mode) if n.endswith("_unsupported") and not n.startswith("_")}
    for name, (tp_text, fp8_text) in UNSUPPORTED.items():
        f = getattr(engine_mode, name)
        assert getattr(gpt2_engine, name) is f and f.__name__ == name  # (importable from the engine as before)
        assert f(1, False) is None
        for tp in (2, 8):
            assert f(tp, False) == tp_text and f(tp, True) == tp_text
        assert f(1, True) == fp8_text
