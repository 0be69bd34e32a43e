"""Generation controls on the CPU: ``GenerationControls``' validation, the Python definition
(models/gpt2.py banned_tokens / stop_hit) against transformers' processors and hand cases, the
reference generation and engine, the oracle, and the plumbing (batcher, tutor CLI)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import controls_cases as cc
from distributed_lms_raft_llm_amd.engine.gpt2_engine import TorchGPT2Engine, controls_unsupported
from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
from distributed_lms_raft_llm_amd.models.config import (CONTROLS_MAX_STOP, CONTROLS_MAX_STOP_LEN, GenerationConfig,
                                                        GenerationControls, SamplingParams, gpt2_config)
from distributed_lms_raft_llm_amd.models.gpt2 import (GPT2Reference, banned_tokens, init_gpt2_weights,
                                                      reference_generate, stop_hit, teacher_forced_controls_check,
                                                      teacher_forced_sampling_check)


# ------------------------------------------------------------------ the object
def test_controls_validation():
    ct = GenerationControls()
    assert (ct.no_repeat_ngram_size, ct.min_new_tokens, ct.stop) == (0, 0, ()) and not ct.bans
    assert CONTROLS_MAX_STOP >= 4 and CONTROLS_MAX_STOP_LEN >= 8
    ct = GenerationControls(3, 5, [[1, 2], (7,)])  # lists are taken as tuples: the object stays hashable
    assert ct.stop == ((1, 2), (7,)) and ct.bans and hash(ct) == hash(GenerationControls(3, 5, ((1, 2), (7,))))
    assert GenerationControls(stop=((1,),)).bans is False and GenerationControls(min_new_tokens=1).bans
    assert GenerationControls(1000).no_repeat_ngram_size == 1000  # any n >= 1
    assert ct.shape_key != GenerationControls(3, 5, ((1, 2), (8,))).shape_key
    with pytest.raises(Exception):
        ct.min_new_tokens = 3  # frozen
    full = tuple(tuple(range(CONTROLS_MAX_STOP_LEN)) for _ in range(CONTROLS_MAX_STOP))
    assert GenerationControls(stop=full).stop == full
    for bad in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
                dict(no_repeat_ngram_size="2"), dict(min_new_tokens=-1), dict(min_new_tokens=1.5),
                dict(min_new_tokens=None), dict(stop=((),)), dict(stop=(1, 2)), dict(stop="ab"), dict(stop=("ab",)),
                dict(stop=((1, -2),)), dict(stop=((1, 2.0),)), dict(stop=((True,),)), dict(stop=None),
                dict(stop=full + ((1,),)), dict(stop=(tuple(range(CONTROLS_MAX_STOP_LEN + 1)),))):
        with pytest.raises(ValueError):
            GenerationControls(**bad)
    assert GenerationConfig().controls() is None
    assert GenerationConfig(no_repeat_ngram_size=2, stop=((5, 6),)).controls() == GenerationControls(2, 0, ((5, 6),))
    assert controls_unsupported(1, False) is None
    assert "tensor parallelism" in controls_unsupported(2, False) and "fp8" in controls_unsupported(1, True)


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_banned_tokens_is_hfs_processors(n):
    transformers = pytest.importorskip("transformers")
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)

    vocab, eos = 50, 49
    assert transformers is not None
    for seq, P, mn in cc.planted_sequences(n, vocab, seed=n):
        ct = GenerationControls(n, mn)
        scores = torch.zeros(1, vocab)
        ids = torch.tensor([seq], dtype=torch.long)
        scores = NoRepeatNGramLogitsProcessor(n)(ids, scores)
        if mn > 0:
            scores = MinNewTokensLengthLogitsProcessor(P, mn, eos, device="cpu")(ids, scores)
        want = torch.nonzero(torch.isinf(scores[0])).flatten().tolist()
        assert banned_tokens(seq, P, ct, eos) == want, (seq, P, mn)


def test_banned_tokens_hand_cases():
    ct = GenerationControls
    assert banned_tokens([1, 2, 3, 1, 2], 2, ct(3), 0) == [3]
    assert banned_tokens([1, 2, 3, 1, 2], 2, ct(2), 0) == [3] and banned_tokens([7, 7], 1, ct(2), 0) == [7]
    assert banned_tokens([4, 2, 4], 1, ct(1), 0) == [2, 4] and banned_tokens([], 0, ct(1), 0) == []
    assert banned_tokens([5], 1, ct(3), 0) == [] and banned_tokens([5, 6], 1, ct(3), 0) == []  # L + 1 < n, = n
    assert banned_tokens([5, 6, 5, 6], 1, ct(5), 0) == []
    assert banned_tokens([5, 6], 2, ct(0, 2), 9) == [9] and banned_tokens([5, 6, 1], 2, ct(0, 2), 9) == [9]
    assert banned_tokens([5, 6, 1, 1], 2, ct(0, 2), 9) == []
    assert banned_tokens([5, 6], 2, ct(0, 0, ((5, 6),)), 9) == []


def test_stop_hit_hand_cases():
    assert stop_hit([1, 2, 3, 4], 2, ((3, 4),))  # starts exactly at P
    assert not stop_hit([1, 2, 3, 4], 3, ((3, 4),))  # straddles the prompt boundary
    assert not stop_hit([1, 2, 3, 4], 4, ((4,),))  # lies in the prompt
    assert not stop_hit([1, 2, 3], 2, ((1, 2, 3),))  # longer than the generated part
    assert not stop_hit([1, 2, 3, 4, 5], 2, ((3, 4),))  # not at the end any more
    assert stop_hit([9, 3, 4], 1, ((8, 3, 4), (3, 4)))  # one stop a suffix of the other: the short one hits
    assert stop_hit([9, 8, 3, 4], 1, ((8, 3, 4), (3, 4))) and stop_hit([9, 8, 3, 4], 2, ((8, 3, 4), (3, 4)))
    assert not stop_hit([9, 8, 3, 4], 3, ((8, 3, 4), (3, 4))) and not stop_hit([1, 2], 1, ())
    assert stop_hit([1, 7], 1, ((7,),)) and not stop_hit([7], 1, ((7,),))


# ------------------------------------------------------------------ reference generation, engine, oracle
def _tiny():
    """test_sampling_cpu.py's 2-layer model with logits spread over a few units."""
    cfg = gpt2_config("gpt2-tiny")
    w = init_gpt2_weights(cfg, seed=0)
    w["transformer.wte.weight"] = w["transformer.wte.weight"] * 20.0
    for k in w:
        if k.endswith("c_proj.weight"):
            w[k] = w[k] * 200.0
    return cfg, w


PROMPTS = [[1, 2, 3, 1, 2], [7, 8], [5]]


@pytest.fixture(scope="module")
def tiny():
    cfg, w = _tiny()
    ref = GPT2Reference(cfg, w)
    plain = reference_generate(ref, PROMPTS, max_length=24, repetition_penalty=1.2)
    return cfg, w, ref, plain


@pytest.mark.parametrize("n", [1, 2, 3])
def test_reference_generate_never_repeats_an_ngram(tiny, n):
    cfg, w, ref, plain = tiny
    ct = GenerationControls(no_repeat_ngram_size=n)
    out = reference_generate(ref, PROMPTS, max_length=24, repetition_penalty=1.2, controls=ct)
    for o, p in zip(out, PROMPTS):
        assert o[: len(p)] == p and len(o) > len(p)
        assert cc.repeated_ngrams(o, len(p), n) == [], (n, o)
        r = teacher_forced_controls_check(ref, o, len(p), 1.2, ct)
        assert r["positions"] == len(o) - len(p) and not r["mismatches"], r
    assert out == TorchGPT2Engine(cfg, w, max_length=24).generate(PROMPTS, repetition_penalty=1.2, controls=ct)
    # the oracle notices a banned token: repeat an earlier generated token where n = 1 forbids it
    if n == 1:
        o, p = out[0], PROMPTS[0]
        bad = o[:-1] + [o[len(p)]]
        assert any(i == len(o) - 1 for i, *_ in teacher_forced_controls_check(ref, bad, len(p), 1.2, ct)["mismatches"])
    # and without controls the reference is what it was
    assert reference_generate(ref, PROMPTS, max_length=24, repetition_penalty=1.2) == plain


def test_reference_generate_stops_and_keeps_generating(tiny):
    cfg, w, ref, plain = tiny
    row = plain[0]
    P = len(PROMPTS[0])
    stop = (tuple(row[P + 3: P + 5]),)
    ct = GenerationControls(stop=stop)
    out = reference_generate(ref, PROMPTS, max_length=24, repetition_penalty=1.2, controls=ct)
    for o, p, full in zip(out, PROMPTS, plain):
        assert o == cc.cut_at_stop(full, len(p), stop), (o, full)
        assert not teacher_forced_controls_check(ref, o, len(p), 1.2, ct)["mismatches"]
    assert len(out[0]) == P + 5 < len(plain[0])
    assert out == TorchGPT2Engine(cfg, w, max_length=24).generate(PROMPTS, repetition_penalty=1.2, controls=ct)
    # minimum length: the model whose EOS is the third generated token of row 0
    import dataclasses

    cfg2 = dataclasses.replace(cfg, eos_token_id=row[P + 2])
    ref2 = GPT2Reference(cfg2, w)
    short = reference_generate(ref2, PROMPTS[:1], max_length=24, repetition_penalty=1.2)[0]
    assert short == row[: P + 3]
    ct = GenerationControls(min_new_tokens=6)
    longer = reference_generate(ref2, PROMPTS[:1], max_length=24, repetition_penalty=1.2, controls=ct)[0]
    assert len(longer) >= P + 6 and cfg2.eos_token_id not in longer[P: P + 6] and longer[: P + 2] == row[: P + 2]
    assert not teacher_forced_controls_check(ref2, longer, P, 1.2, ct)["mismatches"]


def test_sampled_reference_with_bans(tiny):
    cfg, w, ref, _ = tiny
    sp, ct = SamplingParams(0.7, 50, 0.9, 3), GenerationControls(no_repeat_ngram_size=2)
    out = TorchGPT2Engine(cfg, w, max_length=24).generate(PROMPTS, repetition_penalty=1.2, sampling=sp, controls=ct)
    assert out == reference_generate(ref, PROMPTS, max_length=24, repetition_penalty=1.2, sampling=sp, controls=ct)
    for o, p in zip(out, PROMPTS):
        assert cc.repeated_ngrams(o, len(p), 2) == []
        assert not teacher_forced_sampling_check(ref, o, len(p), 1.2, sp, controls=ct)["mismatches"]
    # a repeated bigram is "below top-k" for the sampled oracle
    o, p = out[0], PROMPTS[0]
    bad = o[: len(p) + 2] + [o[len(p)], o[len(p) + 1]]
    assert any(i == len(bad) - 1 for i, *_ in
               teacher_forced_sampling_check(ref, bad, len(p), 1.2, sp, controls=ct)["mismatches"])


def test_recorded_shares_cover_the_gpu_cases():
    """tests/controls_cases.py records the reference-alone decisive share of every engine case; none
    may be under 0.6 (the GPU test's floor is 0.5)."""
    for (rows, T), ns in cc.ENGINE_CASES.items():
        for n in ns:
            d, p = cc.REFERENCE_DECISIVE[(rows, T, n)]
            assert p > 0 and d / p >= 0.6, (rows, T, n, d, p)
    assert cc.MIN_DECISIVE == 0.5


# ------------------------------------------------------------------ plumbing
class _RecordingEngine:
    """A slot engine that finishes every request after its first decode chunk and records the keywords
    its admit / decode were called with (tests/test_sampling_cpu.py's fake, with ``**kw``)."""

    def __init__(self):
        self.max_batch, self.max_length = 2, 8
        self.cfg = SimpleNamespace(eos_token_id=0)
        self.calls = []
        self.seqs = {}
        self.fin = [1, 1]

    def admit(self, prompts, slots, penalty, **kw):
        self.calls.append(("admit", kw))
        for p, s in zip(prompts, slots):
            self.seqs[s], self.fin[s] = list(p) + [5], 0

    def decode(self, B, steps, penalty, **kw):
        self.calls.append(("decode", kw))
        for s in range(B):
            self.fin[s] = 1

    def finished_flags(self, B):
        return self.fin[:B]

    def collect(self, slots):
        return [self.seqs[s] for s in slots]


def test_batcher_forwards_controls_only_when_set():
    ct, sp = GenerationControls(2, 0, ((5,),)), SamplingParams(0.7, 50, 0.9, 4)
    for kw, want in ((dict(controls=ct), {"controls": ct}), (dict(controls=ct, sampling=sp), {"controls": ct,
                                                                                           "sampling": sp}),
                     ({}, {})):
        eng = _RecordingEngine()
        cb = ContinuousBatcher(eng, 1.2, **kw)
        try:
            assert cb.submit([1, 2]).result(10) == [1, 2, 5]  # (results keep their stop tokens)
        finally:
            cb.stop()
        assert {c for c, _ in eng.calls} == {"admit", "decode"}
        assert all(set(k) == set(want) and all(k[x] is want[x] for x in want) for _, k in eng.calls)


def test_tutor_cli_builds_the_controls():
    from distributed_lms_raft_llm_amd.tokenizer import GPT2BPE
    from distributed_lms_raft_llm_amd.tutor.server import (arg_parser, controls_from_args, decode_escapes,
                                                           generation_config, trim_stop)

    tok = GPT2BPE(None, None, eos_token_id=50256)
    assert controls_from_args(arg_parser().parse_args([]), tok) is None
    a = arg_parser().parse_args(["--no-repeat-ngram-size", "3", "--min-new-tokens", "4"])
    assert controls_from_args(a) == GenerationControls(3, 4)
    a = arg_parser().parse_args(["--stop", "\\nQuestion:", "--stop", "END"])
    ct = controls_from_args(a, tok)
    assert ct.stop == (tuple(tok.encode("\nQuestion:")), tuple(tok.encode("END"))) and not ct.bans
    assert tok.decode(list(ct.stop[0])) == "\nQuestion:" and decode_escapes("a\\tbé") == "a\tbé"
    for bad in (["--no-repeat-ngram-size", "-1"], ["--stop", ""], ["--stop", "a", "--stop", "b", "--stop", "c",
                                                                   "--stop", "d", "--stop", "e"]):
        with pytest.raises(ValueError):
            controls_from_args(arg_parser().parse_args(bad), tok)
    assert generation_config(150, 1.2, None, ct).controls() == ct and generation_config(150, 1.2).controls() is None
    assert "will not match" in " ".join(arg_parser().format_help().split())
    # what the servers drop before detokenising: the matched stop sequence, the longest one
    assert trim_stop([1, 2, 8, 3, 4], 2, ((3, 4), (8, 3, 4))) == ([1, 2], True)
    assert trim_stop([1, 2, 8, 3, 4], 3, ((3, 4), (8, 3, 4))) == ([1, 2, 8], True)
    assert trim_stop([1, 2, 8, 3, 4], 4, ((3, 4), (8, 3, 4))) == ([1, 2, 8, 3, 4], False)


def test_server_trims_the_stop_and_counts_it():
    from concurrent.futures import Future

    from distributed_lms_raft_llm_amd.tutor.server import StopTrimmer, front_batcher

    class _B:
        active = 3

        def submit(self, ids):
            f = Future()
            f.set_result(list(ids) + ([9, 3, 4] if ids[0] == 1 else [9, 9]))
            return f

    b = _B()
    assert front_batcher(b, None) is b and front_batcher(b, GenerationControls(2)) is b
    t = front_batcher(b, GenerationControls(stop=((3, 4),)))
    assert isinstance(t, StopTrimmer) and t.active == 3
    assert t.submit([1, 2]).result(1) == [1, 2, 9] and t.submit([2, 3, 4]).result(1) == [2, 3, 4, 9, 9]
    assert t.stopped_by_sequence == 1


def test_tutor_cli_refuses_controls_on_tp_or_fp8(capsys):
    from distributed_lms_raft_llm_amd.tutor.server import main

    for flags in (["--no-repeat-ngram-size", "2"], ["--min-new-tokens", "3"], ["--stop", "x"]):
        for extra, why in ((["--tp", "2"], controls_unsupported(2, False)),
                           (["--weight-dtype", "fp8"], controls_unsupported(1, True))):
            with pytest.raises(SystemExit) as e:
                main(flags + extra)
            assert e.value.code == 2 and why in " ".join(capsys.readouterr().err.split())
    with pytest.raises(SystemExit) as e:  # a bad value exits the same way, before any engine is built
        main(["--no-repeat-ngram-size", "-2"])
    assert e.value.code == 2
