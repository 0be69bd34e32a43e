"""Log-probabilities on the CPU: the Python definition (models/gpt2.py reference_logprob), the
reference engine's ``generate(logprobs=True)`` and ``score()``, the plumbing (batcher, StopTrimmer,
GenerationConfig, tutor CLI) and the recorded noise figures the GPU tolerances are built from."""
import math
import time
from concurrent.futures import Future

import numpy as np
import pytest
import torch

import logprob_cases as lc
from distributed_lms_raft_llm_amd.engine.gpt2_engine import TorchGPT2Engine, logprobs_unsupported
from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
from distributed_lms_raft_llm_amd.models.config import GenerationConfig, GenerationControls, SamplingParams, gpt2_config
from distributed_lms_raft_llm_amd.models.gpt2 import (GPT2Reference, KVCache, init_gpt2_weights, logprob_noise,
                                                      penalised_logits_f32, reference_logprob,
                                                      teacher_forced_logprobs)


def _logsumexp(x):
    m = x[np.isfinite(x)].max()
    return m + math.log(np.exp(x - m).sum())


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize("penalty", [1.0, 1.2])
def test_reference_logprob_is_a_normalised_distribution(penalty):
    g = np.random.default_rng(0)
    z = (g.standard_normal(1000) * 2).astype(np.float32)
    seen = g.random(1000) < 0.5
    lp = reference_logprob(z, seen, penalty)
    assert lp.dtype == np.float64 and lp.shape == (1000,)
    assert abs(_logsumexp(lp)) < 1e-12
    for tok in (0, 17, 999):
        assert reference_logprob(z, seen, penalty, tok) == lp[tok]
    # it is the log-softmax of the float32 penalised logits
    want = torch.log_softmax(torch.from_numpy(penalised_logits_f32(z, seen, penalty)).double(), dim=-1).numpy()
    assert np.abs(lp - want).max() < 1e-12


def test_reference_logprob_penalises_seen_columns_only_with_the_sign_rule():
    z = np.array([2.0, -2.0, 2.0, -2.0, 0.5], dtype=np.float32)
    seen = np.array([True, True, False, False, False])
    th = np.float32(1.2)
    l = np.array([np.float32(2.0) / th, np.float32(-2.0) * th, 2.0, -2.0, 0.5], dtype=np.float64)
    want = l - (l.max() + math.log(np.exp(l - l.max()).sum()))
    got = reference_logprob(z, seen, 1.2)
    assert np.abs(got - want).max() < 1e-12
    assert got[0] < got[2] and got[1] < got[3]  # a seen column loses on either side of zero
    assert np.array_equal(reference_logprob(z, None, 1.2), reference_logprob(z, np.zeros(5, dtype=bool), 1.2))
    assert np.array_equal(reference_logprob(z, seen, 1.0), reference_logprob(z, None, 1.0))


def test_reference_logprob_ignores_banned_columns_and_a_shift():
    g = np.random.default_rng(1)
    z = (g.standard_normal(500) * 2).astype(np.float32)
    seen = g.random(500) < 0.5
    banned = g.choice(500, 100, replace=False)
    keep = np.setdiff1d(np.arange(500), banned)
    zb = z.copy()
    zb[banned] = -np.inf
    lp = reference_logprob(zb, seen, 1.2)
    assert np.all(np.isneginf(lp[banned])) and abs(_logsumexp(lp[keep])) < 1e-12
    # the -inf columns contribute nothing: the others are the distribution of the row without them
    assert np.abs(lp[keep] - reference_logprob(z[keep], seen[keep], 1.2)).max() < 1e-12
    # a row shifted by +80 (exactly representable steps: multiples of 2^-10 below 128)
    zq = (np.round(z * 1024) / 1024).astype(np.float32)
    assert np.array_equal((zq + np.float32(80.0)) - np.float32(80.0), zq)
    assert np.abs(reference_logprob(zq + np.float32(80.0), None, 1.0) - reference_logprob(zq, None, 1.0)).max() < 1e-12


# ------------------------------------------------------------------ the reference engine
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
    return cfg, w, TorchGPT2Engine(cfg, w, max_length=24)


@pytest.mark.parametrize("mode", ["greedy", "sampling", "controls"])
def test_torch_engine_logprobs_are_teacher_forced_logprobs(tiny, mode):
    cfg, w, eng = tiny
    kw = {"greedy": {}, "sampling": dict(sampling=SamplingParams(0.7, 50, 0.9, 5)),
          "controls": dict(controls=GenerationControls(no_repeat_ngram_size=2, min_new_tokens=3))}[mode]
    prompts = PROMPTS + [list(range(30)), []]  # (a pass-through prompt and an empty one)
    plain = eng.generate(prompts, repetition_penalty=1.2, **kw)
    toks, lps = eng.generate(prompts, repetition_penalty=1.2, logprobs=True, **kw)
    assert toks == plain
    assert lps[3] == [] and len(lps) == len(prompts)
    for o, p, lp in zip(toks, prompts, lps):
        n = max(1, len(p))
        assert len(lp) == len(o) - n and all(isinstance(v, float) and math.isfinite(v) and v <= 0 for v in lp)
        want = teacher_forced_logprobs(eng.model, o, n, 1.2, kw.get("controls"))
        assert np.array_equal(np.asarray(lp), want)
    if mode == "controls":  # the bans move probability: the same tokens score lower without them
        o, p = toks[0], prompts[0]
        free = teacher_forced_logprobs(eng.model, o, len(p), 1.2)
        assert np.all(np.asarray(lps[0]) >= free - 1e-12) and np.any(np.asarray(lps[0]) > free + 1e-9)


def test_torch_engine_score_is_a_log_softmax_gather(tiny):
    cfg, w, eng = tiny
    seqs = [[1, 2, 3, 1, 2, 9, 9], [7, 8], [5]]
    got = eng.score(seqs)
    assert got[2] == [] and [len(g) for g in got] == [6, 1, 0]
    for s, g in zip(seqs[:2], got):
        S = len(s)
        cache = KVCache.allocate(cfg, 1, S, dtype=eng.model.dtype)
        hidden = eng.model.forward(torch.tensor([s]), torch.arange(S)[None], cache, torch.zeros(1, dtype=torch.long))[0]
        lsm = torch.log_softmax(eng.model.logits(hidden).double(), dim=-1)
        want = lsm[torch.arange(S - 1), torch.tensor(s[1:])]
        assert np.abs(np.asarray(g) - want.numpy()).max() < 1e-5  # (f32 logits: the gather differs by their ulps)


# ------------------------------------------------------------------ plumbing
def test_generation_config_and_unsupported_shapes():
    assert GenerationConfig().logprobs is False and GenerationConfig(logprobs=True).logprobs is True
    assert logprobs_unsupported(1, False) is None
    assert "tensor parallelism" in logprobs_unsupported(2, False) and "fp8" in logprobs_unsupported(1, True)


def test_continuous_batcher_resolves_to_tokens_and_logprobs():
    from test_scheduler import EOS, FakeSlotEngine, _prompts, solo

    class LogprobFake(FakeSlotEngine):
        """The scheduler tests' CPU engine, recording -(position + token / 100) per generated token."""

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.plen = [1] * self.max_batch
            self.calls = []

        def admit(self, prompts, slots, penalty, logprobs=False):
            self.calls.append(("admit", logprobs))
            for p, s in zip(prompts, slots):
                self.plen[s] = len(p)
            super().admit(prompts, slots, penalty)

        def decode(self, B, steps, penalty, logprobs=False):
            self.calls.append(("decode", logprobs))
            super().decode(B, steps, penalty)

        def collect(self, slots, logprobs=False):
            self.calls.append(("collect", logprobs))
            toks = super().collect(slots)
            return toks, [[-(i + t / 100) for i, t in enumerate(o) if i >= self.plen[s]] for o, s in zip(toks, slots)]

    eng = LogprobFake(max_batch=4, max_length=40)
    cb = ContinuousBatcher(eng, chunk=3, logprobs=True)
    try:
        prompts = _prompts(11) + [list(range(45)), []]
        futs = []
        for i, p in enumerate(prompts):
            futs.append(cb.submit(p))
            if i % 4 == 0:
                time.sleep(0.003)
        outs = [f.result(10) for f in futs]
    finally:
        cb.stop()
    assert all(lp for _, lp in eng.calls) and {c for c, _ in eng.calls} == {"admit", "decode", "collect"}
    for (toks, lps), p in zip(outs, prompts):
        n = len(p) if p else 1
        assert toks == (p if len(p) >= 40 else solo(p or [EOS], 40))
        assert len(lps) == len(toks) - n
        assert lps == [-(i + t / 100) for i, t in enumerate(toks) if i >= n]
    # without the flag the engine is called as before (FakeSlotEngine takes no such keyword)
    cb = ContinuousBatcher(FakeSlotEngine(max_batch=2, max_length=20), chunk=3)
    try:
        assert cb.submit([3, 4]).result(10) == solo([3, 4], 20)
    finally:
        cb.stop()


def test_stop_trimmer_and_meter_trim_and_strip_the_logprobs():
    from distributed_lms_raft_llm_amd.tutor.server import LogprobMeter, StopTrimmer, front_batcher, logprob_stats

    class _B:
        active = 3

        def submit(self, ids):
            f = Future()
            toks = list(ids) + ([9, 3, 4] if ids[0] == 1 else [9, 9])
            f.set_result((toks, [-1.0, -2.0, -4.0][: len(toks) - len(ids)]))
            return f

    b = _B()
    t = StopTrimmer(b, ((3, 4),))
    assert t.submit([1, 2]).result(1) == ([1, 2, 9], [-1.0]) and t.stopped_by_sequence == 1
    assert t.submit([2, 3, 4]).result(1) == ([2, 3, 4, 9, 9], [-1.0, -2.0])
    # the servers' front: tokens alone come out, the means are kept
    assert front_batcher(b, None) is b
    m = front_batcher(b, GenerationControls(stop=((3, 4),)), True, -1.2)
    assert isinstance(m, LogprobMeter) and m.active == 3 and m.mean_token_logprob is None
    assert m.submit([1, 2]).result(1) == [1, 2, 9]  # mean -1.0
    assert m.submit([2, 3, 4]).result(1) == [2, 3, 4, 9, 9]  # mean -1.5
    assert m.mean_token_logprob == -1.25 and m.low_confidence_answers == 1 and m.stopped_by_sequence == 1
    assert logprob_stats(m) == {"mean_token_logprob": -1.25, "low_confidence_answers": 1}
    m2 = front_batcher(b, None, True)
    assert m2.submit([1, 2]).result(1) == [1, 2, 9, 3, 4]
    assert logprob_stats(m2) == {"mean_token_logprob": round(-7 / 3, 4)}


def test_window_batcher_forwards_the_flag(tiny):
    from distributed_lms_raft_llm_amd.tutor.server import Batcher, generation_config

    cfg, w, eng = tiny
    gen = generation_config(24, 1.2, None, None, True)
    assert gen.logprobs and not generation_config(24, 1.2).logprobs
    b = Batcher(eng, gen, max_batch=4, window_ms=1.0)
    try:
        toks, lps = b.submit(PROMPTS[0]).result(30)
    finally:
        b.stop()
    want_t, want_l = eng.generate(PROMPTS[:1], repetition_penalty=1.2, logprobs=True)
    assert toks == want_t[0] and lps == want_l[0]


def test_tutor_cli_refuses_logprobs_on_tp_or_fp8(capsys):
    from distributed_lms_raft_llm_amd.tutor.server import arg_parser, main

    for flags in (["--logprobs"], ["--min-mean-logprob", "-3.5"]):
        for extra, why in ((["--tp", "2"], logprobs_unsupported(2, False)),
                           (["--weight-dtype", "fp8"], logprobs_unsupported(1, True))):
            with pytest.raises(SystemExit) as e:
                main(flags + extra)
            assert e.value.code == 2 and why in " ".join(capsys.readouterr().err.split())
    args = arg_parser().parse_args(["--min-mean-logprob", "-3.5"])
    assert args.min_mean_logprob == -3.5 and args.logprobs is False
    assert arg_parser().parse_args([]).min_mean_logprob is None


# ------------------------------------------------------------------ the recorded noise
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_logprob_noise_reproduces_the_recorded_values(kv):
    cfg = gpt2_config("gpt2")
    w = lc.bf16_exact_weights(cfg)
    got = logprob_noise(cfg, w, lc.prompts(cfg, lc.NOISE_ROWS), lc.NOISE_T, lc.PEN, kv)
    print(f"logprob_noise {kv}: {got!r}")
    assert got == pytest.approx(lc.LOGPROB_NOISE[kv], rel=0.1)  # (a BLAS that blocks differently flips a few bf16 roundings)
    assert lc.LOGPROB_EPS == 4 * lc.LOGPROB_NOISE["bf16"] and lc.LOGPROB_EPS_FP8 == 4 * lc.LOGPROB_NOISE["fp8"]
