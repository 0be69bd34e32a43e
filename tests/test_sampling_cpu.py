"""Sampling without a GPU: the Philox generator, the CPU definition of the sampler
(models/gpt2.py reference_sample) against HF's warper semantics and its own exact distribution, the
reference engine, the oracle check, and the plumbing (parameters, scheduler, tutor CLI)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sampling_cases as sc
from distributed_lms_raft_llm_amd.engine.gpt2_engine import TorchGPT2Engine
from distributed_lms_raft_llm_amd.engine.memory import plan_max_batch, slot_bytes
from distributed_lms_raft_llm_amd.engine.scheduler import ContinuousBatcher
from distributed_lms_raft_llm_amd.models.config import GenerationConfig, SamplingParams, gpt2_config
from distributed_lms_raft_llm_amd.models.gpt2 import (GPT2Reference, KVCache, init_gpt2_weights, penalised_logits_f32,
                                                      philox4x32_10, reference_sample, sampling_candidates,
                                                      sampling_uniform, teacher_forced_check,
                                                      teacher_forced_sampling_check)

PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox_known_answers(counter, key, want):
    assert philox4x32_10(counter, key) == want


def test_uniform_is_24_bits_of_word_0():
    r = philox4x32_10((17, 5, 9, 0), (0xdeadbeef, 0x1234))
    assert sampling_uniform(0x1234deadbeef, (9 << 32) | 5, 17) == (r[0] >> 8) / 2 ** 24


def _row(n=1000, seed=0):
    g = np.random.default_rng(seed)
    z = (g.standard_normal(n) * 3).astype(np.float32)
    seen = g.random(n) < 0.2
    return z, seen


def test_top_k_1_is_the_penalised_argmax_with_ties_to_the_lower_id():
    z, seen = _row()
    l = penalised_logits_f32(z, seen, 1.2)
    for stream in range(5):
        tok, m, dec = reference_sample(z, seen, 1.2, SamplingParams(1.0, 1, 1.0, 3), stream, 7)
        assert (tok, m, dec) == (int(np.argmax(l)), 1, True)
    z[:] = 2.5  # all equal: the lowest id
    z[0], seen[:] = -1.0, False
    assert reference_sample(z, seen, 1.2, SamplingParams(0.7, 1, 0.9, 3), 0, 0)[0] == 1
    # a penalised duplicate of the maximum loses to the unpenalised one, whatever its id
    z[:] = 0.0
    z[10] = z[20] = 4.0
    seen[10] = True
    assert reference_sample(z, seen, 1.2, SamplingParams(0.7, 1, 0.9, 3), 0, 0)[0] == 20


def test_tiny_top_p_is_the_argmax():
    z, seen = _row(seed=1)
    l = penalised_logits_f32(z, seen, 1.2)
    for stream in range(20):
        tok, m, _ = reference_sample(z, seen, 1.2, SamplingParams(1.5, 50, 1e-6, 11), stream, 3)
        assert (tok, m) == (int(np.argmax(l)), 1)


def _hf_kept(scores: torch.Tensor, temperature: float, top_k: int, top_p: float) -> set:
    """HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper (min_tokens_to_keep=1),
    transcribed: the ids left finite."""
    s = scores / temperature
    kth = torch.topk(s, top_k)[0][-1]
    s = s.masked_fill(s < kth, -float("inf"))
    sorted_logits, sorted_idx = torch.sort(s, descending=False)
    cum = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    remove = cum <= (1 - top_p)
    remove[-1:] = False
    s = s.masked_fill(remove.scatter(0, sorted_idx, remove), -float("inf"))
    return set(torch.nonzero(torch.isfinite(s)).flatten().tolist())


@pytest.mark.parametrize("k,p,T", [(50, 0.9, 0.7), (64, 0.5, 1.0), (256, 0.9, 2.0), (10, 0.3, 1.3), (256, 1.0, 1.0)])
def test_kept_set_is_hf_warpers(k, p, T):
    z, seen = _row(seed=2)
    seen[:] = False
    _, m, dec = reference_sample(z, seen, 1.0, SamplingParams(T, k, p, 0), 0, 0)
    assert dec
    kept = set(sampling_candidates(z)[:m].tolist())
    assert kept == _hf_kept(torch.from_numpy(z).double(), T, k, p)


def test_draw_distribution_chi_square():
    """8192 draws (streams 0..8191) on one row against the exact probabilities w_i / c_{m-1}."""
    g = np.random.default_rng(5)
    z = (g.standard_normal(64) * 1.5).astype(np.float32)
    seen = np.zeros(64, dtype=bool)
    sp = SamplingParams(1.0, 8, 0.95, 20240607)
    order = sampling_candidates(z)[:8]
    w = np.exp((z[order] - z[order[0]]).astype(np.float64))
    counts = np.zeros(64)
    m = None
    for stream in range(8192):
        tok, m, _ = reference_sample(z, seen, 1.0, sp, stream, 12)
        counts[tok] += 1
    assert counts.sum() == counts[order[:m]].sum()  # nothing outside the nucleus
    expect = 8192 * w[:m] / w[:m].sum()
    chi2 = float(((counts[order[:m]] - expect) ** 2 / expect).sum())
    crit = {2: 13.82, 3: 16.27, 4: 18.47, 5: 20.52, 6: 22.46, 7: 24.32}[m - 1]  # chi-square, p = 0.001
    assert 2 <= m - 1 and chi2 < crit, (m, chi2)


def test_gpu_test_inputs_are_decisive():
    """At most 3 % of the rows of every kernel-test case may sit within 1e-9 W of a boundary."""
    for case, vocab, ld, rows, k, p, T in sc.all_cases():
        z, seen, streams, positions = sc.make_case(vocab, ld, rows, p, case)
        sp = SamplingParams(T, k, p, sc.SEED)
        dec = [reference_sample(z[r, :vocab], seen[r], sc.PENALTY, sp, int(streams[r]), int(positions[r]))[2]
               for r in range(rows)]
        assert sum(dec) >= math.ceil(0.97 * rows), (case, dec)


# ------------------------------------------------------------------ reference engine, oracle
def _tiny():
    """The 2-layer test model with logits spread over a few units (a plain random init gives +-0.05,
    which no check can tell apart): a larger tied embedding, and residual projections large enough
    that the current token's own embedding does not decide the next one."""
    cfg = gpt2_config("gpt2-tiny")
    w = init_gpt2_weights(cfg, seed=0)
    w["transformer.wte.weight"] = w["transformer.wte.weight"] * 20.0
    for k in w:
        if k.endswith("c_proj.weight"):
            w[k] = w[k] * 200.0
    return cfg, w


def test_reference_engine_sampling():
    cfg, w = _tiny()
    eng = TorchGPT2Engine(cfg, w, max_length=20)
    prompts = [[1, 2, 3], [7, 8], list(range(20))]  # (the last passes through: it keeps stream 2 unused)
    sp = SamplingParams(0.7, 50, 0.9, 1)
    a = eng.generate(prompts, repetition_penalty=1.2, sampling=sp)
    assert a == eng.generate(prompts, repetition_penalty=1.2, sampling=sp)
    assert a != eng.generate(prompts, repetition_penalty=1.2, sampling=SamplingParams(0.7, 50, 0.9, 2))
    assert a[2] == prompts[2] and all(o[: len(p)] == p for o, p in zip(a, prompts))
    greedy = eng.generate(prompts, repetition_penalty=1.2)
    assert eng.generate(prompts, repetition_penalty=1.2, sampling=SamplingParams(0.7, 1, 0.9, 5)) == greedy
    assert a != greedy
    oracle = GPT2Reference(cfg, w)
    for o, p in zip(a[:2], prompts):
        r = teacher_forced_sampling_check(oracle, o, len(p), 1.2, sp)
        assert r["positions"] == len(o) - len(p) and not r["mismatches"], r


def test_oracle_check_flags_an_unlikely_token():
    cfg, w = _tiny()
    oracle = GPT2Reference(cfg, w)
    sp = SamplingParams(0.7, 50, 0.9, 1)
    prompt = [1, 2, 3]
    seq = TorchGPT2Engine(cfg, w, max_length=16).generate([prompt], repetition_penalty=1.2, sampling=sp)[0]
    assert not teacher_forced_sampling_check(oracle, seq, len(prompt), 1.2, sp)["mismatches"]
    # the oracle's rank-1000 token at position 8
    hidden = oracle.forward(torch.tensor([seq[:8]]), torch.arange(8)[None], KVCache.allocate(cfg, 1, 8),
                            torch.zeros(1, dtype=torch.long))[0]
    rank1000 = int(torch.argsort(oracle.logits(hidden[-1]), descending=True)[999])
    bad = seq[:8] + [rank1000] + seq[9:]
    mm = teacher_forced_sampling_check(oracle, bad, len(prompt), 1.2, sp)["mismatches"]
    assert any(i == 8 and got == rank1000 for i, got, _, _ in mm), mm
    # and the greedy oracle still holds a top_k = 1 sequence
    g = TorchGPT2Engine(cfg, w, max_length=16).generate([prompt], repetition_penalty=1.2,
                                                         sampling=SamplingParams(0.7, 1, 0.9, 1))[0]
    assert not teacher_forced_check(oracle, g, len(prompt), 1.2, eps=0.05)["mismatches"]


# ------------------------------------------------------------------ plumbing
def test_sampling_params_validation():
    sp = SamplingParams()
    assert (sp.temperature, sp.top_k, sp.top_p, sp.seed) == (0.7, 50, 0.9, 0)
    assert SamplingParams(2, 256, 1, 2 ** 64 - 1).shape_key == (2.0, 256, 1.0)
    with pytest.raises(Exception):
        sp.top_k = 3  # frozen
    for bad in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
                dict(temperature=float("nan")), dict(top_k=0), dict(top_k=257), dict(top_k=2.5), dict(top_p=0.0),
                dict(top_p=1.01), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)):
        with pytest.raises(ValueError):
            SamplingParams(**bad)
    assert GenerationConfig().sampling() is None
    assert GenerationConfig(do_sample=True, top_k=40, seed=9).sampling() == SamplingParams(0.7, 40, 0.9, 9)


def test_memory_planner_counts_the_logits_row():
    cfg = gpt2_config("gpt2")
    assert slot_bytes(cfg, 150, sampling=True) - slot_bytes(cfg, 150) == cfg.vocab_padded * 4 + 8
    gib = 1 << 30
    assert plan_max_batch(cfg, 150, free_bytes=8 * gib, sampling=True) <= plan_max_batch(cfg, 150, free_bytes=8 * gib)


class _RecordingEngine:
    """A slot engine that finishes every request after its first decode chunk; ``with_kw``: its
    admit / decode take ``sampling``."""

    def __init__(self, with_kw: bool):
        self.max_batch, self.max_length = 2, 8
        self.cfg = SimpleNamespace(eos_token_id=0)
        self.calls = []
        self.seqs = {}
        self.fin = [1, 1]
        if with_kw:
            self.admit = lambda prompts, slots, penalty, sampling=None: self._admit(prompts, slots, sampling)
            self.decode = lambda B, steps, penalty, sampling=None: self._decode(B, sampling)
        else:
            self.admit = lambda prompts, slots, penalty: self._admit(prompts, slots, "absent")
            self.decode = lambda B, steps, penalty: self._decode(B, "absent")

    def _admit(self, prompts, slots, sampling):
        self.calls.append(("admit", sampling))
        for p, s in zip(prompts, slots):
            self.seqs[s], self.fin[s] = list(p) + [5], 0

    def _decode(self, B, sampling):
        self.calls.append(("decode", sampling))
        for s in range(B):
            self.fin[s] = 1

    def finished_flags(self, B):
        return self.fin[:B]

    def collect(self, slots):
        return [self.seqs[s] for s in slots]


def test_batcher_forwards_sampling_only_when_set():
    sp = SamplingParams(0.7, 50, 0.9, 4)
    eng = _RecordingEngine(with_kw=True)
    cb = ContinuousBatcher(eng, 1.2, sampling=sp)
    try:
        assert cb.submit([1, 2]).result(10) == [1, 2, 5]
    finally:
        cb.stop()
    assert eng.calls and all(s is sp for _, s in eng.calls) and {c for c, _ in eng.calls} == {"admit", "decode"}
    eng = _RecordingEngine(with_kw=False)  # an engine without the keyword, called exactly as before
    cb = ContinuousBatcher(eng, 1.2)
    try:
        assert cb.submit([1, 2]).result(10) == [1, 2, 5]
    finally:
        cb.stop()
    assert eng.calls and all(s == "absent" for _, s in eng.calls)


def test_tutor_cli_builds_the_params():
    from distributed_lms_raft_llm_amd.tutor.server import arg_parser, generation_config, sampling_from_args

    assert sampling_from_args(arg_parser().parse_args([])) is None
    assert sampling_from_args(arg_parser().parse_args(["--sample"])) == SamplingParams(0.7, 50, 0.9, 0)
    sp = sampling_from_args(arg_parser().parse_args(
        ["--sample", "--temperature", "1.1", "--top-k", "40", "--top-p", "0.95", "--seed", "12"]))
    assert sp == SamplingParams(1.1, 40, 0.95, 12)
    with pytest.raises(ValueError):
        sampling_from_args(arg_parser().parse_args(["--sample", "--top-k", "0"]))
    assert generation_config(150, 1.2, sp).sampling() == sp and generation_config(150, 1.2).sampling() is None


def test_tutor_cli_refuses_sampling_on_tp_or_fp8(capsys):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import sampling_unsupported
    from distributed_lms_raft_llm_amd.tutor.server import main

    assert sampling_unsupported(1, False) is None
    for argv, why in ((["--sample", "--tp", "2"], sampling_unsupported(2, False)),
                      (["--sample", "--weight-dtype", "fp8"], sampling_unsupported(1, True))):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and why in " ".join(capsys.readouterr().err.split())
