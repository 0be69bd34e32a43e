"""fp8 KV cache on the latency / mid-batch decode paths, the CPU-checkable side: the prompt pool
of the GPU engine tests (kv_fp8_latency_cases.py) clears the decisive-share floor on the reference
alone, and the tutor passes ``latency_path`` through.

Measured here (``GPT2Reference(kv_dtype="fp8")`` on its own generations, T = 48, penalty 1.2, eps
0.25): every one of the 37 prompts is decisive at >= 80 % of its positions; the batches of 1, 2, 3,
8, 9, 17, 33 and 64 rows are 88.7-93.2 % decisive; no prompt reaches EOS."""
import functools

import torch

import kv_fp8_cases as kc
import kv_fp8_latency_cases as lc
from distributed_lms_raft_llm_amd.engine.gpt2_engine import TorchGPT2Engine
from distributed_lms_raft_llm_amd.models.gpt2 import teacher_forced_check_batch


@functools.lru_cache(maxsize=None)
def _pool_results():
    cfg, w = kc.setup("gpt2")
    prompts = lc.pool(cfg)
    eng = TorchGPT2Engine(cfg, w, max_length=lc.T, kv_dtype="fp8")
    outs = eng.generate(prompts, repetition_penalty=1.2)
    res = teacher_forced_check_batch(eng.model, outs, [len(p) for p in prompts], 1.2, kc.KV_FP8_EPS["gpt2"])
    return cfg, prompts, outs, res


def test_prompt_pool_is_37_distinct_prompts_of_all_eight_lengths():
    cfg, prompts, _, _ = _pool_results()
    assert len(prompts) == 37 and len({tuple(p) for p in prompts}) == 37
    assert {len(p) for p in prompts} == set(lc.PATTERN)
    assert lc.batch(cfg, 64)[37:] == prompts[:27] and lc.batch(cfg, 3) == prompts[:3]


def test_prompt_pool_clears_the_decisive_floor_on_the_reference_alone():
    cfg, prompts, outs, res = _pool_results()
    shares = []
    for p, o, r in zip(prompts, outs, res):
        assert o[: len(p)] == p and len(o) == lc.T and cfg.eos_token_id not in o[len(p):]  # no prompt reaches EOS
        assert not r["mismatches"] and r["positions"] == lc.T - len(p)
        shares.append(r["decisive"] / r["positions"])
    print("per-prompt decisive shares:", " ".join(f"{s:.3f}" for s in shares))
    assert min(shares) >= lc.MIN_PROMPT_SHARE, shares
    for n in lc.BATCHES:
        rows = [res[i % len(res)] for i in range(n)]
        share = sum(r["decisive"] for r in rows) / sum(r["positions"] for r in rows)
        print(f"batch {n}: {share:.3f} decisive")
        assert share >= lc.MIN_BATCH_SHARE, (n, share)


def test_tutor_cli_latency_path():
    from distributed_lms_raft_llm_amd.tutor.server import arg_parser, make_engine

    assert arg_parser().parse_args([]).latency_path == "auto"
    assert arg_parser().parse_args(["--latency-path", "on"]).latency_path == "on"
    assert arg_parser().parse_args(["--kv-dtype", "fp8", "--latency-path", "off"]).latency_path == "off"
    eng = make_engine("gpt2-tiny", "cpu", 4, 24, kv_dtype="fp8", latency_path=True)
    assert isinstance(eng, TorchGPT2Engine) and eng.model.kv_dtype == "fp8"
    ref = make_engine("gpt2-tiny", "cpu", 4, 24, kv_dtype="fp8")
    p = kc.prompts(eng.cfg, [4, 9])
    assert eng.generate(p) == ref.generate(p)  # the torch engine is unchanged by the argument
    assert torch.equal(eng.model.w["transformer.wte.weight"], ref.model.w["transformer.wte.weight"])
