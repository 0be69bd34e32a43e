"""Shared by tests/test_kv_fp8_latency_cpu.py and tests/test_kv_fp8_latency_gpu.py: the prompts the
fp8-KV-cache engine tests of the latency / mid-batch decode paths run.

The 70 % floor of decisive positions (kv_fp8_cases.MIN_DECISIVE) is fragile for arbitrary small
prompt sets at GPT-2-124M's eps 0.25: the first two prompts of the 5 / 20 / 11 / 1 / 30 / 8 / 16 / 2
pattern alone sit at 71.8 %, and other seeds and subsets fall to 44-66 %.  So the batches are drawn
from 37 prompts of that pattern (seed 1, weights ``kc.setup("gpt2")``) chosen on the CPU from the
reference alone: with ``GPT2Reference(kv_dtype="fp8")`` on its own generations (T = 48, penalty
1.2, eps 0.25) each of them is decisive at >= 80 % of its positions, the first n of them (cycled
past 37) are 88.7-93.2 % decisive for n in {1, 2, 3, 8, 9, 17, 33, 64}, and none reaches EOS.
tests/test_kv_fp8_latency_cpu.py recomputes these shares without the code under test.
"""
import kv_fp8_cases as kc

PATTERN = [5, 20, 11, 1, 30, 8, 16, 2] * 8
KEEP = [0, 2, 4, 6, 8, 9, 10, 12, 14, 17, 18, 20, 21, 22, 23, 26, 28, 30, 31, 32, 33, 34, 36, 37, 38, 40, 44, 46, 49,
        50, 52, 53, 54, 57, 58, 59, 60]
T = 48
BATCHES = [1, 2, 3, 8, 9, 17, 33, 64]  # engine test; the graph, sampling and checked-build tests use 1, 3, 9, 17
MIN_PROMPT_SHARE = 0.8
MIN_BATCH_SHARE = 0.85


def pool(cfg):
    """The 37 prompts (all eight lengths of the pattern)."""
    all64 = kc.prompts(cfg, PATTERN)
    return [all64[i] for i in KEEP]


def batch(cfg, n):
    """A batch of n rows: the first n prompts of the pool, cycling past 37."""
    p = pool(cfg)
    return [p[i % len(p)] for i in range(n)]
