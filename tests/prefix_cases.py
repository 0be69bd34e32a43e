"""Shared by tests/test_prefix_cpu.py and tests/test_prefix_gpu.py: the prompts of the prompt-prefix
cache's engine tests.

A prefix of P tokens (P = 16, the tutoring template's shared tokens, and 13, no multiple of
anything) drawn from ``torch.Generator().manual_seed(7)``, then
  - eight prompts that share it, with suffixes of 1 / 5 / 16 / 17 / 20 / 3 / 31 / 9 tokens (one row, a
    whole 16-query tile, one row past it, two tiles),
  - three unrelated prompts of P, 4 and 40 tokens,
  - the bare prefix (nothing left to run: it takes the full path),
  - one prompt that differs from the prefix in its last token only,
at max_length 64.  The oracle is the unchanged fp32 ``GPT2Reference`` under the teacher-forced margin
rule at eps = 0.05 with at least 70 % of the positions decisive, as tests/test_engine_gpu.py holds the
engine to: the tokens of a prefix-cache engine are those of the reference, so no new tolerance
exists.  tests/test_prefix_cpu.py recomputes, from the reference alone, that these prompts clear
the 70 % floor (GPT-2-124M, random init: 500 / 504 = 99.2 % and 536 / 537 = 99.8 % of the positions
for P = 16 / 13; gpt2-tiny 96.2 % / 96.1 %; no mismatch of the reference against itself).
"""
import torch

T = 64
P_VALUES = (16, 13)
SUFFIX_LENS = [1, 5, 16, 17, 20, 3, 31, 9]
EPS = 0.05
MIN_DECISIVE = 0.7
CAPACITY = 32


def prefix_and_prompts(cfg, P, seed=7):
    """(prefix, the 13 prompts in the order of the module docstring)."""
    g = torch.Generator().manual_seed(seed)

    def draw(n):
        return torch.randint(0, cfg.vocab_size - 1, (n,), generator=g).tolist()

    prefix = draw(P)
    prompts = [prefix + draw(n) for n in SUFFIX_LENS]
    prompts += [draw(n) for n in (P, 4, 40)]
    prompts.append(list(prefix))
    prompts.append(prefix[:-1] + [(prefix[-1] + 1) % (cfg.vocab_size - 1)] + draw(6))
    return prefix, prompts


def cycled(prompts, batch):
    return [list(prompts[i % len(prompts)]) for i in range(batch)]
