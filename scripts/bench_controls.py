#!/usr/bin/env python3
"""What do the generation controls cost?  On ONE engine per query count, ``generate`` calls of
32-token prompts to 150 tokens alternate between three modes -- greedy, greedy with
``no_repeat_ngram_size=2`` (f32 logits, ``logit_bans``, the sampler at top_k = 1) and greedy with a
stop sequence that never matches (the stop-checking ``decode_update`` alone) -- ``--runs`` each, and
the medians are reported: one JSON line per query count (1, 32, 1024 by default).

``--kernels``: also the time per call of the ``logit_bans`` kernel at ``--kernel-rows`` rows of
150-token sequences (device events around ``--kernel-calls`` back-to-back launches after a warm-up;
the figure includes the gap between two launches of a stream), for n = 1, 2 and 3.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_LEN, MAX_LENGTH, PENALTY = 32, 150, 1.2


def make_engine(queries: int):
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    cfg = gpt2_config("gpt2")
    eng = HipGPT2Engine(cfg, init_gpt2_weights(cfg, seed=0), max_batch=queries, max_length=MAX_LENGTH)
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size - 1, (queries, PROMPT_LEN), generator=g).tolist()
    return eng, prompts


def timed(eng, prompts, controls):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate(prompts, repetition_penalty=PENALTY, controls=controls)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, sum(len(o) - PROMPT_LEN for o in out)


def bench(queries: int, runs: int, modes) -> dict:
    eng, prompts = make_engine(queries)
    for _, ct in modes:  # graph captures, the logits buffer, the stop table
        timed(eng, prompts, ct)
    ms = {name: [] for name, _ in modes}
    toks = {}
    for _ in range(runs):
        for name, ct in modes:
            t, n = timed(eng, prompts, ct)
            ms[name].append(t)
            toks[name] = n
    eng.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"queries": queries, "runs": runs}
    for name, _ in modes:
        out[name + "_ms"] = round(med[name], 3)
        out[name + "_ms_all"] = [round(x, 3) for x in ms[name]]
        out[name + "_new_tokens"] = toks[name]
        if name != "greedy":
            out[name + "_overhead_pct"] = round((med[name] / med["greedy"] - 1) * 100, 2)
    return out


def kernel_time(rows: int, calls: int) -> dict:
    """Per-call time of logit_bans on ``rows`` live rows of MAX_LENGTH - 1 tokens over a 64-id
    alphabet (repeats in every row), GPT-2's vocabulary."""
    import torch

    from distributed_lms_raft_llm_amd import ops

    dev, vocab, ld = "cuda", 50257, 50304
    g = torch.Generator().manual_seed(2)
    toks = (torch.randint(0, 64, (rows, MAX_LENGTH), generator=g) * 701).to(torch.int32).to(dev)
    lens = torch.full((rows,), MAX_LENGTH - 1, dtype=torch.int32, device=dev)
    fin = torch.zeros(rows, dtype=torch.int32, device=dev)
    plen = torch.full((rows,), PROMPT_LEN, dtype=torch.int32, device=dev)
    z = torch.randn(rows, ld, generator=g).to(dev)
    out = {"kernel": "logit_bans", "rows": rows, "calls": calls, "tokens_per_row": MAX_LENGTH - 1}
    for n in (1, 2, 3):
        for _ in range(10):
            ops.logit_bans(z[:, :vocab], lens, fin, plen, toks, n, 0, vocab - 1, vocab)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            ops.logit_bans(z[:, :vocab], lens, fin, plen, toks, n, 0, vocab - 1, vocab)
        e1.record()
        e1.synchronize()
        out[f"n{n}_us_per_call"] = round(e0.elapsed_time(e1) * 1e3 / calls, 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-rows", type=int, default=512)
    ap.add_argument("--kernel-calls", type=int, default=2000)
    args = ap.parse_args()

    from distributed_lms_raft_llm_amd.models.config import GenerationControls

    # (token ids past the vocabulary's last id are never generated: the stop never matches)
    modes = (("greedy", None), ("no_repeat_2", GenerationControls(no_repeat_ngram_size=2)),
             ("stop_never", GenerationControls(stop=((2 ** 31 - 1, 2 ** 31 - 2),))))
    for q in args.queries:
        print(json.dumps(bench(q, args.runs, modes)), flush=True)
    if args.kernels:
        print(json.dumps(kernel_time(args.kernel_rows, args.kernel_calls)), flush=True)


if __name__ == "__main__":
    main()
