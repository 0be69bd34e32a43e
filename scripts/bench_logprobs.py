#!/usr/bin/env python3
"""What do the log-probabilities cost?  On ONE engine per query count, ``generate`` calls of 32-token
prompts to 150 tokens alternate between three modes -- (a) plain greedy (the fused-argmax LM
head), (b) greedy through the f32-logit path without log-probabilities (controls with
``min_new_tokens=1``, which bans only EOS at the first token: f32 logits, ``logit_bans``, the
sampler at top_k = 1) and (c) ``logprobs=True`` (the f32-logit path plus ``token_logprob``) --
``--runs`` each, and the medians are reported: one JSON line per query count (1, 32, 1024 by
default).  (c) - (b) is what the log-softmax kernel itself adds; (b) - (a) is the f32-logit path.

``--score``: also the time of ``score()`` on ``--score-seqs`` sequences of 150 tokens (the engine's
own greedy outputs), one JSON line.  ``--out``: append the lines to that file as well.
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


def timed(eng, prompts, kw):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate(prompts, repetition_penalty=PENALTY, **kw)
    torch.cuda.synchronize()
    if kw.get("logprobs"):
        out = out[0]
    return (time.perf_counter() - t0) * 1e3, sum(len(o) - PROMPT_LEN for o in out)


def bench(queries: int, runs: int, modes) -> dict:
    eng, prompts = make_engine(queries)
    for _, kw in modes:  # graph captures, the logits and log-probability buffers
        timed(eng, prompts, kw)
    ms = {name: [] for name, _ in modes}
    toks = {}
    for _ in range(runs):
        for name, kw in modes:
            t, n = timed(eng, prompts, kw)
            ms[name].append(t)
            toks[name] = n
    eng.close()
    med = {name: statistics.median(v) for name, v in ms.items()}
    out = {"bench": "logprobs", "queries": queries, "runs": runs}
    for name, _ in modes:
        out[name + "_ms"] = round(med[name], 3)
        out[name + "_ms_all"] = [round(x, 3) for x in ms[name]]
        out[name + "_new_tokens"] = toks[name]
        if name != "greedy":
            out[name + "_overhead_pct"] = round((med[name] / med["greedy"] - 1) * 100, 2)
    out["logprobs_minus_f32_path_ms"] = round(med["logprobs"] - med["f32_path"], 3)
    out["logprobs_minus_f32_path_pct"] = round((med["logprobs"] / med["f32_path"] - 1) * 100, 2)
    return out


def bench_score(seqs: int, runs: int) -> dict:
    import torch

    eng, prompts = make_engine(seqs)
    full = eng.generate(prompts, repetition_penalty=PENALTY)
    eng.score(full)  # the logits buffer, code objects
    ms = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lp = eng.score(full)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    eng.close()
    n = sum(len(v) for v in lp)
    med = statistics.median(ms)
    return {"bench": "score", "sequences": seqs, "tokens_scored": n, "runs": runs, "score_ms": round(med, 3),
            "score_ms_all": [round(x, 3) for x in ms], "scored_tokens_per_s": round(n / med * 1e3, 1),
            "mean_logprob": round(sum(sum(v) for v in lp) / max(1, n), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--score", action="store_true")
    ap.add_argument("--score-seqs", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from distributed_lms_raft_llm_amd.models.config import GenerationControls

    modes = (("greedy", {}), ("f32_path", {"controls": GenerationControls(min_new_tokens=1)}),
             ("logprobs", {"logprobs": True}))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for q in args.queries:
        emit(bench(q, args.runs, modes))
    if args.score:
        emit(bench_score(args.score_seqs, args.runs))


if __name__ == "__main__":
    main()
