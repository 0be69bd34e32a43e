#!/usr/bin/env python3
"""What does sampling cost?  On ONE engine per query count, greedy and sampled
(temperature 0.7 / top-k 50 / top-p 0.9) ``generate`` calls of 32-token prompts to 150 tokens
alternate, ``--runs`` each, and the medians are reported -- one JSON line per query count
(1, 32, 1024 by default).

``--kernel-stats DIR``: also one ``rocprofv3 --kernel-trace --stats`` run of a child process (this
script with ``--trace-worker``: a greedy and a sampled generation at ``--trace-queries`` queries)
into DIR, and from its kernel statistics the time per decode step of the sampler kernel and of the
LM heads (the f32-logits one the sampling mode runs, the fused-argmax one of greedy decoding).
The child is started before this process touches the GPU.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
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


def timed(eng, prompts, sampling):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate(prompts, repetition_penalty=PENALTY, sampling=sampling)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, sum(len(o) - PROMPT_LEN for o in out)


def bench(queries: int, runs: int, sp) -> dict:
    eng, prompts = make_engine(queries)
    for mode in (None, sp):  # graph captures, the logits buffer
        timed(eng, prompts, mode)
    ms = {"greedy": [], "sampled": []}
    toks = {}
    for _ in range(runs):
        for name, mode in (("greedy", None), ("sampled", sp)):
            t, n = timed(eng, prompts, mode)
            ms[name].append(t)
            toks[name] = n
    eng.close()
    g, s = statistics.median(ms["greedy"]), statistics.median(ms["sampled"])
    return {"queries": queries, "runs": runs, "greedy_ms": round(g, 3), "sampled_ms": round(s, 3),
            "overhead_pct": round((s / g - 1) * 100, 2), "greedy_ms_all": [round(x, 3) for x in ms["greedy"]],
            "sampled_ms_all": [round(x, 3) for x in ms["sampled"]], "greedy_new_tokens": toks["greedy"],
            "sampled_new_tokens": toks["sampled"],
            "sampling": {"temperature": sp.temperature, "top_k": sp.top_k, "top_p": sp.top_p, "seed": sp.seed}}


def kernel_stats(out_dir: str, queries: int) -> dict:
    """One traced child run; per-launch averages of the sampler and the LM-head kernels."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out_dir, "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--trace-worker", "--trace-queries", str(queries)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        return {"kernel_stats_error": (res.stderr or res.stdout)[-2000:]}
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    out = {"kernel_stats_queries": queries, "kernels": []}
    for r in rows:
        name = r["Name"]
        if "sample_topk_topp" in name or "gemm_ps_kernel" in name or "decode_update" in name:
            out["kernels"].append({"name": name[:120], "calls": int(r["Calls"]),
                                   "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                                   "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", type=int, nargs="+", default=[1, 32, 1024])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    ap.add_argument("--trace-queries", type=int, default=1024)
    ap.add_argument("--trace-worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    stats = kernel_stats(args.kernel_stats, args.trace_queries) if args.kernel_stats else None

    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    sp = SamplingParams(0.7, 50, 0.9, args.seed)
    if args.trace_worker:
        eng, prompts = make_engine(args.trace_queries)
        for mode in (None, sp, None, sp):  # the second pair replays the captured graphs
            timed(eng, prompts, mode)
        eng.close()
        return
    for q in args.queries:
        print(json.dumps(bench(q, args.runs, sp)), flush=True)
    if stats is not None:
        print(json.dumps(stats), flush=True)


if __name__ == "__main__":
    main()
