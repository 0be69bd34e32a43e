#!/usr/bin/env python3
"""What does the fork buy?  On ONE engine per point, ``generate`` calls of 32-token prompts to 150
tokens with ``sampling=`` and ``logprobs=True`` alternate between (a) ``forked``: ``n=k``, one prefill
per prompt and ``ops.kv_fork`` into the k - 1 siblings, and (b) ``repeated``: every prompt listed k
times, the only way to get k completions without it -- the same streams, so the same draws.  ``--runs``
each; the medians of the prefill ms, the decode ms (device events, ``GenerateStats``) and of the
wall-clock tok/s are reported: one JSON line per point, by default (256 prompts, n = 4), (128, 8) and
(8, 4).

``--fork``: also the ``ops.kv_fork`` launch alone at 768 children of 32 keys on a 1024-slot cache
(the (256, 4) point's fork), in us and GB/s (bytes read plus bytes written) -- one JSON line.
``--out``: append the lines to that file as well.
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
COPY_RATE_TBS = 6.29  # the measured HBM copy rate the roofline in VERDICT.md uses


def make_engine(slots: int):
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    cfg = gpt2_config("gpt2")
    return cfg, HipGPT2Engine(cfg, init_gpt2_weights(cfg, seed=0), max_batch=slots, max_length=MAX_LENGTH)


def timed(eng, prompts, k: int, sp, forked: bool):
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import GenerateStats

    st = GenerateStats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if forked:
        toks, _ = eng.generate(prompts, repetition_penalty=PENALTY, sampling=sp, logprobs=True, n=k, stats=st)
        toks = [o for g in toks for o in g]
    else:
        toks, _ = eng.generate([p for p in prompts for _ in range(k)], repetition_penalty=PENALTY, sampling=sp,
                               logprobs=True, stats=st)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return toks, dict(ms=ms, prefill_ms=st.prefill_ms, decode_ms=st.decode_ms,
                      new_tokens=sum(len(o) - PROMPT_LEN for o in toks))


def bench_point(n_prompts: int, k: int, runs: int) -> dict:
    import torch

    from distributed_lms_raft_llm_amd.models.config import SamplingParams

    cfg, eng = make_engine(n_prompts * k)
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size - 1, (n_prompts, PROMPT_LEN), generator=g).tolist()
    sp = SamplingParams(0.7, 50, 0.9, 7)
    modes = (("forked", True), ("repeated", False))
    outs = {}
    for name, forked in modes:  # graph captures (decode and, at the second sighting, prefill), buffers
        for _ in range(2):
            outs[name], _ = timed(eng, prompts, k, sp, forked)
    rec = {name: [] for name, _ in modes}
    for _ in range(runs):
        for name, forked in modes:
            rec[name].append(timed(eng, prompts, k, sp, forked)[1])
    eng.close()
    out = {"bench": "best_of", "prompts": n_prompts, "n": k, "runs": runs,
           "same_tokens": outs["forked"] == outs["repeated"]}
    for name, _ in modes:
        for f in ("prefill_ms", "decode_ms", "ms"):
            out[f"{name}_{f}"] = round(statistics.median(r[f] for r in rec[name]), 3)
            out[f"{name}_{f}_all"] = [round(r[f], 3) for r in rec[name]]
        out[f"{name}_new_tokens"] = rec[name][-1]["new_tokens"]
        out[f"{name}_tok_s"] = round(statistics.median(r["new_tokens"] / r["ms"] * 1e3 for r in rec[name]), 1)
    out["prefill_ms_saved"] = round(out["repeated_prefill_ms"] - out["forked_prefill_ms"], 3)
    out["tok_s_gain_pct"] = round((out["forked_tok_s"] / out["repeated_tok_s"] - 1) * 100, 2)
    return out


def bench_fork(children: int, keys: int, slots: int, iters: int = 20) -> dict:
    """``ops.kv_fork`` alone on an engine's own cache: ``children`` slots of ``keys`` keys, three per parent
    (n = 4)."""
    import torch

    from distributed_lms_raft_llm_amd import ops

    _, eng = make_engine(slots)
    per = 3
    parents = children // per
    perm = torch.randperm(slots, generator=torch.Generator().manual_seed(2))[: parents + children]
    src = perm[:parents].repeat_interleave(per).to(torch.int32).to(eng.device)
    dst = perm[parents:].to(torch.int32).to(eng.device)
    lens = torch.full((children,), keys, dtype=torch.int32, device=eng.device)
    ops.kv_fork(eng.kv, src, dst, lens)  # (checks the table once)
    for _ in range(5):
        ops.kv_fork(eng.kv, src, dst, lens, host_checked=True)
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ops.kv_fork(eng.kv, src, dst, lens, host_checked=True)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    L, _, _, H, _, hd = eng.kv.shape
    moved = 2 * children * L * 2 * H * keys * hd * eng.kv.element_size()  # read + written
    eng.close()
    med = statistics.median(us)
    gbs = moved / med / 1e3
    return {"bench": "kv_fork", "children": children, "keys": keys, "slots": slots, "us": round(med, 2),
            "us_all": [round(u, 2) for u in us], "mbytes_moved": round(moved / 1e6, 1), "gb_s": round(gbs, 1),
            "pct_of_copy_rate": round(gbs / (COPY_RATE_TBS * 1e3) * 100, 1), "copy_rate_tb_s": COPY_RATE_TBS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", type=str, nargs="+", default=["256x4", "128x8", "8x4"], metavar="PROMPTSxN")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--fork", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    for pt in args.points:
        n_prompts, k = (int(v) for v in pt.lower().split("x"))
        emit(bench_point(n_prompts, k, args.runs))
    if args.fork:
        emit(bench_fork(768, 32, 1024))


if __name__ == "__main__":
    main()
