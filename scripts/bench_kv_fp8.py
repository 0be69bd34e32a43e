#!/usr/bin/env python3
"""What does the fp8 (e4m3) KV cache buy?  Per operating point two engines of ONE config, differing
only in ``kv_dtype``, alternate ``generate`` calls (``--runs`` each); tokens/s and decode ms per
generation are reported with their spread, plus the share of generated positions at which the two
engines' greedy tokens agree -- one JSON line per point:

  1024 queries (32 -> 150), 512 queries (32 -> 150), 256 queries with max_length 1024 (32 -> 1024:
  the long-cache point, where attention dominates the step).

``--kernels``: also the two decode attention kernels alone (one wave per (row, head) pair, and the
persistent grid of the overlapped step) at 512 rows x 12 heads, kvlen 150 and 1024, bf16 against
fp8 cache, in us and achieved TB/s of K/V bytes; the caches rotate over enough copies to stay out
of the 256 MB last-level cache, as the 12 layers of a decode step do.
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

PROMPT_LEN, PENALTY = 32, 1.2
POINTS = {"q1024": (1024, 150), "q512": (512, 150), "long256": (256, 1024)}


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "all": [round(x, 3) for x in xs]}


def timed(eng, prompts):
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import GenerateStats

    st = GenerateStats()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = eng.generate(prompts, repetition_penalty=PENALTY, stats=st)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return out, ms, st.decode_ms, sum(len(o) - PROMPT_LEN for o in out)


def bench_point(name: str, runs: int) -> dict:
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    queries, max_length = POINTS[name]
    cfg = gpt2_config("gpt2")
    w = init_gpt2_weights(cfg, seed=0)
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size - 1, (queries, PROMPT_LEN), generator=g).tolist()
    engines = {kv: HipGPT2Engine(cfg, w, max_batch=queries, max_length=max_length, kv_dtype=kv) for kv in ("bf16", "fp8")}
    outs = {}
    for kv, eng in engines.items():  # graph captures
        outs[kv] = timed(eng, prompts)[0]
    res = {kv: {"ms": [], "decode_ms": [], "tok_s": []} for kv in engines}
    for _ in range(runs):
        for kv, eng in engines.items():
            out, ms, dec, n = timed(eng, prompts)
            assert out == outs[kv], "greedy generation is not reproducible"
            res[kv]["ms"].append(ms)
            res[kv]["decode_ms"].append(dec)
            res[kv]["tok_s"].append(n / ms * 1e3)
    same = total = 0
    for a, b in zip(outs["bf16"], outs["fp8"]):
        n = max(len(a), len(b)) - PROMPT_LEN
        total += n
        same += sum(x == y for x, y in zip(a[PROMPT_LEN:], b[PROMPT_LEN:]))
    line = {"point": name, "queries": queries, "prompt_len": PROMPT_LEN, "max_length": max_length, "runs": runs,
            "kv_cache_gb": {kv: round(e.kv_cache_bytes() / 2 ** 30, 3) for kv, e in engines.items()},
            "token_agreement": round(same / max(1, total), 4), "positions": total}
    for kv in engines:
        line[kv] = {k: spread(v) for k, v in res[kv].items()}
    line["fp8_over_bf16_tok_s"] = round(line["fp8"]["tok_s"]["median"] / line["bf16"]["tok_s"]["median"], 4)
    line["fp8_over_bf16_decode_ms"] = round(line["fp8"]["decode_ms"]["median"] / line["bf16"]["decode_ms"]["median"], 4)
    for e in engines.values():
        e.close()
    return line


def bench_kernels(iters: int) -> list[dict]:
    import torch

    from distributed_lms_raft_llm_amd import ops

    dev, R, H = "cuda", 512, 12
    lines = []
    for kvlen in (150, 1024):
        copies = 4 if kvlen == 150 else 2
        q = torch.randn(R, H * 64, device=dev).bfloat16()
        slot = torch.randperm(R, device=dev).to(torch.int32)
        kvl = torch.full((R,), kvlen, dtype=torch.int32, device=dev)
        out = torch.empty(R, H * 64, dtype=torch.bfloat16, device=dev)
        for kv in ("bf16", "fp8"):
            caches = []
            for _ in range(copies):
                k = torch.randn(R, H, kvlen, 64, device=dev).bfloat16()
                v = torch.randn(R, H, kvlen, 64, device=dev).bfloat16()
                caches.append((k.to(ops.FP8), v.to(ops.FP8)) if kv == "fp8" else (k, v))
            nbytes = 2 * R * H * kvlen * 64 * caches[0][0].element_size()
            for impl, kw in (("wave", {}), ("persist", {"blocks": 768})):
                def run(n):
                    for i in range(n):
                        k, v = caches[i % copies]
                        ops.row_attention(q, k, v, slot, kvl, out=out, impl=impl, **kw)
                run(2 * copies)
                us = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run(iters)
                    e1.record()
                    torch.cuda.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3 / iters)
                m = statistics.median(us)
                lines.append({"kernel": impl, "kv_dtype": kv, "rows": R, "heads": H, "kvlen": kvlen,
                              "us": spread(us), "kv_mbytes": round(nbytes / 1e6, 1),
                              "tb_per_s": round(nbytes / (m * 1e-6) / 1e12, 3)})
            del caches
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-iters", type=int, default=48)
    args = ap.parse_args()
    for p in args.points:
        print(json.dumps(bench_point(p, args.runs)), flush=True)
    if args.kernels:
        for line in bench_kernels(args.kernel_iters):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
