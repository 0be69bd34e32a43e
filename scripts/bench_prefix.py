#!/usr/bin/env python3
"""What does the prompt-prefix cache buy?  Per operating point three engines of ONE config in one
process -- ``off``: no prefix store; ``fill``: the shared prefix set (``set_prompt_prefix``), suffix-only
prefill and the store copied into the slots, decode reading the slots (``prefix_decode = False``);
``on``: the same with the wave / persistent decode attention reading the shared keys from the store --
alternate ``generate`` calls (``--runs`` each) on the same prompts: ``--shared`` (16) common tokens
followed by 6 random ones -- the tutoring service's shape -- and, as a second line, by 16 random
ones; max_length 150; 1024 and 256 queries.  One JSON line per point: prefill ms, decode ms and
tokens/s as median (min ... max), the share of generated positions at which the two engines'
greedy tokens agree, the prefix counters, and the fill kernel alone (``fill_kernel``:
``ops.kv_prefix_fill`` over that many slots on the engine's own cache, in us).

``--kernels``: ``ops.row_attention`` wave and persistent (768 workgroups) alone at 512 rows x 12
heads, kvlen 86 (the mean decode position of a 150-token answer), with and without
``prefix=`` at P = 16, the caches rotating over 12 copies (one per layer of a decode step) so they
do not sit in the last-level cache; us as median (min ... max) of 5 windows.
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

PENALTY, MAX_LENGTH, CAPACITY = 1.2, 150, 64


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
    return out, ms, st.prefill_ms, st.decode_ms, sum(len(o) - len(p) for o, p in zip(out, prompts))


def fill_us(eng, n: int, P: int, iters: int = 50) -> dict:
    """``ops.kv_prefix_fill`` alone: n slots x P keys of the engine's store into its cache."""
    import torch

    from distributed_lms_raft_llm_amd import ops

    slots = torch.randperm(eng.max_batch, device=eng.device)[:n].to(torch.int32)
    pfx = torch.full((n,), P, dtype=torch.int32, device=eng.device)
    for _ in range(5):
        ops.kv_prefix_fill(eng.kv, eng.pfx_store, slots, pfx)
    us = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ops.kv_prefix_fill(eng.kv, eng.pfx_store, slots, pfx)
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / iters)
    nbytes = eng.pfx_store[:, :, :, :P].numel() * eng.pfx_store.element_size() * n
    return {"us": spread(us), "mbytes_written": round(nbytes / 1e6, 1)}


def bench_point(queries: int, shared: int, suffix: int, runs: int, kv_dtype: str) -> dict:
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    cfg = gpt2_config("gpt2")
    w = init_gpt2_weights(cfg, seed=0)
    g = torch.Generator().manual_seed(1)
    prefix = torch.randint(0, cfg.vocab_size - 1, (shared,), generator=g).tolist()
    prompts = [prefix + s for s in torch.randint(0, cfg.vocab_size - 1, (queries, suffix), generator=g).tolist()]
    kw = dict(max_batch=queries, max_length=MAX_LENGTH, kv_dtype=kv_dtype)
    engines = {"off": HipGPT2Engine(cfg, w, **kw), "fill": HipGPT2Engine(cfg, w, prefix_capacity=CAPACITY, **kw),
               "on": HipGPT2Engine(cfg, w, prefix_capacity=CAPACITY, **kw)}
    engines["fill"].prefix_decode = False  # (ahead of any capture: decode reads the slots)
    for k in ("fill", "on"):
        engines[k].set_prompt_prefix(prefix)
    outs = {k: timed(e, prompts)[0] for k, e in engines.items()}  # decode graph captures
    for k, e in engines.items():  # ... and the prefill graph, captured when a shape is seen again
        assert timed(e, prompts)[0] == outs[k]
    res = {k: {"ms": [], "prefill_ms": [], "decode_ms": [], "tok_s": []} for k in engines}
    for _ in range(runs):
        for k, eng in engines.items():
            out, ms, pre, dec, n = timed(eng, prompts)
            assert out == outs[k], "greedy generation is not reproducible"
            res[k]["ms"].append(ms)
            res[k]["prefill_ms"].append(pre)
            res[k]["decode_ms"].append(dec)
            res[k]["tok_s"].append(n / ms * 1e3)
    same = total = 0
    for a, b, p in zip(outs["off"], outs["on"], prompts):
        total += max(len(a), len(b)) - len(p)
        same += sum(x == y for x, y in zip(a[len(p):], b[len(p):]))
    on = engines["on"]
    line = {"point": f"q{queries}_{shared}+{suffix}", "queries": queries, "shared": shared, "suffix": suffix,
            "max_length": MAX_LENGTH, "kv_dtype": kv_dtype, "runs": runs,
            "token_agreement": round(same / max(1, total), 4), "positions": total,
            "prefix_hits": on.prefix_hits, "prefix_prompts": on.prefix_prompts,
            "prefix_rows_skipped": on.prefix_rows_skipped, "prefix_decode_launches": on.prefix_decode_launches,
            "prefill_rows": {"off": queries * (shared + suffix), "on": queries * suffix}}
    for k in engines:
        line[k] = {m: spread(v) for m, v in res[k].items()}
    assert outs["fill"] == outs["on"], "the store-reading decode attention changed tokens"
    line["fill_prefix_decode_launches"] = engines["fill"].prefix_decode_launches
    for m in ("prefill_ms", "decode_ms", "tok_s"):
        line[f"fill_over_off_{m}"] = round(line["fill"][m]["median"] / line["off"][m]["median"], 4)
        line[f"on_over_off_{m}"] = round(line["on"][m]["median"] / line["off"][m]["median"], 4)
        line[f"on_over_fill_{m}"] = round(line["on"][m]["median"] / line["fill"][m]["median"], 4)
    line["fill_kernel"] = fill_us(on, queries, shared)
    for e in engines.values():
        e.close()
    return line


def bench_kernels(iters: int, R: int = 512, H: int = 12, kvlen: int = 86, P: int = 16, copies: int = 12):
    import torch

    from distributed_lms_raft_llm_amd import ops

    dev, T = "cuda", MAX_LENGTH
    q = torch.randn(R, H * 64, device=dev).bfloat16()
    slot = torch.randperm(R, device=dev).to(torch.int32)
    kvl = torch.full((R,), kvlen, dtype=torch.int32, device=dev)
    out = torch.empty(R, H * 64, dtype=torch.bfloat16, device=dev)
    caches = [(torch.randn(R, H, T, 64, device=dev).bfloat16(), torch.randn(R, H, T, 64, device=dev).bfloat16(),
               torch.randn(H, CAPACITY, 64, device=dev).bfloat16(), torch.randn(H, CAPACITY, 64, device=dev).bfloat16())
              for _ in range(copies)]
    slot_pfx = torch.full((R,), P, dtype=torch.int32, device=dev)
    lines = []
    for impl, kw in (("wave", {}), ("persist", {"blocks": 768})):
        res = {}
        for mode in ("slots", "prefix", "slots", "prefix"):  # alternating, two rounds each
            def run(n):
                for i in range(n):
                    k, v, pk, pv = caches[i % copies]
                    ops.row_attention(q, k, v, slot, kvl, out=out, impl=impl,
                                      prefix=(pk, pv, slot_pfx) if mode == "prefix" else None, **kw)
            run(2 * copies)
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(iters)
                e1.record()
                torch.cuda.synchronize()
                res.setdefault(mode, []).append(e0.elapsed_time(e1) * 1e3 / iters)
        line = {"kernel": impl, "rows": R, "heads": H, "kvlen": kvlen, "prefix": P, "t_max": T,
                "slots_us": spread(res["slots"]), "prefix_us": spread(res["prefix"])}
        line["prefix_over_slots"] = round(line["prefix_us"]["median"] / line["slots_us"]["median"], 4)
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--queries", nargs="+", type=int, default=[1024, 256])
    ap.add_argument("--shared", type=int, default=16)
    ap.add_argument("--suffixes", nargs="+", type=int, default=[6, 16])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kv-dtype", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--kernels", action="store_true", help="also the decode attention kernels alone, prefix= on / off")
    ap.add_argument("--kernel-iters", type=int, default=96)
    args = ap.parse_args()
    for q in args.queries:
        for s in args.suffixes:
            print(json.dumps(bench_point(q, args.shared, s, args.runs, args.kv_dtype)), flush=True)
    if args.kernels:
        for line in bench_kernels(args.kernel_iters):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
