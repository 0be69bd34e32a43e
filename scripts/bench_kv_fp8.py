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

``--latency``: the low-batch end instead -- 1, 2, 8, 32 and 64 concurrent queries (32 -> 150, greedy,
penalty 1.2), three engines of one config alternating in one process: the fp8 cache on the tiled
step (the default), the fp8 cache with ``latency_path=True`` (latency / mid-batch steps), and the
bf16 cache with the one-row dataflow decode off (``DLMS_DATAFLOW=0``), so that like is compared with
like; ms per generation as median (min ... max) of ``--runs``.  Then the three attention kernels of
those paths alone (split attention at 1 x 12 and 32 x 12 pairs, the fused attention +
out-projection and its head-grouped variant at one row), kvlen 150 and 1024, fp8 against bf16.
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


LATENCY_QUERIES = (1, 2, 8, 32, 64)


def bench_latency_point(queries: int, runs: int, max_length: int = 150) -> dict:
    import torch

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import HipGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    cfg = gpt2_config("gpt2")
    w = init_gpt2_weights(cfg, seed=0)
    g = torch.Generator().manual_seed(1)
    prompts = torch.randint(0, cfg.vocab_size - 1, (queries, PROMPT_LEN), generator=g).tolist()
    kw = dict(max_batch=max(8, queries), max_length=max_length)
    engines = {"fp8_tiled": HipGPT2Engine(cfg, w, kv_dtype="fp8", **kw),
               "fp8_latency": HipGPT2Engine(cfg, w, kv_dtype="fp8", latency_path=True, **kw)}
    df = os.environ.get("DLMS_DATAFLOW")
    os.environ["DLMS_DATAFLOW"] = "0"  # read by the constructor: the bf16 engine runs launch-per-op at one row too
    try:
        engines["bf16_latency"] = HipGPT2Engine(cfg, w, **kw)
    finally:
        if df is None:
            del os.environ["DLMS_DATAFLOW"]
        else:
            os.environ["DLMS_DATAFLOW"] = df
    assert not any(e.dataflow for e in engines.values())
    paths = {k: ("latency" if e._small_ok(queries) else "mid" if e._mid_ok(queries) else "tiled")
             for k, e in engines.items()}
    outs = {k: timed(e, prompts)[0] for k, e in engines.items()}  # decode graph captures
    for k, e in engines.items():  # ... and the prefill graph, captured when a shape is seen again
        assert timed(e, prompts)[0] == outs[k]
    res = {k: {"ms": [], "decode_ms": []} for k in engines}
    for _ in range(runs):
        for k, eng in engines.items():
            out, ms, dec, _ = timed(eng, prompts)
            assert out == outs[k], "greedy generation is not reproducible"
            res[k]["ms"].append(ms)
            res[k]["decode_ms"].append(dec)
    same = total = 0
    for a, b in zip(outs["fp8_tiled"], outs["fp8_latency"]):
        total += max(len(a), len(b)) - PROMPT_LEN
        same += sum(x == y for x, y in zip(a[PROMPT_LEN:], b[PROMPT_LEN:]))
    line = {"point": f"latency_q{queries}", "queries": queries, "prompt_len": PROMPT_LEN, "max_length": max_length,
            "runs": runs, "paths": paths, "fp8_token_agreement_tiled_vs_latency": round(same / max(1, total), 4)}
    for k in engines:
        line[k] = {m: spread(v) for m, v in res[k].items()}
    t, lat = line["fp8_tiled"]["ms"], line["fp8_latency"]["ms"]
    line["fp8_latency_over_tiled_ms"] = round(lat["median"] / t["median"], 4)
    # the dispatch rule: the latency / mid step may be slower than the tiled step of the same tree by
    # at most this point's own run-to-run spread (max - min of the runs)
    line["fp8_latency_slower_by_ms"] = round(lat["median"] - t["median"], 3)
    line["spread_ms"] = round(max(t["max"] - t["min"], lat["max"] - lat["min"]), 3)
    for e in engines.values():
        e.close()
    return line


def bench_latency_kernels(iters: int) -> list[dict]:
    import torch

    from distributed_lms_raft_llm_amd import ops

    dev, H, S = "cuda", 12, 32
    d = H * 64
    lines = []
    wo_sh = ops.shuffle_weight((torch.randn(d, d, device=dev) * 0.05).bfloat16())
    for kvlen in (150, 1024):
        copies = 12  # one cache per layer of a decode step
        caches = {"bf16": [], "fp8": []}
        for _ in range(copies):
            k = torch.randn(S, H, kvlen, 64, device=dev).bfloat16()
            v = torch.randn(S, H, kvlen, 64, device=dev).bfloat16()
            caches["bf16"].append((k, v))
            caches["fp8"].append((k.to(ops.FP8), v.to(ops.FP8)))
        for rows in (1, 32):
            q = torch.randn(rows, d, device=dev).bfloat16()
            slot = torch.randperm(S, device=dev)[:rows].to(torch.int32)
            kvl = torch.full((rows,), kvlen, dtype=torch.int32, device=dev)
            out = torch.empty(rows, d, dtype=torch.bfloat16, device=dev)
            nw, ns = ops.attention_split_geometry(rows * H, kvlen)
            ws = ops.AttnSplitWorkspace(rows * H, ns, dev) if ns > 1 else None
            parts = torch.zeros(H, 4, d, device=dev)
            kernels = {"attention_split": lambda k, v: ops.attention_split(q, k, v, slot, kvl, out=out, waves=nw,
                                                                         splits=ns, workspace=ws)}
            if rows == 1:
                kernels["attention_oproj"] = lambda k, v: ops.attention_oproj(q, k, v, slot, kvl, wo_sh, parts)
                kernels["attention_oproj_grouped"] = lambda k, v: ops.attention_oproj_grouped(q, k, v, slot, kvl, wo_sh,
                                                                                              parts, 3, tiles=3)
            for name, fn in kernels.items():
                for kv in ("bf16", "fp8"):
                    def run(n):
                        for i in range(n):
                            fn(*caches[kv][i % copies])
                    run(copies)
                    us = []
                    for _ in range(5):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run(iters)
                        e1.record()
                        torch.cuda.synchronize()
                        us.append(e0.elapsed_time(e1) * 1e3 / iters)
                    lines.append({"kernel": name, "kv_dtype": kv, "rows": rows, "heads": H, "kvlen": kvlen,
                                  "waves": nw if name == "attention_split" else 4,
                                  "splits": ns if name == "attention_split" else 1, "us": spread(us)})
        del caches
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--points", nargs="+", default=list(POINTS), choices=list(POINTS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--kernel-iters", type=int, default=48)
    ap.add_argument("--latency", action="store_true",
                    help="the low-batch points (fp8 tiled / fp8 latency + mid / bf16) and their attention kernels instead")
    ap.add_argument("--latency-queries", nargs="+", type=int, default=list(LATENCY_QUERIES))
    args = ap.parse_args()
    if args.latency:
        for n in args.latency_queries:
            print(json.dumps(bench_latency_point(n, args.runs)), flush=True)
        if args.kernels:
            for line in bench_latency_kernels(args.kernel_iters):
                print(json.dumps(line), flush=True)
        return
    for p in args.points:
        print(json.dumps(bench_point(p, args.runs)), flush=True)
    if args.kernels:
        for line in bench_kernels(args.kernel_iters):
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
