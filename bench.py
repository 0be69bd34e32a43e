#!/usr/bin/env python3
"""Headline benchmark: tutoring tokens/s for GPT-2-124M (+ p50 query latency) on MI355X.

BASELINE.json metric: "tutoring tokens/sec (GPT-2-124M) + p50 query latency at 1/2/4/8 MI355X".
The reference serves each student query with ``model.generate(max_length=150,
repetition_penalty=1.2)`` (greedy) on CPU: 53.7 tok/s, p50 2198 ms per query.

One benchmark "step" = one batch of concurrent synthetic student queries served end to end by
the tutoring engine: packed prefill of every prompt (32 tokens) + greedy/repetition-penalty
decode up to 150 total tokens, all on the GPU (hipGraph-captured decode steps, hand-written
HIP kernels).  ``ms_per_step`` is therefore the latency of every query in the batch (the p50
query latency); ``value`` is generated tokens/s summed over all GPUs.

Operating point: 1024 concurrent queries per GPU (measured on one MI355X, profiles/r1_bench_lines.jsonl):
512 -> 387k tok/s @ 156 ms, 1024 -> 509k @ 237 ms, 2048 -> 568k @ 426 ms.  1024 keeps every
query ~9x faster than the reference's 2198 ms while the GPU is mostly saturated; the KV slots it
needs (5.3 MiB each) use 5 GB of the 288 GB HBM.

Multi-GPU: one process per GPU (torchrun), data-parallel engine replicas (weak scaling: each GPU
serves its own batch of queries); ``--tp N`` runs tensor-parallel decode over RCCL instead.
Weights are random-init (seeded) GPT-2-124M and prompts are synthetic token ids: no network.

A plain run sets up, warms up, times ``--steps`` steps and prints the result line.  ``--full``
adds the unloaded p50 latency points (``--latency-batches``, keys ``p50_query_latency_ms_b<B>``),
which take generations of their own after the timed steps; ``DLMS_BENCH_FULL=1`` in the environment
is the same switch, for scripts that wrap the benchmark.  ``--dump-outputs DIR`` writes the
token sequences the last timed step returned as ``DIR/*.npy`` (same arguments, same inputs).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BASELINE_TOK_S = 53.7  # reference GPT-2-124M generate on CPU
METRIC = "tutoring tokens/sec (GPT-2-124M) + p50 query latency at 1/2/4/8 MI355X"
# other models (BASELINE configs 3-5) report the same measurement under their own name; the
# published baseline exists for GPT-2-124M in bf16 only, so only that line carries vs_baseline
MODEL_LABELS = {"gpt2": "GPT-2-124M", "gpt2-medium": "GPT-2-medium (355M)", "gpt2-large": "GPT-2-large (774M)",
                "gpt2-xl": "GPT-2-XL (1.5B)"}


def metric_for(model: str) -> str:
    return METRIC.replace("GPT-2-124M", MODEL_LABELS.get(model, model))


def data_for(model: str) -> str:
    """The ``data`` field: synthetic prompts and random-init weights of the benchmarked model."""
    return f"synthetic prompts (random token ids), random-init {MODEL_LABELS.get(model, model)} weights"


def vs_baseline(model: str, weight_dtype: str, tok_s: float):
    return round(tok_s / BASELINE_TOK_S, 1) if model == "gpt2" and weight_dtype == "bf16" else None


def spawn_ranks(n: int) -> int:
    """``--gpus N`` without a launcher: start N ranks of this script as child processes (one per
    GPU, RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* set like torchrun) BEFORE this process touches the
    GPU, wait for all of them and return the first non-zero exit code."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    # poll all ranks: if one dies, the others may block forever in a collective, so terminate
    # (then kill) the rest and return the failing rank's code instead of hanging
    import time

    while True:
        rcs = [p.poll() for p in procs]
        bad = next((rc for rc in rcs if rc not in (None, 0)), None)
        if bad is not None:
            for p in procs:
                if p.poll() is None:
                    p.terminate()
            deadline = time.time() + 10
            for p in procs:
                try:
                    p.wait(timeout=max(0.1, deadline - time.time()))
                except subprocess.TimeoutExpired:
                    p.kill()
                    p.wait()
            return bad
        if all(rc == 0 for rc in rcs):
            return 0
        time.sleep(0.2)


def latency_point(eng, cfg, B: int, prompt_len: int, max_length: int, reps: int, seed: int, gpu: bool) -> dict:
    """p50 wall time of ``reps`` generate() calls of B concurrent queries on an otherwise idle
    engine (after two warmup calls that capture the bucket's hipGraph), and the decode tokens/s."""
    g = torch.Generator().manual_seed(seed)
    prompts = torch.randint(0, cfg.vocab_size - 1, (B, prompt_len), generator=g).tolist()
    from distributed_lms_raft_llm_amd.engine.gpt2_engine import GenerateStats

    for _ in range(2):
        eng.generate(prompts, max_length)
    times, st = [], GenerateStats()
    for _ in range(reps):
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.generate(prompts, max_length, stats=st)
        if gpu:
            torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    p50 = statistics.median(times)
    return {f"p50_query_latency_ms_b{B}": round(p50, 3), f"tok_s_b{B}": round(st.new_tokens / (sum(times) / 1e3), 1),
            f"prefill_ms_b{B}": round(st.prefill_ms / reps, 3)}


def dump_outputs(out_dir: str, seqs: list[list[int]], max_length: int, rank: int) -> None:
    """What a caller of the timed ``generate()`` received in the last timed step, as float32 .npy
    files (token ids are < 2^24, so exact): ``tokens`` is one row per query, prompt + generated
    ids, padded with -1 up to ``max_length``; ``lengths`` is each row's token count.  Rank 0
    writes ``tokens.npy`` / ``lengths.npy``, rank r > 0 ``tokens_rank<r>.npy`` / ``lengths_rank<r>.npy``
    (1024 queries x 150 tokens: 0.6 MB per rank)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    tokens = np.full((len(seqs), max_length), -1.0, dtype=np.float32)
    for i, row in enumerate(seqs):
        tokens[i, : len(row)] = row
    lengths = np.asarray([len(row) for row in seqs], dtype=np.float32)
    tag = "" if rank == 0 else f"_rank{rank}"
    np.save(os.path.join(out_dir, f"tokens{tag}.npy"), tokens)
    np.save(os.path.join(out_dir, f"lengths{tag}.npy"), lengths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--batch", type=int, default=1024, help="concurrent queries per GPU (per TP group)")
    ap.add_argument("--prompt-len", type=int, default=32)
    ap.add_argument("--max-length", type=int, default=150)
    ap.add_argument("--tp", type=int, default=1)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--weight-dtype", choices=("bf16", "fp8"), default="bf16",
                    help="fp8 = W8A8 e4m3 QKV/c_fc/LM head (not the headline: reduced precision)")
    ap.add_argument("--latency-batches", default="1,32",
                    help="with --full, after the timed headline: unloaded p50 latency at these batch sizes ('' = skip)")
    ap.add_argument("--full", action="store_true", default=os.environ.get("DLMS_BENCH_FULL", "0") not in ("", "0"),
                    help="also measure what the headline does not need (the unloaded latency points of "
                         "--latency-batches); a plain run only sets up, warms up and times --steps steps.  "
                         "DLMS_BENCH_FULL=1 in the environment switches it on as well (for wrapper scripts)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (the token sequences of "
                         "every query) as DIR/<name>.npy")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(spawn_ranks(args.gpus))
    if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}")

    from distributed_lms_raft_llm_amd.engine.gpt2_engine import GenerateStats, HipGPT2Engine, TorchGPT2Engine
    from distributed_lms_raft_llm_amd.models.config import gpt2_config
    from distributed_lms_raft_llm_amd.models.gpt2 import init_gpt2_weights

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    gpu = torch.cuda.is_available()
    dist = None
    if world > 1:
        import torch.distributed as dist

        if gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl" if gpu else "gloo", device_id=torch.device(f"cuda:{local_rank}") if gpu else None)
    elif gpu:
        torch.cuda.set_device(0)

    cfg = gpt2_config(args.model)
    weights = init_gpt2_weights(cfg, seed=args.seed)
    tp = args.tp
    if world % tp:
        raise SystemExit("WORLD_SIZE must be a multiple of --tp")
    dp_size = world // tp
    tp_group = None
    if tp > 1:
        groups = [dist.new_group(list(range(g * tp, (g + 1) * tp))) for g in range(dp_size)]
        tp_group = groups[rank // tp]
    dp_rank = rank // tp

    B = args.batch if gpu else min(args.batch, 4)
    if gpu:
        eng = HipGPT2Engine(cfg, weights, max_batch=B, max_length=args.max_length, tp_group=tp_group,
                            weight_dtype=args.weight_dtype,
                            use_graph=not args.no_graph)
    else:
        eng = TorchGPT2Engine(cfg, weights, max_length=args.max_length)
    del weights

    g = torch.Generator().manual_seed(1000 + dp_rank)
    prompts = torch.randint(0, cfg.vocab_size - 1, (B, args.prompt_len), generator=g).tolist()

    def sync():
        if gpu:
            torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    for _ in range(args.warmup):
        eng.generate(prompts, args.max_length)
    sync()

    per_step_ms: list[float] = []
    stats = GenerateStats()
    t0 = time.perf_counter()
    last_out: list[list[int]] = []
    for _ in range(args.steps):
        ts = time.perf_counter()
        last_out = eng.generate(prompts, args.max_length, stats=stats)
        if gpu:
            torch.cuda.synchronize()
        per_step_ms.append((time.perf_counter() - ts) * 1e3)
    sync()
    elapsed = time.perf_counter() - t0

    # tokens generated by this rank's TP group (count once per group: tp rank 0)
    new_tok = stats.new_tokens if (rank % tp == 0) else 0
    t = torch.tensor([elapsed, float(new_tok)], dtype=torch.float64)
    if dist is not None:
        tt = t.cuda() if gpu else t
        el = tt[:1].clone()
        tk = tt[1:].clone()
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        dist.all_reduce(tk, op=dist.ReduceOp.SUM)
        elapsed_max, total_new = float(el.item()), float(tk.item())
    else:
        elapsed_max, total_new = elapsed, float(new_tok)

    tok_s = total_new / elapsed_max
    p50 = statistics.median(per_step_ms)
    if args.dump_outputs is not None:
        dump_outputs(args.dump_outputs, last_out, args.max_length, rank)
    extra = {}
    for lb in [int(b) for b in args.latency_batches.split(",") if b.strip()] if args.full else []:
        if lb <= B:  # outside the timed region: the unloaded latency operating points
            extra.update(latency_point(eng, cfg, lb, args.prompt_len, args.max_length, 5, 2000 + dp_rank, gpu))
    if dist is not None:
        dist.barrier()
    if rank == 0:
        line = {
            "metric": metric_for(args.model),
            "value": round(tok_s, 1) if tok_s >= 100 else round(tok_s, 4),  # (CPU contract runs: < 1 tok/s)
            "unit": "tokens/s",
            "n_gpus": world if gpu else 0,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max * 1e3 / args.steps, 3),
            "higher_is_better": True,
            "scaling": "weak" if tp == 1 else "strong",
            "vs_baseline": vs_baseline(args.model, args.weight_dtype, tok_s),
            "dtype": "bf16" if args.weight_dtype == "bf16" else "fp8-w8a8+bf16",
            "data": data_for(args.model),
            "p50_query_latency_ms": round(p50, 3),
            "baseline_p50_query_latency_ms": 2198,
            "new_tokens_per_step": total_new / args.steps,
            "prefill_ms": round(stats.prefill_ms / max(1, args.steps), 3),  # per generation, this rank
            "decode_ms": round(stats.decode_ms / max(1, args.steps), 3),
            **extra,
            "config": {
                "model": f"{args.model} ({cfg.num_params() / 1e6:.0f}M)",
                "global_batch": B * dp_size,
                "seq_len": args.max_length,
                "prompt_len": args.prompt_len,
                "decode": "greedy + repetition_penalty 1.2, max_length 150 (tutoring_server.py:21-29)",
                "parallelism": f"dp{dp_size}" + (f"_tp{tp}" if tp > 1 else ""),
                "hipgraph": bool(gpu and not args.no_graph),
                "device": torch.cuda.get_device_name(0) if gpu else "cpu",
            },
        }
        print(json.dumps(line), flush=True)
    if hasattr(eng, "close"):
        eng.close()  # graphs, dataflow buffers, xGMI mappings released before interpreter teardown
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
